"""Semi-global block matching on 8UC3 pairs (cn = 3) restated in numpy from the written contract of svo_sgbm_*_bgr
(include/svo.h, DESIGN.md section 8 "f-4 SGBM: colour"): the yardstick the device is compared against, bit for bit.

What differs from the gray contract (tests/sgbm_ref.py) is restated here in full - the planes, the pixel cost, the block sum
kept in a short, the path recurrence with wrapped carries and unwrapped sums; the stages the contract leaves alone (winner,
left-right check, speckles) are the gray restatement's own functions.  Plain sequential loops over the pixels of each path,
vectorised over the disparity axis only, int64 throughout.  Nothing here is taken from the kernels."""
import numpy as np

from sgbm_ref import DIRS, INVALID, default_D, lr_check, sat16, speckles, winner   # noqa: F401  (the unchanged stages)

CN = 3
P1, P2, CAP = 8 * CN * 81, 32 * CN * 81, 63
R = 4                                   # the 9 x 9 block


def wrap16(a):
    """The low 16 bits, sign-extended: what a `short` keeps of an int."""
    return ((np.asarray(a, np.int64) + 32768) & 0xffff) - 32768


def gradient_plane(ch):
    """G_c: clip(2 (I(x+1,y) - I(x-1,y)) + the same of the rows above and below (rows clamped), -63, 63) + 63; border columns 63."""
    I = ch.astype(np.int64)
    H, W = I.shape
    G = np.full((H, W), CAP, np.int64)
    for y in range(H):
        a, b = I[max(y - 1, 0)], I[min(y + 1, H - 1)]
        v = 2 * (I[y, 2:] - I[y, :-2]) + (a[2:] - a[:-2]) + (b[2:] - b[:-2])
        G[y, 1:-1] = np.clip(v, -CAP, CAP) + CAP
    return G


def _lo_hi(A):
    """Per pixel the min and max over the value and its half-way points to the left and right neighbour (none at the borders)."""
    left = A.copy(); right = A.copy()
    left[:, 1:] = (A[:, 1:] + A[:, :-1]) // 2
    right[:, :-1] = (A[:, :-1] + A[:, 1:]) // 2
    return np.minimum(A, np.minimum(left, right)), np.maximum(A, np.maximum(left, right))


def bt(A, B, D):
    """Birchfield-Tomasi cost of the planes A (left) and B (right): H x W x D, zero for x < D."""
    H, W = A.shape
    A0, A1 = _lo_hi(A)
    B0, B1 = _lo_hi(B)
    out = np.zeros((H, W, D), np.int64)
    for d in range(D):
        u, u0, u1 = A[:, D:], A0[:, D:], A1[:, D:]
        v, v0, v1 = B[:, D - d:W - d], B0[:, D - d:W - d], B1[:, D - d:W - d]
        out[:, D:, d] = np.minimum(np.maximum(0, np.maximum(u - v1, v0 - u)), np.maximum(0, np.maximum(v - u1, u0 - v)))
    return out


def pixel_cost(L, Rt, D):
    """sum over the channels of BT(G_c) + (BT(I_c) >> 2): the shift per channel, before the sum.  0 .. 567."""
    H, W, _ = L.shape
    P = np.zeros((H, W, D), np.int64)
    for c in range(CN):
        P += bt(gradient_plane(L[:, :, c]), gradient_plane(Rt[:, :, c]), D)
        P += bt(L[:, :, c].astype(np.int64), Rt[:, :, c].astype(np.int64), D) >> 2
    assert P.min() >= 0 and P.max() <= 567
    return P


def block_sum(L, Rt, D):
    """The true 9 x 9 sum of the pixel cost, x clamped to [D, W-1] and y to [0, H-1]; zero for x < D.  Up to 45 927."""
    P = pixel_cost(L, Rt, D)
    H, W, _ = L.shape
    T = np.zeros((H, W, D), np.int64)
    xs, ys = np.arange(D, W), np.arange(H)
    for dy in range(-R, R + 1):
        rows = P[np.clip(ys + dy, 0, H - 1)]
        for dx in range(-R, R + 1):
            T[:, D:] += rows[:, np.clip(xs + dx, D, W - 1)]
    assert T.min() >= 0 and T.max() <= 81 * 567
    return T


def path_cost(C, D, direction):
    """The unwrapped int32 steps v of one direction over the whole image.  The successor reads them as stored in a short:
    Lp = wrap16(v_prev), m = wrap16(min_d v_prev[d]) - the wrap of the minimum of the unwrapped values."""
    H, W, _ = C.shape
    dx, dy = DIRS[direction]
    V = np.zeros((H, W, D), np.int64)
    xs = range(W - 1, D - 1, -1) if dx > 0 else range(D, W)
    big = 1 << 40
    for y in range(H):
        for x in xs:
            px, py = x + dx, y + dy
            if D <= px <= W - 1 and 0 <= py <= H - 1:
                Lp = wrap16(V[py, px])
                m = int(wrap16(V[py, px].min()))
            else:                                   # a predecessor outside the image: all zeros, m = 0
                Lp = np.zeros(D, np.int64)
                m = 0
            lo = np.concatenate(([big], Lp[:-1] + P1))
            hi = np.concatenate((Lp[1:] + P1, [big]))
            v = C[y, x] + np.minimum(np.minimum(Lp, lo), np.minimum(hi, m + P2)) - (m + P2)
            assert np.abs(v).max() < 1 << 31
            V[y, x] = v
    return V


def sgbm(L, Rt, D=None):
    """Every stage of one 8UC3 pair: sgbm_ref.sgbm's dict (C is wrap16 of the true sum; sum4 = v0 + .. + v3 and sum5 = S4 + v4
    unsaturated) plus Ctrue, the true block sum, and carried_out, the number of steps v (x >= D, all five directions) that
    leave int16 and are therefore carried on wrapped."""
    L = np.ascontiguousarray(L, np.uint8); Rt = np.ascontiguousarray(Rt, np.uint8)
    H, W, cn = L.shape
    assert cn == CN and Rt.shape == L.shape
    D = default_D(H) if D is None else D
    assert D in (16, 32, 48, 64) and W > D + 8 and H >= 2
    Ctrue = block_sum(L, Rt, D)
    C = wrap16(Ctrue)
    V = [path_cost(C, D, k) for k in range(5)]
    sum4 = V[0] + V[1] + V[2] + V[3]
    S4 = sat16(sum4)
    sum5 = S4 + V[4]
    S = sat16(sum5)
    S4[:, :D] = 0; S[:, :D] = 0
    raw, disp2 = winner(S, D)
    lr = lr_check(raw, disp2)
    fin = speckles(lr)
    carried_out = int(sum(((v[:, D:] > 32767) | (v[:, D:] < -32768)).sum() for v in V))
    return dict(D=D, Ctrue=Ctrue.astype(np.int32), carried_out=carried_out, sum4=sum4.astype(np.int32), sum5=sum5.astype(np.int32),
                C=C.astype(np.int16), S4=S4.astype(np.int16), S=S.astype(np.int16), disp2=disp2.astype(np.int16),
                disp1_raw=raw.astype(np.int16), disp1_lr=lr.astype(np.int16), disp16=fin.astype(np.int16),
                disp=(fin.astype(np.float32) / np.float32(16.0)))
