"""Semi-global block matching (8-bit gray, 5 directions, single pass) restated in numpy from the written contract of
svo_sgbm_* (include/svo.h): the yardstick the device is compared against, bit for bit.

Plain sequential loops over the pixels of each path, vectorised over the disparity axis only, int32 / int64 throughout.
Nothing here is taken from the kernels."""
import numpy as np

P1, P2, CAP = 648, 2592, 63
SW2 = SH2 = 4
UNIQ, DISP12, SPECKLE_WIN, SPECKLE_RANGE = 10, 1, 100, 32
INVALID = -16
DIRS = ((-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0))   # predecessor offsets (dx, dy)


def default_D(height):
    return ((height // 8) + 15) & -16


def sat16(a):
    return np.clip(a, -32768, 32767)


def prefilter(I):
    """G(x, y) = tab(2 (I(x+1,y) - I(x-1,y)) + the same of the rows above and below (clamped)); border columns 63."""
    I = I.astype(np.int32)
    H, W = I.shape
    up = I[np.maximum(np.arange(H) - 1, 0)]
    dn = I[np.minimum(np.arange(H) + 1, H - 1)]
    G = np.full((H, W), CAP, np.int32)
    v = 2 * (I[:, 2:] - I[:, :-2]) + (up[:, 2:] - up[:, :-2]) + (dn[:, 2:] - dn[:, :-2])
    G[:, 1:-1] = np.clip(v, -CAP, CAP) + CAP
    return G


def _minmax(A):
    """Per pixel: the value and the min / max over it and its half-way points to the left and right neighbour."""
    H, W = A.shape
    ul = A.copy(); ur = A.copy()
    ul[:, 1:] = (A[:, 1:] + A[:, :-1]) // 2
    ur[:, :-1] = (A[:, :-1] + A[:, 1:]) // 2
    return np.minimum(A, np.minimum(ul, ur)), np.maximum(A, np.maximum(ul, ur))


def _bt(A, A0, A1, B, B0, B1, D):
    """Birchfield-Tomasi cost of plane pair (A left, B right): H x W x D, zero for x < D."""
    H, W = A.shape
    out = np.zeros((H, W, D), np.int32)
    for d in range(D):
        u, u0, u1 = A[:, D:], A0[:, D:], A1[:, D:]
        v, v0, v1 = B[:, D - d:W - d], B0[:, D - d:W - d], B1[:, D - d:W - d]
        c0 = np.maximum(0, np.maximum(u - v1, v0 - u))
        c1 = np.maximum(0, np.maximum(v - u1, u0 - v))
        out[:, D:, d] = np.minimum(c0, c1)
    return out


def pixel_cost(L, R, D):
    IL, IR = L.astype(np.int32), R.astype(np.int32)
    GL, GR = prefilter(L), prefilter(R)
    g = _bt(GL, *_minmax(GL), GR, *_minmax(GR), D)
    i = _bt(IL, *_minmax(IL), IR, *_minmax(IR), D)
    return g + (i >> 2)


def block_cost(L, R, D):
    """C(x, y, d): 9 x 9 sum of the pixel cost with x clamped to [D, W-1] and y to [0, H-1]; zero for x < D."""
    P = pixel_cost(L, R, D)
    H, W = L.shape
    C = np.zeros((H, W, D), np.int32)
    xs = np.arange(D, W)
    ys = np.arange(H)
    for dy in range(-SH2, SH2 + 1):
        yy = np.clip(ys + dy, 0, H - 1)
        for dx in range(-SW2, SW2 + 1):
            xx = np.clip(xs + dx, D, W - 1)
            C[:, D:] += P[yy][:, xx]
    assert C.max() <= 15309 and C.min() >= 0
    return C


def path_cost(C, D, direction):
    """L_r over the whole image for one direction, pixel by pixel in the order that direction needs."""
    H, W, _ = C.shape
    dx, dy = DIRS[direction]
    Lr = np.zeros((H, W, D), np.int32)
    ys = range(H)                                   # predecessors lie in the row above, or in the same row on the side dx names
    xs = range(W - 1, D - 1, -1) if dx > 0 else range(D, W)
    big = np.int32(1 << 28)
    for y in ys:
        for x in xs:
            px, py = x + dx, y + dy
            if D <= px <= W - 1 and 0 <= py <= H - 1:
                Lp = Lr[py, px]
                m = int(Lp.min())
            else:
                Lp = np.zeros(D, np.int32)
                m = 0
            lo = np.concatenate(([big], Lp[:-1] + P1))
            hi = np.concatenate((Lp[1:] + P1, [big]))
            best = np.minimum(np.minimum(Lp, lo), np.minimum(hi, m + P2))
            v = C[y, x] + best - (m + P2)
            assert v.min() >= -32768 and v.max() <= 32767
            Lr[y, x] = v
    return Lr


def subpixel(S, best, D):
    """disp1 of one pixel from its S vector (python ints) and winning disparity: C division, truncating toward zero."""
    if 0 < best < D - 1:
        den = max(int(S[best - 1]) + int(S[best + 1]) - 2 * int(S[best]), 1)
        num = (int(S[best - 1]) - int(S[best + 1])) * 16 + den
        q = abs(num) // (2 * den)
        return best * 16 + (q if num >= 0 else -q)
    return best * 16


def winner(S, D):
    """disp1 (before the left-right check) and disp2 from the summed volume S (H x W x D)."""
    H, W, _ = S.shape
    disp1 = np.full((H, W), INVALID, np.int32)
    disp2 = np.full((H, W), -1, np.int32)
    dd = np.arange(D)
    for y in range(H):
        cost2 = np.full(W, 1 << 30, np.int64)
        for x in range(W - 1, D - 1, -1):
            s = S[y, x].astype(np.int64)
            best = int(np.argmin(s))                # the first minimum over d ascending
            minS = int(s[best])
            if np.any((np.abs(dd - best) > 1) & (s * (100 - UNIQ) < minS * 100)):   # signed, as written
                continue
            x2 = x - best
            if cost2[x2] > minS:
                cost2[x2] = minS
                disp2[y, x2] = best
            disp1[y, x] = subpixel(s, best, D)
    return disp1, disp2


def lr_check(disp1, disp2):
    H, W = disp1.shape
    out = disp1.copy()
    for y in range(H):
        for x in range(W):
            d1 = int(disp1[y, x])
            if d1 == INVALID:
                continue
            bad = 0
            for a in (d1 >> 4, (d1 + 15) >> 4):
                xa = x - a
                if 0 <= xa < W and disp2[y, xa] >= 0 and abs(int(disp2[y, xa]) - a) > DISP12:
                    bad += 1
            if bad == 2:
                out[y, x] = INVALID
    return out


def speckles(disp, max_size=SPECKLE_WIN, max_diff=16 * SPECKLE_RANGE):
    """4-connected components of valid pixels joined where |difference| <= max_diff; those of <= max_size pixels go."""
    H, W = disp.shape
    out = disp.copy()
    seen = np.zeros((H, W), bool)
    for y0 in range(H):
        for x0 in range(W):
            if seen[y0, x0] or disp[y0, x0] == INVALID:
                continue
            comp = [(y0, x0)]
            seen[y0, x0] = True
            k = 0
            while k < len(comp):
                y, x = comp[k]; k += 1
                v = int(disp[y, x])
                for yy, xx in ((y, x + 1), (y, x - 1), (y + 1, x), (y - 1, x)):
                    if 0 <= yy < H and 0 <= xx < W and not seen[yy, xx] and disp[yy, xx] != INVALID \
                            and abs(int(disp[yy, xx]) - v) <= max_diff:
                        seen[yy, xx] = True
                        comp.append((yy, xx))
            if len(comp) <= max_size:
                for y, x in comp:
                    out[y, x] = INVALID
    return out


def sgbm(L, R, D=None):
    """Every stage of one pair: dict with C, S4, S (H x W x D int16), sum4 and sum5 (the unsaturated int32 sums behind S4 and S: L0 + .. + L3, and S4 + L4), disp2, disp1_raw, disp1_lr, disp16 (int16), disp (float32)."""
    L = np.ascontiguousarray(L, np.uint8); R = np.ascontiguousarray(R, np.uint8)
    H, W = L.shape
    D = default_D(H) if D is None else D
    assert D in (16, 32, 48, 64) and W > D + 8 and H >= 2
    C = block_cost(L, R, D)
    Ls = [path_cost(C, D, k) for k in range(5)]
    S4 = sat16(Ls[0] + Ls[1] + Ls[2] + Ls[3])
    sum5 = S4 + Ls[4]
    S = sat16(sum5)
    S4[:, :D] = 0; S[:, :D] = 0
    raw, disp2 = winner(S, D)
    lr = lr_check(raw, disp2)
    fin = speckles(lr)
    return dict(D=D, sum4=Ls[0] + Ls[1] + Ls[2] + Ls[3], sum5=sum5, C=C.astype(np.int16), S4=S4.astype(np.int16), S=S.astype(np.int16), disp2=disp2.astype(np.int16),
                disp1_raw=raw.astype(np.int16), disp1_lr=lr.astype(np.int16), disp16=fin.astype(np.int16),
                disp=(fin.astype(np.float32) / np.float32(16.0)))
