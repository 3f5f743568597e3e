"""Semi-global block matching in its eight-direction, two-pass mode (MODE_HH), gray and 8UC3, restated in numpy from the
written contract (include/svo.h "MODE_HH", DESIGN.md section 8 "f-4 SGBM: MODE_HH"): the yardstick the device is compared
against, bit for bit.

What the mode changes is restated here in full: the eight predecessor offsets, the path recurrence over all of them (with the
colour contract's wrapped carries when cn = 3), and the last sum S = sat16(S4 + v4 + v5 + v6 + v7).  Everything the mode leaves
alone - planes, pixel and block cost, the winner loop, the left-right check, the speckle filter - is the gray and the colour
restatement's own functions.  Plain sequential loops over the pixels of each path, vectorised over the disparity axis only,
int64 throughout.  Nothing here is taken from the kernels."""
import numpy as np

import sgbm_bgr_ref
import sgbm_ref
from sgbm_ref import INVALID, default_D, lr_check, sat16, speckles, winner   # noqa: F401  (the unchanged stages)
from sgbm_bgr_ref import wrap16

MODE_SGBM, MODE_HH = 0, 1
# predecessor offsets (dx, dy): 0 .. 3 the first pass (rows top to bottom, columns left to right), 4 .. 7 the second (rows
# bottom to top, columns right to left).  Only the set of predecessors matters: the steps are summed.
DIRS8 = ((-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1), (0, 1), (-1, 1))
_PEN = {1: (sgbm_ref.P1, sgbm_ref.P2), 3: (sgbm_bgr_ref.P1, sgbm_bgr_ref.P2)}


def path_cost8(C, D, direction, cn=1):
    """The steps v of one of the eight directions over the whole image, pixel by pixel in an order in which every predecessor
    comes first.  cn = 1: the successor reads v itself (it fits a short; asserted).  cn = 3: the successor reads
    Lp = wrap16(v_prev) and m = wrap16(min_d v_prev[d]), and v is the unwrapped int32 step.  A predecessor outside the image
    (x < D included) counts as all zeros with m = 0: both passes start from zeroed buffers."""
    P1, P2 = _PEN[cn]
    H, W, _ = C.shape
    dx, dy = DIRS8[direction]
    V = np.zeros((H, W, D), np.int64)
    ys = range(H - 1, -1, -1) if dy > 0 else range(H)
    xs = range(W - 1, D - 1, -1) if dx > 0 else range(D, W)
    big = 1 << 40
    zero = np.zeros(D, np.int64)
    for y in ys:
        for x in xs:
            px, py = x + dx, y + dy
            if D <= px <= W - 1 and 0 <= py <= H - 1:
                prev = V[py, px]
                Lp, m = (prev, int(prev.min())) if cn == 1 else (wrap16(prev), int(wrap16(prev.min())))
            else:
                Lp, m = zero, 0
            lo = np.concatenate(([big], Lp[:-1] + P1))
            hi = np.concatenate((Lp[1:] + P1, [big]))
            v = C[y, x] + np.minimum(np.minimum(Lp, lo), np.minimum(hi, m + P2)) - (m + P2)
            if cn == 1:
                assert v.min() >= -P2 and v.max() <= 15309      # C <= 15 309 and min(..) - (m + P2) in [-P2, 0]
            else:
                assert np.abs(v).max() < 1 << 31
            V[y, x] = v
    return V


def _finish(D, C, V, extra):
    sum4 = V[0] + V[1] + V[2] + V[3]
    S4 = sat16(sum4)
    sum8 = S4 + V[4] + V[5] + V[6] + V[7]       # one saturation of the second pass's four steps added together
    S = sat16(sum8)
    S4[:, :D] = 0; S[:, :D] = 0
    raw, disp2 = winner(S, D)
    lr = lr_check(raw, disp2)
    fin = speckles(lr)
    out = dict(D=D, sum4=sum4.astype(np.int32), sum5=sum8.astype(np.int32), C=C.astype(np.int16), S4=S4.astype(np.int16),
               S=S.astype(np.int16), disp2=disp2.astype(np.int16), disp1_raw=raw.astype(np.int16), disp1_lr=lr.astype(np.int16),
               disp16=fin.astype(np.int16), disp=(fin.astype(np.float32) / np.float32(16.0)))
    out.update(extra)
    return out


def sgbm_hh(L, R, D=None):
    """Every stage of one gray pair in MODE_HH: sgbm_ref.sgbm's dict, with sum5 holding sum8 = S4 + L4 + L5 + L6 + L7
    (unsaturated), plus second3_max = the largest L5 + L6 + L7 (what an int16 accumulator of three directions would hold)."""
    L = np.ascontiguousarray(L, np.uint8); R = np.ascontiguousarray(R, np.uint8)
    H, W = L.shape
    D = default_D(H) if D is None else D
    assert D in (16, 32, 48, 64) and W > D + 8 and H >= 2
    C = sgbm_ref.block_cost(L, R, D).astype(np.int64)
    V = [path_cost8(C, D, k) for k in range(8)]
    # the ranges the device's accumulators are designed for: two directions fit a short; the sums never leave it on the low side
    for a in range(8):
        for b in range(a + 1, 8):
            two = V[a] + V[b]
            assert two.min() >= -32768 and two.max() <= 2 * 15309 <= 32767
    out = _finish(D, C, V, dict(second3_max=int((V[5] + V[6] + V[7]).max())))
    assert out["sum5"].min() >= -32768 and out["sum4"].min() >= -32768
    return out


def sgbm_hh_bgr(L, Rt, D=None):
    """Every stage of one 8UC3 pair in MODE_HH: sgbm_bgr_ref.sgbm's dict, with sum5 holding sum8 over the unwrapped int32 steps,
    carried_out counting all eight directions, and carried_out_dir the same count per direction."""
    L = np.ascontiguousarray(L, np.uint8); Rt = np.ascontiguousarray(Rt, np.uint8)
    H, W, cn = L.shape
    assert cn == 3 and Rt.shape == L.shape
    D = default_D(H) if D is None else D
    assert D in (16, 32, 48, 64) and W > D + 8 and H >= 2
    Ctrue = sgbm_bgr_ref.block_sum(L, Rt, D)
    C = wrap16(Ctrue)
    V = [path_cost8(C, D, k, cn=3) for k in range(8)]
    per_dir = [int(((v[:, D:] > 32767) | (v[:, D:] < -32768)).sum()) for v in V]
    return _finish(D, C, V, dict(Ctrue=Ctrue.astype(np.int32), carried_out=sum(per_dir), carried_out_dir=per_dir))
