"""numpy / plain Python twin of MSA dense stereo, written from the reference's Thirdparty/MB/MSA.cpp and
ctmf.c:222-320 read as DEFINITIONS - not from oracle/orc_msa.c and not from the kernels: gray (:42-47), `gradient` with both
offsets (:65-76, :118-138), `getCost` (:78-108), the clamped median, `TreeDp` (:929-990), `WTA` (:992-1006), `LRcheck`
(:1027-1105), `output` (:1107-1124), `setExp` (:1126-1130) and `solve` (:1132-1169) glued from those.  The graph stages that make
the aggregation trees (:141-926) stay out: `solve` takes the two trees as arguments.

Arithmetic is float64 and values are stored as float32 exactly where the reference stores `float` (the cost volumes, costUp,
costA).  The loop over the disparities is a numpy axis wherever its iterations do not depend on each other (getCost's first nest,
TreeDp, LRcheck's rewrite); the dependent one - the right volume's `pR[j][d] = pR[j][d - 1]` chain - is the literal scalar loop.

Every rule with a plausible wrong neighbour is a switch of `Rules`, so that a test can show a named case tells the rule from that
neighbour (the mutant table of tests/test_msa_cpu.py).  The defaults are the reference's rules."""
import math

import numpy as np


class Rules:
    """The reference's rules; each keyword names the neighbour a mutant takes instead."""

    def __init__(self, **kw):
        self.dp_children_reversed = False    # a node's children added last to first
        self.dp_round_product = False        # w * up[v] rounded to float before it is added
        self.dp_one_minus_w_sq = False       # (1 - w) * (1 - w) where 1 - w * w belongs
        self.refine_o_not_halved = False     # setExp(o) instead of setExp(o / 2) before the refinement
        self.wta_last = False                # the last minimum (scan from the top)
        self.wta_le = False                  # `<=`: a later equal value replaces the minimum
        self.lr_dd_ge0 = False               # d >= 0 instead of d > 0
        self.lr_j_gt = False                 # j - d > 0 instead of j - d >= 0
        self.lr_tol1 = False                 # |d - d2| <= 1 instead of == 0
        self.occ_left_col0 = False           # left of the image: the LEFT image's first pixel of the row instead of the right one's
        self.costR_clamp0 = False            # past the right border: disparity 0's value instead of the previous disparity's
        self.col_cap8 = False                # colour term capped at 8 instead of 7
        self.gra_cap_before_abs = False      # abs(min(difference, 2)) instead of min(abs(difference), 2)
        self.gray_no_half = False            # gray without + 0.5
        self.border_grad_halved = False      # the one-sided border differences times 0.5 as well
        self.median_rank_off = False         # rank 2r^2 + 2r + 1 instead of 2r^2 + 2r
        self.scale_saturate = False          # d * scale saturated at 255 instead of wrapped into the byte
        for k, v in kw.items():
            if not hasattr(self, k):
                raise TypeError("no rule %r" % k)
            setattr(self, k, v)


CONTRACT = Rules()


# ---- MSA::init ------------------------------------------------------------------------------------------------------------------------
def gray(bgr, rules=CONTRACT):
    """:42-47 - (int)(0.299 R + 0.587 G + 0.114 B + 0.5), stored in a byte"""
    b = np.asarray(bgr, np.uint8).astype(np.float64)
    v = 0.299 * b[..., 2] + 0.587 * b[..., 1] + 0.114 * b[..., 0]
    if not rules.gray_no_half:
        v = v + 0.5
    return v.astype(np.int64).astype(np.uint8)


def gradient(img, along_rows=True, offset=127.5, rules=CONTRACT):
    """:65-76 (offset 127.5, along a row) and :118-138 (offset 0, along a row and along a column): (next - previous) * 0.5 inside,
    next - this at the first position, this - previous at the last."""
    f = np.asarray(img, np.uint8).astype(np.float64)
    if not along_rows:
        f = f.T
    g = np.empty_like(f)
    edge = 0.5 if rules.border_grad_halved else 1.0
    g[:, 1:-1] = (f[:, 2:] - f[:, :-2]) * 0.5 + offset
    g[:, 0] = (f[:, 1] - f[:, 0]) * edge + offset
    g[:, -1] = (f[:, -1] - f[:, -2]) * edge + offset
    return np.ascontiguousarray(g if along_rows else g.T)


def get_cost(bgrL, bgrR, graL, graR, disp, rules=CONTRACT):
    """:78-108 - the two loop nests.  costL[i][j][d] from pixel j of the left and j - d of the right row, or the right row's
    FIRST pixel (`occ`) when j - d < 0; then costR[i][j][d] = costL[i][j + d][d] while j + d < m, else costR[i][j][d - 1]."""
    L = np.asarray(bgrL, np.uint8).astype(np.int64)
    R = np.asarray(bgrR, np.uint8).astype(np.int64)
    n, m = L.shape[:2]
    costL = np.zeros((n, m, disp), np.float32)
    ds = np.arange(disp)
    cap_col = 8.0 if rules.col_cap8 else 7.0
    for i in range(n):
        for j in range(m):
            src = np.where(j - ds >= 0, j - ds, 0)
            gR, cR = graR[i, src], R[i, src]
            if rules.occ_left_col0:
                out = j - ds < 0
                gR = np.where(out, graL[i, 0], gR)
                cR = np.where(out[:, None], L[i, 0][None, :], cR)
            dg = graL[i, j] - gR
            dg = np.abs(np.minimum(dg, 2.0)) if rules.gra_cap_before_abs else np.minimum(np.abs(dg), 2.0)
            dc = np.minimum(np.abs(L[i, j][None, :] - cR).sum(1) / 3, cap_col)
            costL[i, j] = (0.11 * dc + (1 - 0.11) * dg).astype(np.float32)
    pL = costL.tolist()
    pR = [[[0.0] * disp for _ in range(m)] for _ in range(n)]
    for i in range(n):
        for j in range(m):
            row = pR[i][j]
            for d in range(disp):
                if j + d < m:
                    row[d] = pL[i][j + d][d]
                else:
                    row[d] = row[0] if rules.costR_clamp0 else row[d - 1]
    return costL, np.array(pR, np.float32).reshape(n, m, disp)


def cost_right_closed_form(costL):
    """What the product computes instead of the chain: costR[i][j][d] = costL[i][j + d'][d'], d' = min(d, m - 1 - j)."""
    n, m, disp = costL.shape
    j = np.arange(m)[:, None]
    dd = np.minimum(np.arange(disp)[None, :], m - 1 - j)
    return np.ascontiguousarray(costL[:, j + dd, dd])


def median_clamped(a, r, rules=CONTRACT):
    """ctmf.c:222-320 as a definition: per channel the element of rank 2r^2 + 2r of the (2r + 1)^2 window, rows and columns
    replicated at the borders."""
    a = np.asarray(a, np.uint8)
    H, W = a.shape[:2]
    p = np.pad(a, ((r, r), (r, r)) + ((0, 0),) * (a.ndim - 2), mode="edge")
    st = np.stack([p[dy:dy + H, dx:dx + W] for dy in range(2 * r + 1) for dx in range(2 * r + 1)], 0)
    return np.sort(st, 0)[2 * r * r + 2 * r + (1 if rules.median_rank_off else 0)]


def init(bgrL, bgrR, disp, rules=CONTRACT):
    """:22-63 - what svo_msa_init returns, under the same names"""
    gL, gR = gray(bgrL, rules), gray(bgrR, rules)
    graL, graR = gradient(gL, True, 127.5, rules), gradient(gR, True, 127.5, rules)
    costL, costR = get_cost(bgrL, bgrR, graL, graR, disp, rules)
    o = dict(costL=costL, costR=costR, grayL=gL, grayR=gR, graL=graL, graR=graR)
    for side, img in (("L", bgrL), ("R", bgrR)):
        m3 = median_clamped(img, 1, rules)
        o["m3" + side] = m3
        o["r_gra" + side] = gradient(gray(m3, rules), True, 0.0, rules)
        o["c_gra" + side] = gradient(gray(m3, rules), False, 0.0, rules)
    return o


# ---- the stages that consume the tree -----------------------------------------------------------------------------------------------------
def exp_table(o):
    """:1126-1130"""
    return np.array([math.exp(-i * 1.0 / o / 255) for i in range(256)], np.float64)


def tree_dp(cost, seq, child_ptr, child, child_c, root, Exp, rules=CONTRACT, keep_up=False):
    """:929-990 - leaves to root `up[u] += w * up[v]` over u's children in child-list order, every `+=` rounded to float; then
    root to leaves A[v] = w * A[u] + (1 - w * w) * up[v], rounded to float once."""
    cost = np.asarray(cost, np.float32)
    up = cost.copy()
    seq = [int(u) for u in seq]
    cp = [int(x) for x in child_ptr]
    ch = [int(x) for x in child]
    w_of = [float(Exp[int(c)]) for c in child_c]

    def edges(u):
        e = range(cp[u], cp[u + 1])
        return reversed(e) if rules.dp_children_reversed else e

    for u in reversed(seq):
        for e in edges(u):
            term = w_of[e] * up[ch[e]].astype(np.float64)
            if rules.dp_round_product:
                term = term.astype(np.float32).astype(np.float64)
            up[u] = (up[u].astype(np.float64) + term).astype(np.float32)
    A = np.zeros_like(up)
    A[root] = up[root]
    for u in seq:
        for e in edges(u):
            v, w = ch[e], w_of[e]
            k = (1 - w) * (1 - w) if rules.dp_one_minus_w_sq else 1 - w * w
            A[v] = (w * A[u].astype(np.float64) + k * up[v].astype(np.float64)).astype(np.float32)
    return (A, up) if keep_up else A


def wta_raw(costA, rules=CONTRACT):
    """:994-1003 - k = 0; for j = 1 .. D - 1: if A[j] < A[k] then k = j"""
    A = np.asarray(costA, np.float32)
    D = A.shape[-1]
    order = range(D - 2, -1, -1) if rules.wta_last else range(1, D)
    k = np.full(A.shape[:-1], D - 1 if rules.wta_last else 0, np.int64)
    best = A[..., D - 1].copy() if rules.wta_last else A[..., 0].copy()
    for j in order:
        c = A[..., j]
        better = c <= best if rules.wta_le else c < best
        k = np.where(better, j, k)
        best = np.where(better, c, best)
    return k.astype(np.uint8)


def wta(costA, n, m, rules=CONTRACT):
    """:992-1006 - the first minimum, then ctmf r = 2 on the map"""
    D = np.asarray(costA).shape[-1]
    return median_clamped(wta_raw(np.asarray(costA, np.float32).reshape(n, m, D), rules), 2, rules)


def lrcheck(d1, d2, D, rules=CONTRACT):
    """:1027-1105 - mask[i][j] = (j - d >= 0 and d > 0 and d == d2[i][j - d]) with d = d1[i][j]; the volume: |k - d| for the masked
    pixels, 0 for every other."""
    d1 = np.asarray(d1, np.uint8)
    d2 = np.asarray(d2, np.uint8)
    n, m = d1.shape
    mask = np.zeros((n, m), np.uint8)
    for i in range(n):
        for j in range(m):
            d = int(d1[i, j])
            if (j - d > 0) if rules.lr_j_gt else (j - d >= 0):
                dif = abs(d - int(d2[i, j - d]))
                if ((d >= 0) if rules.lr_dd_ge0 else (d > 0)) and ((dif <= 1) if rules.lr_tol1 else (dif == 0)):
                    mask[i, j] = 1
    vol = np.abs(np.arange(D)[None, None, :] - d1.astype(np.int64)[:, :, None]).astype(np.float32)
    return np.where(mask[:, :, None] != 0, vol, np.float32(0)), mask


def output(d0, scale, rules=CONTRACT):
    """:1107-1124 - `*p++ = d0[cur++] * scale`: the int product stored in a byte"""
    v = np.asarray(d0, np.uint8).astype(np.int64) * int(scale)
    return (np.minimum(v, 255) if rules.scale_saturate else v & 255).astype(np.uint8)


def solve(bgrL, bgrR, d, scale, treeL, treeR, rules=CONTRACT):
    """:1132-1169.  treeL / treeR: (root, seq, child_ptr, child, child_c) of the left / right image's aggregation tree (what the
    graph stages return for init's m3 / r_gra / c_gra).  Returns every intermediate; "out" is the map."""
    D = d + 1
    n, m = np.asarray(bgrL).shape[:2]
    N = n * m
    o = 0.1
    s = init(bgrL, bgrR, D, rules)
    E = exp_table(o)
    dp = lambda cost, t, Ex: tree_dp(cost.reshape(N, D), t[1], t[2], t[3], t[4], int(t[0]), Ex, rules)
    s["A_R"] = dp(s["costR"], treeR, E)
    s["disp1"] = wta(s["A_R"], n, m, rules)
    s["A_L"] = dp(s["costL"], treeL, E)
    s["disp0_first"] = wta(s["A_L"], n, m, rules)
    s["cost_checked"], s["mask"] = lrcheck(s["disp0_first"], s["disp1"], D, rules)
    E2 = exp_table(o if rules.refine_o_not_halved else o / 2)
    s["A_refined"] = dp(s["cost_checked"], treeL, E2)
    s["disp0"] = wta(s["A_refined"], n, m, rules)
    s["out"] = output(s["disp0"], scale, rules)
    return s
