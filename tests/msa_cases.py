"""Hand-made inputs for the MSA stages (csrc/svo_msa.hip), each built to sit on one edge of a kernel or of the host code that picks a
kernel, and each with a `prove` that asserts ON THE TWIN'S DATA ALONE that the edge is reached (tests/test_msa_cpu.py runs every
prove; tests/test_msa_gpu.py holds the device to the twin, tests/msa_ref.py).  All seeded, all small.

The three byte budgets of the aggregation (svo_msa.hip, MsaDpPlan): k_msa_dp_bfs needs lds() = 8 * (256 + 2 * maxw) + 4 * (levels + 2)
bytes of LDS - up to 64 KB without, up to 150 KB with the opt-in - and k_msa_bfs_gather a tile of 64 * (D + 1) * 4 bytes, at most
64 KB.  `lds_bytes` restates the formula; the GPU tests compare it with what the probe reports."""
import functools

import numpy as np

import msa_ref as R

KB64, KB150 = 64 * 1024, 150 * 1024
T_DP = 512         # threads of k_msa_dp_bfs: a level wider than this makes a thread take a second node


def lds_bytes(maxw, levels):
    return 8 * (256 + 2 * maxw) + 4 * (levels + 2)


def gather_tile_bytes(D):
    return 64 * (D + 1) * 4


# ---- trees ----------------------------------------------------------------------------------------------------------------------------
def mixed_costs(rng, N, D):
    """magnitudes 1e-3 .. 1e6, a fifth of them negative: every float rounding of a sum and the order of its terms show in the bytes"""
    c = 10.0 ** rng.uniform(-3, 6, (N, D)) * np.where(rng.random((N, D)) < 0.2, -1.0, 1.0)
    return c.astype(np.float32)


def tree_arrays(kids, root=0, perm=None, weights=None, rng=None, seq_kids=None):
    """kids[u]: u's children in child-list order (node 0 .. N - 1, `root` the root).  Returns (seq, child_ptr, child, child_c) with the
    node ids renamed by `perm` (so that a node's id is neither its position in seq nor in its level).  seq visits level by level;
    inside a level the children of a node follow seq_kids[u] if given (another order than the child list), else the child list."""
    N = len(kids)
    perm = np.arange(N) if perm is None else np.asarray(perm)
    seq, q = [], [root]
    while q:
        nq = []
        for u in q:
            seq.append(u)
            nq += (seq_kids or {}).get(u, kids[u])
        q = nq
    assert len(seq) == N
    inv_kids = [None] * N
    for u in range(N):
        inv_kids[perm[u]] = [int(perm[v]) for v in kids[u]]
    child_ptr = np.zeros(N + 1, np.int32)
    child = []
    for u in range(N):
        child_ptr[u + 1] = child_ptr[u] + len(inv_kids[u])
        child += inv_kids[u]
    child = np.array(child, np.int32).reshape(-1)
    if weights is None:
        weights = rng.integers(0, 256, len(child))
    child_c = np.broadcast_to(np.asarray(weights, np.uint8), (len(child),)).copy()
    return np.array([perm[u] for u in seq], np.int32), child_ptr, child, child_c, int(perm[root])


def level_widths(seq, child_ptr, child, root):
    N = len(seq)
    depth = np.zeros(N, np.int64)
    for u in seq:
        depth[child[child_ptr[u]:child_ptr[u + 1]]] = depth[u] + 1
    return np.bincount(depth).tolist()


def kids_from_widths(widths, max_children=255):
    """A tree whose level l has widths[l] nodes, the children of a level dealt out evenly over the nodes of the level above."""
    kids, prev, nxt = [[]], [0], 1
    for w in widths[1:]:
        cur = list(range(nxt, nxt + w))
        nxt += w
        kids += [[] for _ in cur]
        per = -(-w // len(prev))
        assert per <= max_children, (w, len(prev))
        for k, v in enumerate(cur):
            kids[prev[k // per]].append(v)
        prev = cur
    return kids


class TreeCase:
    def __init__(self, name, kids, D, seed, expect_bfs, os_=(0.1,), root=0, weights=None, cost=None, seq_kids=None, why=""):
        rng = np.random.default_rng(seed)
        N = len(kids)
        perm = rng.permutation(N) if N > 2 else np.arange(N)[::-1].copy()
        self.name, self.D, self.os, self.expect_bfs, self.why = name, D, os_, expect_bfs, why
        self.seq, self.cp, self.ch, self.cc, self.root = tree_arrays(kids, root, perm, weights, rng, seq_kids)
        self.cost = mixed_costs(rng, N, D) if cost is None else cost(rng, N, D)
        self.N = N
        self.widths = level_widths(self.seq, self.cp, self.ch, self.root)
        self.maxw, self.levels = max(self.widths), len(self.widths)
        self.max_children = int(np.diff(self.cp).max())
        self.lds = lds_bytes(self.maxw, self.levels)
        self.proofs = []
        for a in (self.seq, self.cp, self.ch, self.cc, self.cost):
            a.setflags(write=False)

    def args(self):
        return self.cost, self.seq, self.cp, self.ch, self.cc, self.root

    def siblings_in_child_order(self):
        """what msa_bfs_records checks: in level order (by depth, seq order inside a level) every node's children are the next
        positions of the next level, in child-list order"""
        depth = np.zeros(self.N, np.int64)
        for u in self.seq:
            depth[self.ch[self.cp[u]:self.cp[u + 1]]] = depth[u] + 1
        order = self.seq[np.argsort(depth[self.seq], kind="stable")]
        nxt = 1
        for u in order:
            k = self.ch[self.cp[u]:self.cp[u + 1]]
            if not np.array_equal(order[nxt:nxt + len(k)], k):
                return False
            nxt += len(k)
        return True

    def predicted_bfs(self):
        """the decision of MsaDpPlan::decide with the opt-in granted, restated from the case's own numbers"""
        return int(self.lds <= KB150 and gather_tile_bytes(self.D) <= KB64 and self.max_children <= 255 and self.siblings_in_child_order())

    def prove(self):
        assert self.predicted_bfs() == self.expect_bfs, (self.name, self.lds, self.max_children)
        for p in self.proofs:
            p(self)


def path_kids(N):
    return [[u + 1] if u + 1 < N else [] for u in range(N)]


def star_kids(N):
    return [list(range(1, N))] + [[] for _ in range(N - 1)]


def _has(attr, value):
    def p(c):
        assert getattr(c, attr) == value, (c.name, attr, getattr(c, attr), value)
    return p


def _zeros(rng, N, D):
    return np.zeros((N, D), np.float32)


def _small_ints(rng, N, D):
    return rng.integers(0, 256, (N, D)).astype(np.float32)


def random_kids(rng, N, chain=0.3):
    parent = [-1] + [v - 1 if rng.random() < chain else int(rng.integers(0, v)) for v in range(1, N)]
    kids = [[] for _ in range(N)]
    for v in rng.permutation(np.arange(1, N)):
        kids[parent[v]].append(int(v))
    return kids


@functools.lru_cache(maxsize=None)
def tree_cases():
    cs = []

    def add(c, *proofs):
        c.proofs += list(proofs)
        cs.append(c)
        return c

    add(TreeCase("n1", [[]], 5, 1, 1), _has("N", 1), _has("levels", 1))
    add(TreeCase("n2", [[1], []], 4, 2, 1, os_=(0.1, 0.05)), _has("widths", [1, 1]))
    for N in (63, 64, 65):      # the 64-position tiles of k_msa_bfs_gather: one short of a tile, a full tile, one into the next
        add(TreeCase("path%d" % N, path_kids(N), 1 + N % 5, 10 + N, 1), _has("levels", N), _has("maxw", 1))
        add(TreeCase("star%d" % N, star_kids(N), 1 + (N + 2) % 5, 20 + N, 1), _has("widths", [1, N - 1]))
    for n, bfs in ((254, 1), (255, 1), (256, 0), (300, 0)):      # the 8 bits of MsaBfsRec::meta that hold the child count
        add(TreeCase("star_%dch" % n, star_kids(n + 1), 3, 30 + n, bfs), _has("max_children", n))
    # same seed, same node names, same costs and weights per CHILD; only the order of the root's child list is reversed
    rev = TreeCase("star_300ch_reversed", star_kids(301), 3, 330, 0)
    rev.seq, rev.cp, rev.ch, rev.cc = _reverse_root_children(rev)
    add(rev, _has("max_children", 300), _reversal_changes_bytes)
    # the thread stride of k_msa_dp_bfs: levels of 511, 512, 513 and 1,025 nodes - a thread's first node comes from the prefetch,
    # node tid + 512 and tid + 1,024 from the loads in the loop.  (1, 3 lead up to 511: no node may have more than 255 children.)
    add(TreeCase("stride_levels", kids_from_widths([1, 3, 511, 512, 513, 1025, 1]), 4, 41, 1, os_=(0.1, 0.05)),
        _has("widths", [1, 3, 511, 512, 513, 1025, 1]), lambda c: _le(c.max_children, 255))
    # 64 KB of LDS: the opt-in launch.  Three levels: root, inner nodes, one wide level
    for maxw, over in ((3966, False), (3967, True)):
        add(TreeCase("lds64k_maxw%d" % maxw, kids_from_widths([1, 16, maxw]), 3, 50 + over, 1), _has("maxw", maxw), _has("levels", 3),
            (lambda c: _gt(c.lds, KB64)) if over else (lambda c: _le(c.lds, KB64)), lambda c: _le(c.max_children, 255))
    # 150 KB: the widest level, then the level table, push lds() over what the opt-in grants
    for maxw, bfs in ((9470, 1), (9471, 0)):
        add(TreeCase("lds150k_maxw%d" % maxw, kids_from_widths([1, 38, maxw]), 2, 60 + bfs, bfs), _has("maxw", maxw), _has("levels", 3),
            (lambda c: _le(c.lds, KB150)) if bfs else (lambda c: _gt(c.lds, KB150)), lambda c: _le(c.max_children, 255))
    for levels, bfs in ((1886, 1), (1887, 0)):      # a path hanging from one node of the wide level: the fall-back costs 2 x 1,887 launches
        add(TreeCase("lds150k_levels%d" % levels, kids_from_widths([1, 36, 9000] + [1] * (levels - 3)), 2, 70 + bfs, bfs),
            _has("maxw", 9000), _has("levels", levels), (lambda c: _le(c.lds, KB150)) if bfs else (lambda c: _gt(c.lds, KB150)))
    # a valid seq (parents before children, level by level) that lists one node's children in the reverse of its child list
    kids = kids_from_widths([1, 4, 13, 30])
    add(TreeCase("siblings_reversed_in_seq", kids, 5, 80, 0, seq_kids={2: kids[2][::-1]}), lambda c: _le(c.max_children, 255),
        lambda c: _le(c.lds, KB64), _seq_is_valid)
    for w in (0, 255):      # w = Exp[0] = 1: 1 - w * w = 0, a child takes its parent's value; Exp[255]: the smallest weight
        add(TreeCase("weights_all_%d" % w, random_kids(np.random.default_rng(90 + w), 40), 5, 90 + w, 1, os_=(0.1, 0.05), weights=w),
            lambda c, w=w: _eq(set(c.cc.tolist()), {w}))
    for D, bfs in ((1, 1), (255, 1), (256, 0)):      # the gather tile 64 * (D + 1) * 4: exactly 64 KB at D = 255
        add(TreeCase("random3000_D%d" % D, random_kids(np.random.default_rng(100), 3000), D, 100 + D, bfs),
            (lambda c: _le(gather_tile_bytes(c.D), KB64)) if bfs else (lambda c: _gt(gather_tile_bytes(c.D), KB64)),
            lambda c: _le(c.max_children, 255), lambda c: _le(c.lds, KB64))
    add(TreeCase("volume_zero", random_kids(np.random.default_rng(110), 200), 5, 110, 1, cost=_zeros), lambda c: _eq(float(np.abs(c.cost).max()), 0.0))
    add(TreeCase("volume_small_ints", random_kids(np.random.default_rng(111), 200), 5, 111, 1, os_=(0.05,), cost=_small_ints),
        lambda c: _eq(bool((c.cost == np.round(c.cost)).all() and c.cost.max() <= 255 and c.cost.min() >= 0), True))
    return {c.name: c for c in cs}


def _le(a, b):
    assert a <= b, (a, b)


def _gt(a, b):
    assert a > b, (a, b)


def _eq(a, b):
    assert a == b, (a, b)


def _reverse_root_children(c):
    r = c.root
    a, b = int(c.cp[r]), int(c.cp[r + 1])
    ch, cc, seq = c.ch.copy(), c.cc.copy(), c.seq.copy()
    ch[a:b] = ch[a:b][::-1]
    cc[a:b] = cc[a:b][::-1]
    seq[1:] = ch[a:b]
    for x in (ch, cc, seq):
        x.setflags(write=False)
    return seq, c.cp, ch, cc


def _reversal_changes_bytes(c):
    """same children, same weight per child, same costs: only the order of the additions differs, and it reaches the bytes"""
    f = tree_cases()["star_300ch"]
    assert np.array_equal(f.cost, c.cost) and f.root == c.root
    assert dict(zip(f.ch.tolist(), f.cc.tolist())) == dict(zip(c.ch.tolist(), c.cc.tolist())) and f.ch.tolist() == c.ch.tolist()[::-1]
    E = R.exp_table(0.1)
    assert R.tree_dp(*f.args(), E).tobytes() != R.tree_dp(*c.args(), E).tobytes()


def _seq_is_valid(c):
    seen = {c.root}
    for u in c.seq:
        assert int(u) in seen
        seen.update(c.ch[c.cp[u]:c.cp[u + 1]].tolist())
    assert not c.siblings_in_child_order()


# ---- hand-made BGR pairs for MSA::init ------------------------------------------------------------------------------------------------------
def half_triples():
    """BGR triples whose 0.299 R + 0.587 G + 0.114 B is EXACTLY k + 0.5 (299 R + 587 G + 114 B = 1000 k + 500): `+ 0.5` puts the
    double sum on an integer boundary, and which side it lands on is the float evaluation's business.  Found by search."""
    out = []
    for r in range(0, 256, 5):
        for g in range(0, 256, 3):
            for b in range(0, 256):
                if (299 * r + 587 * g + 114 * b) % 1000 == 500:
                    out.append((b, g, r))
    return out


@functools.lru_cache(maxsize=None)
def init_pair(W, H):
    """Left: ramps (3 gray levels per column, channels apart) with a step edge, rows offset.  Right: the left shifted by two columns
    plus per-channel noise of -4 .. 4, so that colour sums and gradient differences around the two caps occur.  Planted where the
    image has room: colour sums of exactly 20, 21, 22 at disparity 0 (row 0, columns 3 .. 5), `.5` gray triples (row 1), and a
    right image whose first pixel of every row differs from the second."""
    rng = np.random.default_rng(1000 * W + H)
    x = np.arange(W + 2)[None, :, None]
    y = np.arange(H)[:, None, None]
    base = 40 + 3 * x + 7 * y + np.array([0, 9, 21])[None, None, :] + 60 * (x > (W + 2) // 2)
    base = (base % 256).astype(np.int64)
    L = base[:, :W].copy()
    Rr = np.clip(base[:, 2:] + rng.integers(-4, 5, (H, W, 3)), 0, 255)
    Rr[:, 0] = np.clip(Rr[:, 1] + np.array([31, -17, 5])[None, :] + y[:, 0], 0, 255)
    Rr[:, 0] = np.where((Rr[:, 0] == Rr[:, 1]).all(1, keepdims=True), 255 - Rr[:, 1], Rr[:, 0])
    if W >= 7:
        for k, s in enumerate((20, 21, 22)):
            L[0, 3 + k] = (100, 110, 120)
            Rr[0, 3 + k] = (100 + 7, 110 - 7, 120 + s - 14)
    if W >= 5 and H >= 2:
        t = half_triples()
        for k in range(1, W - 1):
            L[1, k] = t[(7 * k) % len(t)]
            Rr[1, k] = t[(11 * k + 3) % len(t)]
    L, Rr = np.ascontiguousarray(L, np.uint8), np.ascontiguousarray(Rr, np.uint8)
    L.setflags(write=False)
    Rr.setflags(write=False)
    return L, Rr


INIT_SIZES = [(2, 2), (5, 5), (7, 40), (257, 3), (300, 2)]     # W x H
INIT_DISPS = [1, 6, 49, 256]


@functools.lru_cache(maxsize=None)
def init_twin(W, H, disp):
    L, Rr = init_pair(W, H)
    o = R.init(L, Rr, disp)
    for a in o.values():
        a.setflags(write=False)
    return o


def prove_init(W, H, disp):
    """the edges this size reaches, counted on the twin's intermediates"""
    L, Rr = init_pair(W, H)
    o = init_twin(W, H, disp)
    j = np.arange(W)[:, None]
    d = np.arange(disp)[None, :]
    if disp > 1:
        assert (j - d < 0).any() and (j + d >= W).any()            # the occ branch and the chain are on the path
    if disp > W:
        assert (j - d < 0)[W - 1].any()                            # even the last column looks left of the image
        assert (j + d >= W)[0].any()                               # even the first column's chain runs
    assert (Rr[:, 0] != Rr[:, 1]).any(1).all()                     # occ is not "replicate the neighbour"
    assert (L[:, 0] != Rr[:, 0]).any(1).all()                      # ... nor the left image's column 0
    if W >= 7:
        sums = np.abs(L[0, 3:6].astype(int) - Rr[0, 3:6].astype(int)).sum(1).tolist()
        assert sums == [20, 21, 22]
        c = 0.11 * np.minimum(np.array(sums) / 3, 7.0)
        assert c[0] < c[1] == c[2]                                 # saturates exactly at 21 / 3
        if disp >= 6:
            dif = np.abs(o["graL"][:, :, None] - np.stack([o["graR"][:, np.maximum(np.arange(W) - k, 0)] for k in range(min(disp, W))], 2))
            assert (dif == 2.0).any() and (dif == 1.5).any() and (dif == 2.5).any()      # the gradient cap, exactly and either side
    if W >= 5 and H >= 2:
        for k in range(1, W - 1):
            for img in (L, Rr):
                b, g, r = (int(v) for v in img[1, k])
                assert (299 * r + 587 * g + 114 * b) % 1000 == 500
                lo = (299 * r + 587 * g + 114 * b) // 1000         # the exact sum is lo + 0.5: the byte is lo or lo + 1
                assert int(R.gray(np.array([[b, g, r]], np.uint8))[0]) in (lo, lo + 1)
        assert (R.gray(L) != R.gray(L, R.Rules(gray_no_half=True)))[1, 1:W - 1].any()


# ---- WTA --------------------------------------------------------------------------------------------------------------------------------
def wta_volume(W, H, D=256):
    """Column bands at least five wide (so that the 5 x 5 median keeps them) of: a tie of disparities 0 and D - 1 (the first wins), a
    minimum at D - 1 alone, a strictly decreasing row, a minimum one float ulp below its neighbour at 7 / 8, and a tie of 3 and 4.
    A map five wide is one band of the first kind with a few pixels of the others: its r = 2 window is the whole image."""
    rng = np.random.default_rng(W * 31 + H)
    A = (1.0 + rng.random((H, W, D))).astype(np.float32)
    kind = np.zeros((H, W), np.int64)
    if W >= 25:
        kind[:] = (np.arange(W) // 5 % 5)[None, :]
    elif H >= 25:
        kind[:] = (np.arange(H) // 5 % 5)[:, None]
    else:
        kind[1, 1], kind[2, 3], kind[3, 0], kind[4, 4] = 1, 2, 3, 4
    for (i, j), k in np.ndenumerate(kind):
        if k == 0:
            A[i, j, 0] = A[i, j, D - 1] = 0.5
        elif k == 1:
            A[i, j, D - 1] = 0.25
        elif k == 2:
            A[i, j] = np.linspace(3.0, 1.0, D, dtype=np.float32) if D > 1 else A[i, j]
        elif k == 3 and D > 8:
            A[i, j, 8] = 0.75
            A[i, j, 7] = np.nextafter(np.float32(0.75), np.float32(0))
        elif k == 4 and D > 4:
            A[i, j, 3] = A[i, j, 4] = 0.125
    A.setflags(write=False)
    return A, kind


WTA_SIZES = [(5, 5), (5, 300), (300, 5)]     # W x H


def prove_wta(W, H, D=256):
    A, kind = wta_volume(W, H, D)
    raw = R.wta_raw(A)
    want = {0: 0, 1: D - 1, 2: D - 1, 3: 7, 4: 3}
    for k, v in want.items():
        assert (kind == k).any() and (raw[kind == k] == v).all(), (k, v)
    a = A[kind == 3][0]
    assert a[7] < a[8] and np.nextafter(a[7], np.float32(1)) == a[8]
    a = A[kind == 2][0]
    assert (np.diff(a) < 0).all()
    if min(W, H) == 5 and max(W, H) == 5:
        assert (R.wta(A, H, W) == 0).all()        # the window is the whole image: the majority's first minimum everywhere
    else:
        assert np.array_equal(R.wta(A, H, W), raw)     # bands five wide survive the median


# ---- LRcheck ----------------------------------------------------------------------------------------------------------------------------
def lr_maps(W):
    """d1 / d2 of 4 rows x W (W = 256, 257), D = 256, all pixels unstable (d1 = 9 looks at a d2 of 200) except the named ones."""
    d1 = np.full((4, W), 9, np.uint8)
    d2 = np.full((4, W), 200, np.uint8)
    named = {}
    d1[0, 5] = 5; d2[0, 0] = 5; named["j - dd == 0, stable"] = ((0, 5), 1)
    d1[1, 4] = 5; d2[0, W - 1] = 5; named["j - dd == -1: the previous row's last pixel agrees, must not be looked at"] = ((1, 4), 0)
    d1[1, 20] = 0; d2[1, 20] = 0; named["dd == 0 with d2 equal: not stable"] = ((1, 20), 0)
    d1[1, 40] = 12; d2[1, 28] = 13; named["d2 off by one (+)"] = ((1, 40), 0)
    d1[1, 60] = 12; d2[1, 48] = 11; named["d2 off by one (-)"] = ((1, 60), 0)
    d1[1, 80] = 12; d2[1, 68] = 12; named["inside, stable"] = ((1, 80), 1)
    d1[2, 255] = 255; d2[2, 0] = 255; named["dd = 255 at column 255, stable"] = ((2, 255), 1)
    d1[3, 254] = 255; d2[2, W - 1] = 255; named["dd = 255 at column 254: j - dd == -1"] = ((3, 254), 0)
    if W > 256:
        d1[3, 256] = 255; d2[3, 1] = 255; named["dd = 255 at column 256, stable"] = ((3, 256), 1)
    d1[0, 0] = 0; d2[0, 0] = 5
    for a in (d1, d2):
        a.setflags(write=False)
    return d1, d2, named


def prove_lr(W):
    d1, d2, named = lr_maps(W)
    vol, mask = R.lrcheck(d1, d2, 256)
    for why, ((i, j), m) in named.items():
        assert mask[i, j] == m, why
    assert int(mask.sum()) == sum(m for _, m in named.values())
    (i, j), _ = named["j - dd == 0, stable"]
    assert j - int(d1[i, j]) == 0
    (i, j), _ = named["j - dd == -1: the previous row's last pixel agrees, must not be looked at"]
    assert j - int(d1[i, j]) == -1 and d2.reshape(-1)[i * W + j - int(d1[i, j])] == d1[i, j]
    assert vol[2, 255].tolist() == [float(255 - k) for k in range(256)] and not vol[1, 20].any()


# ---- ctmf -------------------------------------------------------------------------------------------------------------------------------
CTMF_SHAPES = [(1, 1), (1, 9), (9, 1), (3, 3), (1, 1, 3), (3, 3, 3), (1, 9, 3)]     # H x W [x channels]: all smaller than an r = 2 window


def ctmf_image(shape):
    a = np.random.default_rng(sum(shape) * 7 + len(shape)).integers(0, 256, shape, dtype=np.uint8)
    a.setflags(write=False)
    return a


# ---- whole solves -------------------------------------------------------------------------------------------------------------------------
def solve_pair(W, H, shift=0):
    """init_pair's left image; with `shift` the right one is the left shifted by `shift` columns (a wider image cropped twice)"""
    if not shift:
        return init_pair(W, H)
    rng = np.random.default_rng(W + 1000 * H + shift)
    wide = rng.integers(0, 256, (H, W + shift, 3), dtype=np.uint8)
    wide = R.median_clamped(np.repeat(np.repeat(wide[::2, ::2], 2, 0), 2, 1)[:H, :W + shift], 1)     # blobs, not salt and pepper
    return np.ascontiguousarray(wide[:, :W]), np.ascontiguousarray(wide[:, shift:shift + W])


# (name, W, H, d, shift, scales, bfs the probe must report)
SOLVE_CASES = [
    ("5x5_d16", 5, 5, 16, 0, (1,), 1),          # the r = 2 median window is the whole image
    ("5x40_d3", 5, 40, 3, 0, (1,), 1),
    ("40x5_d48", 40, 5, 48, 0, (1,), 1),
    ("33x21_d0", 33, 21, 0, 0, (1,), 1),        # D = 1: every pixel unstable, the map all zero
    ("48x32_d254", 48, 32, 254, 0, (1,), 1),    # the gather tile is exactly 64 KB
    ("48x32_d255", 48, 32, 255, 0, (1,), 0),    # the fall-back a caller reaches without any variable
    ("shift40", 96, 24, 48, 40, (1, 3, 7), 1),  # d * scale wraps past 255
]


def gray_to_bgr(g):
    return np.ascontiguousarray(np.repeat(np.asarray(g, np.uint8)[:, :, None], 3, 2))


def batch_frames(B=3, W=48, H=32):
    """B gray pairs: init_pair's blue, green, red channels of one colour pair, so that the frames differ"""
    L, Rr = init_pair(W, H)
    return [(np.ascontiguousarray(L[:, :, b % 3] + 5 * b), np.ascontiguousarray(Rr[:, :, b % 3] + 5 * b)) for b in range(B)]


def trees_of(init_out):
    """the two aggregation trees of a pair from the product's host-side graph stages (svo_msa_tree; no GPU): left, right"""
    import svo_loader
    pkg = svo_loader.load()
    return tuple(pkg.msa_tree(init_out["m3" + s], init_out["r_gra" + s], init_out["c_gra" + s]) for s in "LR")


@functools.lru_cache(maxsize=None)
def solved(name):
    """the twin's solve of a whole-solve case on the product's trees (scale 1): every intermediate, computed once"""
    _, W, H, d, shift, _, _ = next(c for c in SOLVE_CASES if c[0] == name)
    L, Rr = solve_pair(W, H, shift)
    tL, tR = trees_of(R.init(L, Rr, 1))
    s = R.solve(L, Rr, d, 1, tL, tR)
    s["treeL"], s["treeR"] = tL, tR
    for a in s.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def batch_twin_maps(d, B=3):
    """what svo_msa_batch_dev must return for batch_frames(): the twin's solve of every B = G = R pair, as floats"""
    out = []
    for gl, gr in batch_frames(B):
        L, Rr = gray_to_bgr(gl), gray_to_bgr(gr)
        tL, tR = trees_of(R.init(L, Rr, 1))
        out.append(R.solve(L, Rr, d, 1, tL, tR)["out"].astype(np.float32))
    return tuple(out)


BATCH_PITCH, BATCH_FILL = 64, 0xEE


def prove_batch_padding(d, B=3, W=48, H=32):
    """Reading the padding would change the result.  Two ways to read it, both on the twin: rows taken W bytes apart where they lie
    BATCH_PITCH apart (the padding slides into every row but the first) gives another map for EVERY frame; the image taken at its
    full pitch (the 16 columns of BATCH_FILL as pixels) and cropped back to W columns gives another map for at least one.  (With
    d = 0 every map is zero whatever the images hold, so only d > 0 can carry this.)"""
    assert d > 0

    def solved_map(gl, gr):
        L, Rr = gray_to_bgr(gl), gray_to_bgr(gr)
        tL, tR = trees_of(R.init(L, Rr, 1))
        return R.solve(L, Rr, d, 1, tL, tR)["out"].astype(np.float32)

    wide_differs = 0
    for (gl, gr), want in zip(batch_frames(B, W, H), batch_twin_maps(d, B)):
        wide = [np.concatenate([g, np.full((H, BATCH_PITCH - W), BATCH_FILL, np.uint8)], 1) for g in (gl, gr)]
        sheared = [np.ascontiguousarray(g.reshape(-1)[:H * W].reshape(H, W)) for g in wide]
        assert solved_map(*sheared).tobytes() != want.tobytes()
        wide_differs += solved_map(*wide)[:, :W].tobytes() != want.tobytes()
    assert wide_differs >= 1
