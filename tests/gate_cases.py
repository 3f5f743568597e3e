"""Seeded inputs of the semantic gate's matching tests (tests/test_gate_cpu.py checks that each case has the property it is
named for, with the plain references of tests/gate_ref.py alone; tests/test_gate_gpu.py runs the device on them)."""
import functools

import numpy as np

import gate_ref
import util

W, H = 1241, 376
# the first box's padded left and top edges are negative
BOXES = np.array([[5, 200, 3, 150], [400, 800, 100, 300], [900, 1100, 50, 200]], np.int32)

BF_SHAPES = [(1, 1), (5, 63), (5, 64), (5, 65), (3, 1024), (501, 500), (4, 0)]
GATED_SHAPES = [(40, 7), (64, 64), (65, 65), (200, 500), (20, 512), (20, 513), (30, 1000)]


def _K():
    return np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1.0]])


def general_F():
    """A rank-2 F with F[8] = 1: yaw 0.03 and a general translation between two KITTI cameras."""
    a = 0.03
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    t = np.array([0.4, -0.1, -1.0])
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(_K())
    F = Ki.T @ tx @ R @ Ki
    return F / F[2, 2]


def line_F(y):
    """F whose line for every last-frame point is cur_y = y: the distance is |cur_y - y|, exact in any rounding."""
    return np.array([[0, 0, 0], [0, 0, 1.0], [0, 0, -float(y)]])


# ---- svo_bf_match ---------------------------------------------------------------------------------------------------------
def bf_shape_case(M, N):
    if N == 0:
        return util.random_descriptors(11, M), np.zeros((0, 32), np.uint8)
    return util.planted_descriptors(300 + M + N, M, N)


def bf_tie_case():
    """One train descriptor at j = 3, 64 + 3 and 700: the same lane on two trips, and another lane.  Queries at several
    distances of it, and queries whose tie does not include j = 3 (that copy is replaced for them by a farther one)."""
    rng = np.random.default_rng(21)
    t = util.random_descriptors(22, 1024)
    t[67] = t[3]; t[700] = t[3]
    q = np.stack([util.flip_bits(t[3], d, rng) for d in (0, 1, 7, 30, 31, 64)])
    t2 = t.copy(); t2[3] = util.flip_bits(t[67], 40, rng)
    return (q, t), (q, t2)


def bf_minimum_case(gmin):
    """Global minimum gmin (0: the threshold is 30, 16: it is 32) and rows at exactly the threshold and one above."""
    rng = np.random.default_rng(31 + gmin)
    t = util.random_descriptors(32 + gmin, 100)
    thr = max(2 * gmin, 30)
    q = np.stack([util.flip_bits(t[5], gmin, rng), util.flip_bits(t[9], thr, rng), util.flip_bits(t[11], thr + 1, rng),
                  util.random_descriptors(33 + gmin, 1)[0]])
    return q, t, thr


# ---- svo_match_greedy_gated -----------------------------------------------------------------------------------------------
def _on_line_q(F, txy, rng, off):
    """A last-frame point q with txy `off` pixels (in q's y) away from being on its line: [t,1]^T F [q,1] = 0 at off = 0."""
    l = F.T @ np.array([txy[0], txy[1], 1.0], np.float64)
    while True:
        x = rng.uniform(0, W)
        if abs(l[1]) > 1e-9:
            return np.array([x, -(l[0] * x + l[2]) / l[1] + off])


def _draw_gated(seed, M, N, max_dist, ratio, boxes, release):
    rng = np.random.default_rng(seed)
    F = general_F()
    t = util.random_descriptors(seed + 1, N)
    q = util.random_descriptors(seed + 2, M)
    t_xy = np.stack([rng.uniform(0, W, N), rng.uniform(0, H, N)], 1).astype(np.float32)
    q_xy = np.stack([rng.uniform(0, W, M), rng.uniform(0, H, M)], 1).astype(np.float32)
    assigned = (rng.random(N) < 0.1).astype(np.uint8)
    skip = (rng.random(M) < 0.2).astype(np.uint8)
    dists = [0, 5, 14, 15, 29, 30]
    pairs = []
    rel_cols = []
    if release:
        rel_cols = [int(j) for j in rng.permutation(N)[:release]]
        for j in rel_cols:                   # an unclaimed column whose point lies inside the middle box
            assigned[j] = 0
            t_xy[j] = (rng.uniform(410, 790), rng.uniform(110, 290))
    free_cols = [j for j in range(N) if j not in rel_cols]
    rel_rows = []
    for k, j in enumerate(rel_cols):         # row i is vetoed at column j, row i + 1 takes it
        i = 3 + 5 * k
        rel_rows += [i, i + 1]
        pairs.append((i, j))
        skip[i] = skip[i + 1] = 0
        q[i] = util.flip_bits(t[j], 2, rng); q[i + 1] = util.flip_bits(t[j], 3, rng)
        q_xy[i] = _on_line_q(F, t_xy[j], rng, 15.0).astype(np.float32)
        q_xy[i + 1] = _on_line_q(F, t_xy[j], rng, 0.0).astype(np.float32)
    for i in range(M):
        if i in rel_rows:
            continue
        j = int(free_cols[rng.integers(0, len(free_cols))])
        q[i] = util.flip_bits(t[j], dists[i % len(dists)], rng)
        off = 0.0 if rng.random() < 0.5 else float(rng.choice([-1, 1]) * rng.uniform(2, 20))
        q_xy[i] = _on_line_q(F, t_xy[j], rng, off).astype(np.float32)
    return dict(q=q, t=t, assigned=assigned, q_skip=skip, max_dist=max_dist, ratio=ratio, q_xy=q_xy, t_xy=t_xy,
                boxes=np.asarray(boxes, np.int32), F=F, release=pairs)


def reference(c):
    return gate_ref.greedy_gated_ref(c["q"], c["q_skip"], c["t"], c["assigned"], c["max_dist"], c["ratio"], c["q_xy"], c["t_xy"],
                                     c["boxes"], c["F"])


def well_conditioned(c, ref):
    """No in-box candidate within 1e-9 of the 0.1 px threshold, at least one veto and one in-box acceptance, and every
    claimed release of a vetoed column happens - by the reference alone."""
    bi, b, s, acc, asg, vet, info = ref
    if any(inb and abs(d - gate_ref.VETO_PX) < 1e-9 for _, _, inb, d in info):
        return False
    if vet.sum() == 0 or not any(inb and acc[i] for i, _, inb, _ in info):
        return False
    return all(vet[i] == 1 and acc[i + 1] == 1 and bi[i] == j and bi[i + 1] == j for i, j in c["release"])


@functools.lru_cache(maxsize=None)
def gated_case(M, N, max_dist=15, ratio=0.0, many_boxes=False):
    """The (M, N) case and its reference result.  Seeds are re-drawn until well_conditioned holds (no case is exempted at
    run time); release pairs are planted where the shape has room for them."""
    boxes = BOXES
    if many_boxes:          # 64 boxes, 63 of them far outside the image: the deciding ones come last
        far = np.array([[5000 + 10 * k, 5005 + 10 * k, 5000, 5005] for k in range(61)], np.int32)
        boxes = np.concatenate([far, BOXES])
    release = 1 if N < 64 else 2
    seed = 7000 + 13 * M + N + int(max_dist) + (500 if many_boxes else 0)
    for attempt in range(50):
        c = _draw_gated(seed + 104729 * attempt, M, N, max_dist, ratio, boxes, release)
        ref = reference(c)
        if well_conditioned(c, ref):
            return c, ref
    raise AssertionError("no well-conditioned gated case for %r" % ((M, N, max_dist, ratio),))


def _plant_rows(t, n_rows, seed):
    """Row i is a near copy (distance 3) of train column i."""
    rng = np.random.default_rng(seed)
    return np.stack([util.flip_bits(t[i], 3, rng) for i in range(n_rows)])


@functools.lru_cache(maxsize=None)
def threshold_case():
    """The line is y = 100: the distance is |cy - 100| exactly.  cy: the two float32 values on either side of 100.1, then
    100.0 and 99.875.  Expected veto: only where cy - 100 > 0.1 in exact arithmetic."""
    v = np.float32(100.1)                    # 100.09999847: below 100.1
    ys = np.array([np.nextafter(v, np.float32(0)), v, np.nextafter(v, np.float32(200)),
                   np.nextafter(np.nextafter(v, np.float32(200)), np.float32(200)), 100.0, 99.875], np.float32)
    expect = np.array([0, 0, 1, 1, 0, 1], np.uint8)
    n = len(ys)
    t = util.random_descriptors(41, n)
    c = dict(q=_plant_rows(t, n, 42), t=t, assigned=np.zeros(n, np.uint8), q_skip=np.zeros(n, np.uint8), max_dist=15, ratio=0.0,
             q_xy=np.full((n, 2), 50.0, np.float32), t_xy=np.stack([np.full(n, 600.0, np.float32), ys], 1),
             boxes=BOXES[1:2], F=line_F(100), release=[])
    return c, reference(c), expect


@functools.lru_cache(maxsize=None)
def box_edge_case():
    """Train points on, and one float32 step inside, each padded edge of two boxes (one with negative padded edges).  The
    line is y = 120 and every edge point is far from it, so a row is vetoed exactly where its point is inside; two more
    points sit on the line inside a box (in-box acceptances)."""
    f = np.float32
    pts, inside = [], []
    for left, right, top, bottom in BOXES[:2]:
        xm, ym = f((left + right) / 2), f((top + bottom) / 2 + 7)
        L, R, T, B = f(left - 10), f(right + 10), f(top - 10), f(bottom + 10)
        pts += [(L, ym), (np.nextafter(L, f(1e9)), ym), (np.nextafter(R, f(-1e9)), ym), (R, ym),
                (xm, T), (xm, np.nextafter(T, f(1e9))), (xm, np.nextafter(B, f(-1e9))), (xm, B)]
        inside += [0, 1, 1, 0, 0, 1, 1, 0]
    pts += [(f(100), f(120)), (f(600), f(120))]
    n = len(pts)
    expect = np.array(inside + [0, 0], np.uint8)
    t = util.random_descriptors(51, n)
    c = dict(q=_plant_rows(t, n, 52), t=t, assigned=np.zeros(n, np.uint8), q_skip=np.zeros(n, np.uint8), max_dist=15, ratio=0.0,
             q_xy=np.full((n, 2), 50.0, np.float32), t_xy=np.array(pts, np.float32), boxes=BOXES[:2], F=line_F(120), release=[])
    return c, reference(c), expect


@functools.lru_cache(maxsize=None)
def zero_F_case():
    """F = 0 and every train point inside a box: every distance is NaN, nothing is vetoed, the result is the ungated one."""
    c, _ = gated_case(64, 64)
    c = dict(c)
    rng = np.random.default_rng(61)
    c["t_xy"] = np.stack([rng.uniform(410, 790, 64), rng.uniform(110, 290, 64)], 1).astype(np.float32)
    c["F"] = np.zeros((3, 3))
    return c, reference(c)
