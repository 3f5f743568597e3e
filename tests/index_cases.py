"""Seeded, hand-made descriptor frames for the tracker's matching passes (tests/test_index_cpu.py, tests/test_index_gpu.py).

A case is a list of at most 8 frames of at most 500 keypoints.  Descriptors are built by flipping chosen bits of seeded bases, so
every distance that matters is known by construction (two flips of one base are as far apart as their flipped bit sets differ);
bases are random, ~128 bits apart, and never interact.  The columns nobody cares about hold `background` descriptors that
come back unchanged in every frame: pass 1 matches them at distance 0 and they keep PnP and the LM well-posed.

Positions and depths come from ONE rigid seeded scene seen from a slowly moving camera.  The index side never reads positions,
so each keypoint is given the scene point of the map point the plain restatement (index_ref) matches it to - every match is then
a geometric inlier - and a fresh scene point otherwise; observations carry NOISE_PX of pixel noise.  Depths lie in [2, 80] m;
"no depth" is -1.

build(name, cam) -> dict(frames=[(kp, desc, depth, boxes)], expect=[(frame, column, source or None, pass)], ref=[index_ref's
results per frame], fiat={frame: (veto, nocreate)} for the case with boxes).  `source` = (frame, column) of the keypoint whose
map point the column must be matched to."""
import functools

import numpy as np

import index_ref

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                     ("class_id", "<i4")])
MAX_KP = 500
NOISE_PX = 0.4      # keypoints are observed with this much Gaussian noise, as real corners are: on exact data the LM ends at the
                    # rounding floor, where its decisions (and so the iteration count the records carry) have no margin


def v(d, *ranges):
    """d with the bits lo .. lo + n - 1 flipped, for every (lo, n)."""
    d = d.copy()
    for lo, n in ranges:
        assert 0 <= lo and lo + n <= 256
        for p in range(lo, lo + n):
            d[p >> 3] ^= np.uint8(1 << (p & 7))
    return d


class Frames:
    def __init__(self, seed, nframes, size, motion=(0.3, 0.0, 0.1), yaw=0.002):
        self.rng = np.random.default_rng(seed)
        self.seed, self.motion, self.yaw = seed, motion, yaw
        self.bg = self.rng.integers(0, 256, (512, 32), dtype=np.uint8)
        self.slots = [dict() for _ in range(nframes)]
        self.size = [size] * nframes if np.isscalar(size) else list(size)
        self.expect, self.pinned, self.fiat, self.boxes = [], {}, {}, {}
        self.bg_depth = {}
        self.exact_frames = ()           # frames whose keypoints carry no pixel noise

    def base(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def put(self, f, desc, col=None, depth=True):
        s = self.slots[f]
        if col is None:
            col = 0
            while col in s:
                col += 1
        assert col not in s and 0 <= col < self.size[f], (f, col)
        s[col] = (desc, depth)
        return (f, col)

    def want(self, at, src, which=0):
        self.expect.append((at[0], at[1], src, which))

    def arrays(self):
        out = []
        for f, s in enumerate(self.slots):
            n = self.size[f]
            assert n <= MAX_KP
            desc = self.bg[:n].copy()
            has = np.full(n, self.bg_depth.get(f, True))
            for col, (d, z) in s.items():
                desc[col] = d; has[col] = z
            out.append((desc, has))
        return out


def realise(fr, cam):
    """Run the plain restatement over the descriptors, give every keypoint its scene point, project."""
    arr = fr.arrays()
    trk = index_ref.Tracker()
    rng = np.random.default_rng(fr.seed + 1000)
    scene, of_gid, ref, where = [], {}, [], []
    for f, (desc, has) in enumerate(arr):
        veto, nocreate = fr.fiat.get(f, (None, None))
        r = trk.step(desc, np.where(has, 1.0, -1.0), veto=veto, nocreate=nocreate)
        ids = np.zeros(len(desc), np.int64)
        for j in range(len(desc)):
            g = int(r["match_gid"][j])
            if g >= 0:
                ids[j] = of_gid[g]
            else:
                ids[j] = len(scene)
                if (f, j) in fr.pinned:
                    scene.append(fr.pinned[(f, j)])
                else:
                    while True:
                        p = (rng.uniform(30, 1210), rng.uniform(20, 350), rng.uniform(6, 60))
                        if not any(a <= p[0] <= b and c <= p[1] <= d for a, b, c, d in fr.boxes.get("keep_out", [])):
                            break
                    scene.append(p)
            if r["new_gid"][j] >= 0:
                of_gid[int(r["new_gid"][j])] = ids[j]
        ref.append(r); where.append(ids)
    S = np.array(scene, np.float64).reshape(-1, 3)
    Xw = np.stack([(S[:, 0] - cam["cx"]) * S[:, 2] / cam["fx"], (S[:, 1] - cam["cy"]) * S[:, 2] / cam["fy"], S[:, 2]], 1)
    frames = []
    noise = np.random.default_rng(fr.seed + 2000)
    for f, (desc, has) in enumerate(arr):
        th = fr.yaw * f
        R = np.array([[np.cos(th), 0, -np.sin(th)], [0, 1, 0], [np.sin(th), 0, np.cos(th)]])
        Xc = (Xw[where[f]] - f * np.array(fr.motion)) @ R.T
        kp = np.zeros(len(desc), KP_DTYPE)
        kp["x"] = cam["fx"] * Xc[:, 0] / Xc[:, 2] + cam["cx"]
        kp["y"] = cam["fy"] * Xc[:, 1] / Xc[:, 2] + cam["cy"]
        e = noise.normal(0.0, NOISE_PX, (len(desc), 2))
        if f not in fr.exact_frames:
            kp["x"] += e[:, 0]; kp["y"] += e[:, 1]
        kp["size"] = 31; kp["angle"] = -1; kp["response"] = 1; kp["class_id"] = -1
        depth = np.where(has, Xc[:, 2], -1.0).astype(np.float32)
        assert ((depth == -1) | ((depth >= 2) & (depth <= 80))).all()
        frames.append((kp, desc, depth, fr.boxes.get(f, np.zeros((0, 4), np.int32))))
    return dict(frames=frames, expect=fr.expect, ref=ref, fiat=fr.fiat)


# ---- a. thresholds ------------------------------------------------------------------------------------------------------
def _thresholds(fr):
    """frame 0: pass-2 rows, frame 1: pass-1 rows, frame 2: the columns."""
    def p1():
        x = fr.base(); src = fr.put(1, x)
        return x, src

    def p2():
        y = fr.base(); src = fr.put(0, y)
        return y, src
    x, s = p1(); fr.want(fr.put(2, v(x, (0, 14))), s, 1)                    # pass 1: 14 matches
    x, s = p1(); fr.want(fr.put(2, v(x, (0, 15))), s, 2)                    # 15 does not (pass 2 then takes it: 15 < 30)
    y, s = p2(); fr.want(fr.put(2, v(y, (0, 29))), s, 2)                     # pass 2: 29 matches
    y, s = p2(); fr.want(fr.put(2, v(y, (0, 30))), None)                     # 30 does not
    for b in (10, 14, 20):                                                   # runner-up 2 x best / 2 x best + 1 (10, 14: the
        y, s = p2()                                                          # runner-up is an entry of the list; 20: a stored blocker)
        fr.want(fr.put(2, v(y, (0, 2 * b))), None); fr.want(fr.put(2, v(y, (100, b))), None)
        y, s = p2()
        fr.want(fr.put(2, v(y, (0, 2 * b + 1))), None); fr.want(fr.put(2, v(y, (100, b))), s, 2)
    y, s = p2(); fr.want(fr.put(2, v(y, (0, 5))), None); fr.want(fr.put(2, y.copy()), s, 2)      # best = 0: 5 / 0 = inf
    y, s = p2(); fr.want(fr.put(2, v(y, (0, 10))), s, 2); fr.want(fr.put(2, v(y, (100, 12))), None)   # smaller-than-2x AFTER the best
    y, s = p2(); fr.want(fr.put(2, v(y, (0, 29))), s, 2)                     # the best is the first unclaimed column: second = 256
    x, s = p1(); fr.want(fr.put(2, x.copy()), s, 1)                         # pass 1: 0


def thresholds():
    fr = Frames(11, 3, 80)
    _thresholds(fr)
    return fr


# ---- b. ties ----------------------------------------------------------------------------------------------------------------
TIE_GROUPS = ((60, 61), (3, 67), (16, 24), (100, 199), (130, 131, 194))     # j / j+1, j / j+64, j / j+8, the last column, three


def ties(dense):
    """Each group: as many identical rows as tied columns, + one row more - for pass 2 (rows of frame 0, columns of frame 2) and
    for pass 1 (frames 3 and 4), all at distance 10.  dense: every row also has nine columns at 29 (behind most of its ties)."""
    fr = Frames(12 + dense, 5, 200)
    tail = iter(range(140, 190))
    for which, f_rows, f_cols in ((2, 0, 2), (1, 3, 4)):
        bases = [fr.base() for g in TIE_GROUPS]
        for g, x in zip(TIE_GROUPS, bases):
            rows = [fr.put(f_rows, x.copy()) for _ in range(len(g) + 1)]
            for k, col in enumerate(g):
                fr.want(fr.put(f_cols, v(x, (20 * k, 10)), col), rows[k], which)
        if dense:
            for x in bases:
                for k in range(9):
                    fr.put(f_cols, v(x, (128 + 8 * k, 29)), next(tail) if which == 2 else None)
    return fr


# ---- c. chains ------------------------------------------------------------------------------------------------------------
def chain(R, which, size, alternate=False):
    """R identical rows against R identical columns: row k ends on column k.  alternate: odd rows are 10 bits off and have a
    blocker in column 0 that nobody can claim - rejected for good; even row 2 i takes column 1 + i."""
    fr = Frames(13 + R + which, 3, size)
    x = fr.base()
    f_rows = 0 if which == 2 else 1
    c = v(x, (0, 10))
    if alternate:
        assert which == 2
        fr.put(2, v(x, (10, 10), (100, 35)), 0)
        rows = [fr.put(f_rows, x.copy() if k % 2 == 0 else v(x, (10, 10))) for k in range(R)]
        for i in range(R):
            fr.want(fr.put(2, c.copy(), 1 + i), rows[2 * i] if 2 * i < R else None, 2 if 2 * i < R else 0)
    else:
        rows = [fr.put(f_rows, x.copy()) for k in range(R)]
        for k in range(R):
            fr.want(fr.put(2, c.copy()), rows[k], which)
    return fr


def chains_small():
    fr = Frames(14, 3, 200)
    for R, which in ((2, 1), (2, 2), (65, 1), (65, 2)):
        x = fr.base()
        rows = [fr.put(0 if which == 2 else 1, x.copy()) for k in range(R)]
        for k in range(R):
            fr.want(fr.put(2, v(x, (0, 10))), rows[k], which)
    return fr


# ---- d. displacement and flipping blockers (pass 2) -----------------------------------------------------------------------------
def _blockers(fr, f_rows=0, f_cols=2):
    put, want = fr.put, fr.want
    for e_bits in (20, 32):                              # the best column goes to an earlier row: fall to the second entry
        a = fr.base(); b = v(a, (0, 6))
        ra, rb = put(f_rows, a), put(f_rows, b)
        want(put(f_cols, v(a, (200, 3))), ra, 2)
        want(put(f_cols, v(b, (100, e_bits))), rb if e_bits < 30 else None, 2 if e_bits < 30 else 0)
    for kd, cd, nblockers, stays in ((20, 12, 1, False), (35, 20, 1, False), (35, 20, 4, False),
                                     (20, 12, 1, True), (35, 20, 1, True), (35, 20, 4, True)):
        # row b: best column c at cd, blockers k before it at kd; earlier rows a claim the blockers away (or one stays)
        b = fr.base()
        ks = [v(b, (30 * q, kd)) for q in range(nblockers)]
        ras = [put(f_rows, v(k, (250, 2))) for q, k in enumerate(ks) if not (stays and q == nblockers - 1)]
        rb = put(f_rows, b)
        kcols = [put(f_cols, k) for k in ks]
        for q, ra in enumerate(ras):
            want(kcols[q], ra, 2)
        if stays:
            want(kcols[-1], None)
        ccol = put(f_cols, v(b, (200, cd)))
        if stays:                                        # a LATER row takes c in the end
            rc = put(f_rows, v(b, (200, cd), (240, 3)))
            want(ccol, rc, 2)
        else:
            want(ccol, rb, 2)
    # ranks: F takes f; E (then on its second entry e2) is blocked by x, which the LATER row L claims in the first round -
    # E must not see that claim
    e = fr.base()
    f_ = v(e, (0, 5)); e2 = v(e, (100, 20)); x = v(e, (150, 35))
    rF, rE, rL = put(f_rows, v(f_, (250, 2))), put(f_rows, e), put(f_rows, v(x, (240, 3)))
    want(put(f_cols, x), rL, 2); want(put(f_cols, e2), None); want(put(f_cols, f_), rF, 2)


def blockers():
    fr = Frames(15, 3, 90)
    _blockers(fr)
    return fr


# ---- e. dense rows ----------------------------------------------------------------------------------------------------------
def dense_lcap():
    """Rows with 1, 2, 3, 8, 9 and 12 columns below 30 (lcap and lcap + 1 for track_lcap 1, 2 and 8): the first at 10 is
    taken; and the same rows with the FIRST column at 25 and the best at 12 behind it - rejected (25 <= 24 is false: accepted)
    at 25, rejected at 24."""
    fr = Frames(16, 3, 160)
    for n in (1, 2, 3, 8, 9, 12):
        for first, best in ((10, None), (25, 12), (24, 12)):
            y = fr.base(); s = fr.put(0, y)
            cols = [fr.put(2, v(y, (0, first)))]
            for k in range(1, n):
                cols.append(fr.put(2, v(y, (40 + 16 * k, 12 if (best and k == 1) else 26))))
            for k, c in enumerate(cols):
                if best is None or n == 1:
                    hit = k == 0
                else:
                    hit = k == 1 and first == 25
                fr.want(c, s if hit else None, 2 if hit else 0)
    return fr


def dense_join():
    """A row that goes dense in mid-pass (its three stored blockers are claimed, a fourth exists) while 40 dense rows are
    already on the list: it lands on list position 40, beyond the LDS cache."""
    fr = Frames(17, 3, 120)
    x = fr.base()
    rows = [fr.put(0, x.copy()) for k in range(40)]
    _blockers(fr)
    for k in range(40):
        fr.want(fr.put(2, v(x, (0, 10))), rows[k], 2)
    return fr


def many_rows(n_active, holes, chain=0):
    """Three frames of unmatched keypoints, then a frame whose keypoint c lies 16 .. 29 bits from the three points of
    cluster c (one per frame, 44 bits from each other); static camera (frames 1 and 2 match nothing).  holes: clusters
    c % 5 == 4 have no depth in frames 0 and 1, so the row of frame 2 - among the last in pass 2 - wins them.  chain: the
    last `chain` clusters exist in frame 2 only, with ONE descriptor, against identical columns 20 bits off: a chain of
    dense rows, all of them past row 1024 and past the LDS cache."""
    base_n = 500
    lost = len([c for c in range(base_n) if c % 5 == 4]) if holes else chain
    n2 = n_active - 2 * (base_n - lost)
    assert 0 < n2 <= base_n and not (holes and chain)
    fr = Frames(18 + n_active, 4, [base_n, base_n, n2, base_n], motion=(0.0, 0.0, 0.0))
    K = [fr.base() for c in range(base_n)]
    z = fr.base()
    for f, n in enumerate((base_n, base_n, n2)):
        for c in range(n):
            if c >= base_n - chain:
                src = fr.put(f, z.copy(), c, depth=f == 2)
                if f == 2:
                    fr.want((3, c), src, 2)
            else:
                fr.put(f, v(K[c], (22 * f, 16 + (c + f) % 7), (22 * f + 66, (c // 7) % 8)), c, depth=not (holes and f < 2 and c % 5 == 4))
    for c in range(base_n):
        fr.put(3, K[c] if c < base_n - chain else v(z, (0, 20)), c)
    return fr


# ---- f. counts --------------------------------------------------------------------------------------------------------------
def counts(ns, depthless=()):
    """The first n of one persistent set of descriptors per frame, each appearance 3 bits off."""
    fr = Frames(19 + len(ns), len(ns), list(ns))
    rng = np.random.default_rng(190)
    for f, n in enumerate(ns):
        if f in depthless:
            fr.bg_depth[f] = False
        for c in range(n):
            d = fr.bg[c].copy()
            for p in rng.choice(256, 3, replace=False):
                d[p >> 3] ^= np.uint8(1 << (p & 7))
            fr.put(f, d, c, depth=f not in depthless)
    return fr


# ---- g. cull and compaction ---------------------------------------------------------------------------------------------------
def cull(extra):
    """Created at frame 1, back at frames 4 (f + 3) and 5 (f + 4): pass 2 finds them; at frame 6 (f + 5): culled, a new
    point.  A point seen in every frame is culled after frame 4 but stays referenced: pass 1 keeps matching it, and when it
    comes back 20 bits off (pass 2's business) at frame 6 nothing finds it, while a point created at frame 4 is found.
    extra: single keypoints that shift the pool size by one."""
    fr = Frames(20, 8, [60 + extra] + [60] * 7)
    for k in range(extra):
        fr.put(0, fr.base(), 59 + 1 + k)
    for back, found in ((4, True), (5, True), (6, False)):
        for k in range(3):
            u = fr.base(); s = fr.put(1, u)
            fr.want(fr.put(back, v(u, (0, 16 + k))), s if found else None, 2 if found else 0)
    old = fr.base(); s_old = fr.put(0, old)
    young = fr.base()
    for f in range(1, 6):
        fr.want(fr.put(f, old.copy()), s_old, 1)
    s_young = fr.put(4, young); fr.want(fr.put(5, young.copy()), s_young, 1)
    fr.want(fr.put(6, v(old, (0, 20))), None)
    fr.want(fr.put(6, v(young, (0, 20))), s_young, 2)
    return fr


# ---- h. veto inside a chain ---------------------------------------------------------------------------------------------------
def veto_chain():
    """Four identical last-frame points against four identical columns inside a box: the second row's best column belongs
    (geometrically) to the third row's point, far off the second's epipolar line - vetoed, it claims nothing, the third row
    takes that column.  The vetoed point is bad: pass 2 skips it (it would take the fourth column otherwise); it stays in the
    pool while it is local and is culled with its generation.
    The reference solves F with (current, last) points and then measures the current point against the line F * last
    (src/pnpmatch.cc:110-113, :302-337) - F used the other way round.  That is exact only where F is skew-symmetric, so this
    camera translates without turning: true matches then lie ~1e-3 px from "their" line, the planted one 12 px."""
    fr = Frames(21, 8, 100, yaw=0.0)
    fr.exact_frames = (1, 2)             # the two frames F is solved from: the veto's 0.1 px is far below the noise elsewhere
    x = fr.base()
    u0 = 300.0
    rows = [fr.put(1, x.copy(), k) for k in range(4)]
    for k in range(4):
        fr.pinned[(1, k)] = (u0, 100.0 + 12.0 * k, 20.0)
    cols = [fr.put(2, v(x, (0, 5)), k) for k in range(4)]
    fr.pinned[(2, 3)] = (u0, 100.0 + 12.0 * 4, 20.0)
    fr.want(cols[0], rows[0], 1); fr.want(cols[1], rows[2], 1); fr.want(cols[2], rows[3], 1); fr.want(cols[3], None)
    veto = np.zeros((100, 100), bool); veto[1, 1] = True
    nocreate = np.zeros(100, bool); nocreate[:4] = True     # the four columns lie in the box padded by 5 px
    fr.fiat[2] = (veto, nocreate)
    # the scene moves ~ -9 px in x per frame at 20 m: the box holds the four columns of frame 2 with room to spare
    fr.boxes[2] = np.array([[int(u0) - 60, int(u0) + 30, 80, 170]], np.int32)
    fr.boxes["keep_out"] = [(u0 - 150, u0 + 250, 30, 230)]
    for f in range(3, 8):                                   # the three matched points live on
        for k in (0, 2, 3):
            fr.want(fr.put(f, x.copy(), k), rows[k], 1)
    return fr


CASES = {
    "thresholds": thresholds,
    "ties_packed": lambda: ties(0),
    "ties_dense": lambda: ties(1),
    "chains_small": chains_small,
    "chain_p1_300": lambda: chain(300, 1, 340),
    "chain_p2_300": lambda: chain(300, 2, 340),
    "chain_alternating": lambda: chain(61, 2, 100, alternate=True),
    "blockers": blockers,
    "dense_lcap": dense_lcap,
    "dense_15": lambda: chain(15, 2, 60),
    "dense_16": lambda: chain(16, 2, 60),
    "dense_17": lambda: chain(17, 2, 60),
    "dense_40": lambda: chain(40, 2, 90),
    "dense_41": lambda: chain(41, 2, 90),
    "dense_60": lambda: chain(60, 2, 100),
    "dense_join": dense_join,
    "rows_1023": lambda: many_rows(1023, True),
    "rows_1024": lambda: many_rows(1024, True),
    "rows_1025": lambda: many_rows(1025, True),
    "rows_1300": lambda: many_rows(1300, True),
    "rows_1500": lambda: many_rows(1500, False),
    "rows_1440": lambda: many_rows(1440, False, chain=30),
    "counts": lambda: counts((0, 64, 500, 0, 63, 65, 1, 500)),
    "counts_no_depth": lambda: counts((100, 120, 90, 120), depthless=(1,)),
    "cull_0": lambda: cull(0),
    "cull_1": lambda: cull(1),
    "cull_2": lambda: cull(2),
    "veto_chain": veto_chain,
}
NAMES = list(CASES)
SMALL_FIRST = sorted(NAMES, key=lambda n: (n.startswith("rows_"), "300" in n))


@functools.lru_cache(maxsize=None)
def _build(name, cam_items):
    return realise(CASES[name](), dict(cam_items))


def build(name, cam):
    return _build(name, tuple(sorted(cam.items())))


# ---- the oracle's side, computed once per case ------------------------------------------------------------------------------
W, H = 1241, 376
_ORACLE = {}


def oracle_tail(orc, cam, name):
    """orc_track_tail over the case's frames: per frame (record, pool rows, match_gid, new_gid, F, vetoes)."""
    if name not in _ORACLE:
        trk = orc.Tracker(W, H, cam)
        out = []
        for kp, desc, depth, boxes in build(name, cam)["frames"]:
            res, cur, pnp, Tp = trk.track_tail(kp, desc, depth, boxes=boxes)
            out.append((res.copy(), cur.copy(), trk.match_gid.copy(), trk.new_gid.copy(), trk.F.copy(), trk.vetoes))
        trk.close()
        _ORACLE[name] = out
    return _ORACLE[name]


def in_boxes(x, y, boxes, pad):
    """src/pnpmatch.cc:108: strictly inside the padded box {left, right, top, bottom}."""
    return any(x > b[0] - pad and x < b[1] + pad and y > b[2] - pad and y < b[3] + pad for b in boxes)


def oracle_veto(orc, F, boxes, last_kp, kp):
    """(veto[i, j], distance[i, j]) of last-frame keypoint i against column j, by the oracle's F and distance; columns outside
    the boxes padded by 10 px are never vetoed (distance NaN there)."""
    veto = np.zeros((len(last_kp), len(kp)), bool)
    dist = np.full((len(last_kp), len(kp)), np.nan)
    for j in range(len(kp)):
        if in_boxes(kp["x"][j], kp["y"][j], boxes, 10):
            for i in range(len(last_kp)):
                dist[i, j] = orc.epipolar_distance(F, (last_kp["x"][i], last_kp["y"][i]), (kp["x"][j], kp["y"][j]))
                veto[i, j] = dist[i, j] > 0.1
    nocreate = np.array([in_boxes(kp["x"][j], kp["y"][j], boxes, 5) for j in range(len(kp))], bool)
    return veto, dist, nocreate
