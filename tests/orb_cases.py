"""Hand-made images for the ORB extraction, each with the property it was made for.

A case is a named builder that returns (image, prove): `prove(r)` takes the twin's result for that image (tests/orb_ref.py
`extract`, plus r["img"]) and asserts, from the twin's intermediate results, that the image still reaches the edge it was made
for - tests/test_orb_cpu.py runs every one, so a case that drifts off its edge fails there and not silently on the GPU.

Building blocks: a DOT is one pixel that differs from a flat background by d; all 16 ring pixels are background, so its FAST
score is d - 1 and scores can be dialled.  Dots on an 8-pixel grid do not see each other in FAST (radius 3) or in the Harris
measure (9 x 9 pixels), so identical dots tie in both.

Contexts (W, H, max_kp): 192 x 128 (tile seams of k_fast at x = 147 | 148 and y = 60 | 61) for FAST, orientation and descriptor;
128..131 x 96 for the right image border at every w mod 4; 352 x 330 at max_kp 8 (quota 2, target 4), 9, 500 and 512 for the
selection."""
import functools

import numpy as np

import orb_ref
import util

CASES = {}
BG = 100
SW, SH = 352, 330          # the selection cases' image


def case(W, H, max_kp=500, fast=False):
    def deco(fn):
        CASES[fn.__name__] = dict(build=fn, W=W, H=H, max_kp=max_kp, fast=fast, doc=fn.__doc__)
        return fn
    return deco


def flat(W, H, v=BG):
    return np.full((H, W), v, np.uint8)


def l0(r):
    """Level-0 corners of a twin result as {(x, y): score}."""
    return {(int(x), int(y)): int(s) for x, y, s in r["corners"][0]}


def l0_kps(r):
    k = r["kp"][r["kp"]["octave"] == 0]
    return [(int(x), int(y)) for x, y in zip(k["x"], k["y"])]


def expect_l0(r, present, absent=()):
    got = l0(r)
    for (x, y), s in present.items():
        assert got.get((x, y)) == s, ("level-0 corner", (x, y), "score", s, "twin has", got.get((x, y)))
    for p in absent:
        assert p not in got, ("not a level-0 corner", p, got[p])


# ---- FAST: contrast ladder -------------------------------------------------------------------------------------------------------
def _ladder(bg):
    img = flat(192, 128, bg)
    present, absent = {}, []
    for i, d in enumerate((20, 21, 22, 23, 24)):
        for y, sign in ((44, 1), (76, -1)):
            x = 44 + 24 * i
            img[y, x] = bg + sign * d
            if d >= 21:
                present[(x, y)] = d - 1
            else:
                absent.append((x, y))

    def prove(r):
        expect_l0(r, present, absent)
        assert len(l0(r)) == 8
        sc = orb_ref.fast_scores(r["img"])
        assert (sc > 0).sum() == 8                       # nothing else scores: the corners are isolated
    return img, prove


for _bg in (100, 101, 102, 103):
    def _mk(bg=_bg):
        def fn():
            return _ladder(bg)
        fn.__name__ = "ladder_bg%d" % bg
        fn.__doc__ = ("dots of contrast 20..24, bright and dark, on %d: 20 is no corner, 21 scores 20; bright centres "
                      "%d (mod 4 = %d), dark centres %d (mod 4 = %d) at contrast 21" % (bg, bg + 21, (bg + 21) % 4, bg - 21, (bg - 21) % 4))
        return fn
    case(192, 128, fast=True)(_mk())


def _extreme(bg, vals):
    def fn():
        img = flat(192, 128, bg)
        present, absent = {}, []
        for i, v in enumerate(vals):
            p = (50 + 30 * i, 50 + 10 * i)
            img[p[1], p[0]] = v
            if abs(v - bg) >= 21:
                present[p] = abs(v - bg) - 1
            else:
                absent.append(p)

        def prove(r):
            expect_l0(r, present, absent)
            assert len(l0(r)) == len(present)
        return img, prove
    return fn


for _n, _bg, _vals in (("extreme_0", 0, (20, 21, 255)), ("extreme_255", 255, (235, 234, 0)), ("extreme_234", 234, (254, 255)),
                       ("extreme_21", 21, (1, 0))):
    _f = _extreme(_bg, _vals)
    _f.__name__ = _n
    _f.__doc__ = "grey levels at the ends of the range: background %d, dots %s (contrast 20 is no corner, 21 and 255 are)" % (_bg, _vals)
    case(192, 128, fast=True)(_f)


# ---- FAST: arc length ------------------------------------------------------------------------------------------------------------
def _draw_arc(img, cx, cy, start, length, v):
    for k in range(length):
        i = (start + k) % 16
        img[cy + orb_ref.RING_Y[i], cx + orb_ref.RING_X[i]] = v


def _arc_grid():
    return [(40 + 12 * i, 40 + 12 * j) for j in range(4) for i in range(10)]     # crosses the seams x = 148, y = 61


def _arc9(v):
    def fn():
        img = flat(192, 128)
        cs = _arc_grid()[:16]
        for s, (cx, cy) in enumerate(cs):
            _draw_arc(img, cx, cy, s, 9, v)

        def prove(r):
            sc = orb_ref.fast_scores(r["img"])
            for cx, cy in cs:
                assert sc[cy, cx] == abs(v - BG) - 1, (cx, cy, sc[cy, cx])
            expect_l0(r, {c: abs(v - BG) - 1 for c in cs})         # ... and each survives NMS, so the device must find it
        return img, prove
    return fn


for _n, _v in (("arc9_bright", 150), ("arc9_dark", 50)):
    _f = _arc9(_v)
    _f.__name__ = _n
    _f.__doc__ = ("an arc of exactly 9 ring pixels of %d around a centre of 100, at each of its 16 start positions: score 49 "
                  "every time (the compass pre-test must pass all of them)" % _v)
    case(192, 128, fast=True)(_f)


@case(192, 128, fast=True)
def arc_lengths():
    """arcs of 8, 9, 10 and 16 ring pixels, both polarities: 8 is no corner, the others score 49; 8 + gap + 6 + gap and
    7 + gap + 7 + gap (two arcs of 8 do not fit a ring of 16 with gaps) are no corners although 14 ring pixels differ"""
    img = flat(192, 128)
    cs = _arc_grid()
    want = {}
    k = 0
    for v in (150, 50):
        for start in (0, 5, 11):
            for length in (8, 9, 10, 16):
                cx, cy = cs[k]; k += 1
                _draw_arc(img, cx, cy, start, length, v)
                want[(cx, cy)] = 49 if length >= 9 else 0
        for a, b in ((8, 6), (7, 7)):
            cx, cy = cs[k]; k += 1
            _draw_arc(img, cx, cy, 2, a, v)
            _draw_arc(img, cx, cy, 2 + a + 1, b, v)
            want[(cx, cy)] = 0

    def prove(r):
        sc = orb_ref.fast_scores(r["img"])
        for (cx, cy), s in want.items():
            assert sc[cy, cx] == s, (cx, cy, s, sc[cy, cx])
        expect_l0(r, {c: s for c, s in want.items() if s}, [c for c, s in want.items() if not s])
    return img, prove


# ---- FAST: NMS ties, tile seams --------------------------------------------------------------------------------------------------
@case(192, 128, fast=True)
def nms_pairs():
    """two adjacent dots, horizontally, vertically and on both diagonals: equal scores suppress each other, of unequal ones the
    higher stays; the same pairs straddle k_fast's tile seams x = 147 | 148 and y = 60 | 61"""
    img = flat(192, 128)
    present, absent = {}, []
    steps = ((1, 0), (0, 1), (1, 1), (1, -1))
    spots = [(40 + 14 * i, 40) for i in range(4)] + [(40 + 14 * i, 80) for i in range(4)]       # inside a tile
    spots += [(147, 40), (147, 80), (147, 50), (147, 90)]                                       # across x = 147 | 148
    spots += [(50, 60), (64, 60), (78, 60), (92, 61)]                                           # across y = 60 | 61
    spots += [(147, 60), (147, 61)]                                                             # across both (diagonals)
    steps_of = steps + steps + ((1, 0), (1, 0), (1, 1), (1, -1)) + ((0, 1), (0, 1), (1, 1), (1, -1)) + ((1, 1), (1, -1))
    for k, ((x, y), (dx, dy)) in enumerate(zip(spots, steps_of)):
        equal = k < 4 or k in (8, 10, 12, 14, 16, 17)
        img[y, x] = 150
        img[y + dy, x + dx] = 150 if equal else 140
        if equal:
            absent += [(x, y), (x + dx, y + dy)]
        else:
            present[(x, y)] = 49
            absent.append((x + dx, y + dy))

    def prove(r):
        sc = orb_ref.fast_scores(r["img"])
        for p in absent:
            assert sc[p[1], p[0]] in (39, 49)            # each IS a FAST corner; only the NMS removes it
        expect_l0(r, present, absent)
        assert len(present) >= 8
    return img, prove


# ---- FAST: the 31-pixel border, the right image edge -----------------------------------------------------------------------------
def _border(W):
    def fn():
        H = 96
        img = flat(W, H)
        present, absent = {}, []
        for x, y, inside in ((30, 36, 0), (31, 44, 1), (W - 32, 52, 1), (W - 31, 60, 0),
                             (50, 30, 0), (60, 31, 1), (70, H - 32, 1), (80, H - 31, 0),
                             (31, 31, 1), (W - 32, H - 32, 1)):
            img[y, x] = 150
            if inside:
                present[(x, y)] = 49
            else:
                absent.append((x, y))
        # a stronger corner outside the border suppresses its neighbour inside
        for (xo, yo), (xi, yi) in (((30, 52), (31, 52)), ((W - 31, 40), (W - 32, 40)), ((90, 30), (90, 31)), ((112, H - 31), (112, H - 32))):
            img[yo, xo] = 160
            img[yi, xi] = 150
            absent += [(xo, yo), (xi, yi)]

        def prove(r):
            sc = orb_ref.fast_scores(r["img"])
            for x, y in absent:
                assert sc[y, x] >= 49                    # a FAST corner; only the NMS or the border removes it
            expect_l0(r, present, absent)
            assert len(l0(r)) == len(present)
        return img, prove
    fn.__name__ = "border_w%d" % W
    fn.__doc__ = ("dots at x = 30, 31, w - 32, w - 31 and likewise in y: 31 and w - 32 are kept; a stronger dot at 30 suppresses its "
                  "neighbour at 31 (NMS before the border filter); w = %d, w mod 4 = %d for the dword over the right edge" % (W, W % 4))
    return fn


for _W in (128, 129, 130, 131):
    case(_W, 96, fast=True)(_border(_W))


@functools.lru_cache(maxsize=None)
def _upper_level_blobs(W, H, level):
    """Positions of (level + 1) x (level + 1) blobs on level 0 whose corner on `level` lands on that level's x = 31, x = w - 32,
    y = 31, y = h - 32: found by searching with the twin's resize and FAST."""
    w, h, _, _ = orb_ref.geometry(W, H)
    lw, lh = int(w[level]), int(h[level])
    s = float(orb_ref.geometry(W, H)[2][level])
    found = {}

    def corners_of(px, py):
        img = flat(W, H)
        img[py:py + level + 1, px:px + level + 1] = 220
        lv = img
        for l in range(1, level + 1):
            lv = orb_ref.resize_fixed(lv, int(w[l]), int(h[l]))
        return orb_ref.fast_corners(lv)

    targets = {"x_lo": (0, 31), "x_hi": (0, lw - 32), "y_lo": (1, 31), "y_hi": (1, lh - 32)}
    for name, (axis, t) in targets.items():
        centre = int(round(t * s))
        mid = int(round((lh if axis == 0 else lw) // 2 * s))
        # along the border: a few positions around the target; across it: off the middle, the two sides on different offsets
        tries = [(p, a) for a in ((mid - 4, mid - 12) if name.endswith("hi") else (mid + 8, mid + 4))
                 for p in range(centre - 3, centre + 4)]
        for p, across in tries:
            px, py = (p, across) if axis == 0 else (across, p)
            hit = [tuple(int(v) for v in row) for row in corners_of(px, py) if row[axis] == t]
            if hit:
                found[name] = ((px, py), hit[0])
                break
    return found


def _border_level(W, H, level):
    def fn():
        found = _upper_level_blobs(W, H, level)
        img = flat(W, H)
        for (px, py), _ in found.values():
            img[py:py + level + 1, px:px + level + 1] = 220

        def prove(r):
            assert sorted(found) == ["x_hi", "x_lo", "y_hi", "y_lo"], found
            got = {(int(x), int(y)): int(s) for x, y, s in r["corners"][level]}
            for name, (_, (x, y, s)) in found.items():
                assert got.get((x, y)) == s, (name, (x, y, s), got)
        return img, prove
    fn.__name__ = "border_level%d" % level
    fn.__doc__ = ("blobs placed (by search with the twin's resize) so that their LEVEL-%d corners sit on that level's x = 31, "
                  "x = w - 32, y = 31 and y = h - 32: the border filter and the right edge on a level the pyramid kernels wrote" % level)
    return fn


case(128, 96, fast=True)(_border_level(128, 96, 1))
case(192, 128, fast=True)(_border_level(192, 128, 2))
case(SW, SH, 500, fast=True)(_border_level(SW, SH, 3))


# ---- selection: retainBest's target ----------------------------------------------------------------------------------------------
def _block(img, x0, y0, v):
    """A bright block from (x0, y0) to the image's bottom right, its corner pixel one grey level brighter (a plain block's
    corner ties with its neighbours and strict NMS removes them all): its only FAST corner is (x0, y0), score v - bg, and its
    Harris measure is far above a dot's."""
    img[y0:, x0:] = v
    img[y0, x0] = v + 1


@case(SW, SH, 8)
def target_exact4():
    """max_kp 8: quota 2, target 4, and exactly 4 level-0 corners with distinct scores: nothing is cut by FAST score"""
    img = flat(SW, SH)
    for i, d in enumerate((40, 50, 60, 70)):
        img[60, 60 + 20 * i] = BG + d

    def prove(r):
        assert int(r["quota"][0]) == 2 and len(l0(r)) == 4
        kept, T = orb_ref.retain_best(r["corners"][0], 2)
        assert len(kept) == 4 and T == 0
        assert l0_kps(r) == [(120, 60), (100, 60)]
    return img, prove


@case(SW, SH, 8)
def target_5_distinct():
    """5 level-0 corners with distinct scores, the weakest with by far the largest Harris measure: it is cut BEFORE Harris"""
    img = flat(SW, SH)
    for i, d in enumerate((40, 41, 42, 43)):
        img[60, 60 + 20 * i] = BG + d
    _block(img, 250, 250, BG + 30)

    def prove(r):
        c = l0(r)
        assert len(c) == 5 and c[(250, 250)] == 30
        kept, T = orb_ref.retain_best(r["corners"][0], 2)
        assert T == 39 and len(kept) == 4
        R = orb_ref.harris(r["img"], [250, 120], [250, 60])
        assert R[0] > R[1]                                   # it would have won
        assert l0_kps(r) == [(120, 60), (100, 60)]
    return img, prove


@case(SW, SH, 8)
def target_5_tied():
    """5 level-0 corners, the two weakest tied at the target: all five reach Harris and the last one in raster order wins it"""
    img = flat(SW, SH)
    for i, d in enumerate((41, 42, 43, 31)):
        img[60, 60 + 20 * i] = BG + d
    _block(img, 250, 250, BG + 30)

    def prove(r):
        c = l0(r)
        assert len(c) == 5 and c[(250, 250)] == 30 and c[(120, 60)] == 30
        kept, T = orb_ref.retain_best(r["corners"][0], 2)
        assert T == 30 and len(kept) == 5
        assert l0_kps(r)[0] == (250, 250)
    return img, prove


# ---- selection: Harris ties, the sort's padding, CAP1 ----------------------------------------------------------------------------
def grid_dots(n, v=150, bg=BG, per_row=32, W=SW, H=SH):
    img = flat(W, H, bg)
    pts = [(33 + 8 * (k % per_row), 33 + 8 * (k // per_row)) for k in range(n)]
    for x, y in pts:
        img[y, x] = v
    return img, pts


def _identical(n, per_row):
    def fn():
        img, pts = grid_dots(n, per_row=per_row)

        def prove(r):
            c = l0(r)
            assert len(c) == n and set(c.values()) == {49}           # exactly n level-0 corners of one score
            kept, T = orb_ref.retain_best(r["corners"][0], 2)
            if n <= orb_ref.CAP1:
                assert len(kept) == n and T == (49 if n > 4 else 0)
                R = orb_ref.harris(r["img"], kept[:, 0], kept[:, 1])
                assert len(set(R)) == 1                               # R equal for all candidates
                assert l0_kps(r) == pts[:2] if n > 1 else l0_kps(r) == pts       # raster order, y before x
            else:
                assert len(kept) == 0 and T == 50                     # CAP1: the threshold passes every corner
                assert l0_kps(r) == []
        return img, prove
    return fn


for _n, _pr, _doc in ((1, 8, "1 candidate"), (64, 8, "64 candidates in 8 rows of 8: the bitonic sort needs no padding"),
                      (65, 8, "65 candidates: the sort pads to 128"),
                      (1024, 32, "1,024 candidates: the full table, exactly CAP1; level 0 is filled in raster order"),
                      (1025, 32, "1,025 identical dots: CAP1 raises the threshold past all of them and level 0 is EMPTY")):
    _f = _identical(_n, _pr)
    _f.__name__ = "identical_%d" % _n
    _f.__doc__ = "identical dots tie in FAST score and in the Harris measure, so the cut falls by raster order; " + _doc
    case(SW, SH, 8)(_f)


@case(SW, SH, 8)
def cap1_plus_strong():
    """1,025 identical dots and one stronger dot: the raised threshold leaves only that one"""
    img, pts = grid_dots(1025)
    img[297, 305] = 250

    def prove(r):
        c = l0(r)
        assert len(c) == 1026 and c[(305, 297)] == 149
        kept, T = orb_ref.retain_best(r["corners"][0], 2)
        assert T == 50 and len(kept) == 1
        assert l0_kps(r) == [(305, 297)]
    return img, prove


@case(SW, SH, 500)
def regular_texture_1188():
    """grey 60 with dots of 200 on the 8-pixel grid from (33, 33), 36 x 33 = 1,188 dots: every level-0 corner scores 139, CAP1
    empties level 0 (OpenCV keeps ties and would return the quota of 109 there); 280 keypoints, 90 / 75 / 63 / 52 on levels 1-4"""
    img, pts = grid_dots(1188, v=200, bg=60, per_row=36)

    def prove(r):
        c = l0(r)
        assert len(c) == 1188 and set(c.values()) == {139}
        assert [len(x) for x in r["corners"][1:5]] == [1088, 896, 404, 52]
        assert int(r["quota"][0]) == 109
        n = np.bincount(r["kp"]["octave"], minlength=8).tolist()
        assert len(r["kp"]) == 280 and n == [0, 90, 75, 63, 52, 0, 0, 0], n
    return img, prove


# ---- selection: quota 0, quota within SVO_QMAX -----------------------------------------------------------------------------------
def _blocky(max_kp):
    def fn():
        img = util.blocky_image(0, SW, SH)

        def prove(r):
            q = r["quota"]
            n = np.bincount(r["kp"]["octave"], minlength=8)
            assert len(r["corners"][7]) > 0
            if max_kp in (8, 9):
                assert int(q[7]) == 0 and n[7] == 0 and len(r["kp"]) == max_kp
                assert q.tolist() == ([2, 1, 1, 1, 1, 1, 1, 0] if max_kp == 8 else [2, 2, 1, 1, 1, 1, 1, 0])
            else:
                assert q.tolist() == [111, 93, 77, 64, 54, 45, 37, 31] and n[0] == 111 and n[7] > 0
        return img, prove
    fn.__name__ = "blocky_kp%d" % max_kp
    fn.__doc__ = ("a textured 352 x 330 image at max_kp %d: " % max_kp) + (
        "level 7 has corners but quota 0" if max_kp < 10 else "quota 111 on level 0, within SVO_QMAX = 128; descriptors at every angle, one of "
        "them with a rotated pattern coordinate on an exact .5 (cvRound's half-to-even)")
    return fn


for _k in (8, 9, 512):
    case(SW, SH, _k)(_blocky(_k))


# ---- orientation and descriptor --------------------------------------------------------------------------------------------------
def _kp_at(r, x, y):
    k = r["kp"]
    i = np.nonzero((k["octave"] == 0) & (k["x"] == x) & (k["y"] == y))[0]
    assert len(i) == 1, ("no level-0 keypoint at", (x, y))
    return int(i[0])


@case(192, 128)
def lone_dot():
    """a lone dot: m10 = m01 = 0, the (0, 0) case of fastAtan2; angle 0"""
    img = flat(192, 128)
    img[64, 96] = 200

    def prove(r):
        m10, m01 = orb_ref.moments(r["img"], [96], [64])
        assert (int(m10[0]), int(m01[0])) == (0, 0)
        assert r["kp"]["angle"][_kp_at(r, 96, 64)] == 0.0
    return img, prove


def _satellite(dx, dy, want):
    def fn():
        img = flat(192, 128)
        img[64, 96] = 200
        img[64 + dy - 1:64 + dy + 2, 96 + dx - 1:96 + dx + 2] = 180

        def prove(r):
            m10, m01 = orb_ref.moments(r["img"], [96], [64])
            m10, m01 = int(m10[0]), int(m01[0])
            assert (np.sign(m10), np.sign(m01)) == (np.sign(dx), np.sign(dy))
            if dx and dy:
                assert abs(m10) == abs(m01)                   # ax == ay: the branch switch of fastAtan2
            a = float(r["kp"]["angle"][_kp_at(r, 96, 64)])
            assert a == want, (a, want)
        return img, prove
    return fn


# the angles are what the polynomial delivers (the twin says which): exact on the axes, 44.99... on the diagonal
for _n, _dx, _dy, _a in (("satellite_east", 10, 0, 0.0), ("satellite_south", 0, 10, 90.0), ("satellite_west", -10, 0, 180.0),
                         ("satellite_north", 0, -10, 270.0), ("satellite_diagonal", 7, 7, float(orb_ref.fast_atan2(1.0, 1.0)))):
    _f = _satellite(_dx, _dy, _a)
    _f.__name__ = _n
    _f.__doc__ = "a dot with a 3 x 3 blob at (%d, %d) from it (y down): angle %r" % (_dx, _dy, _a)
    case(192, 128)(_f)


def _saturated(bg, v):
    def fn():
        img = flat(192, 128, bg)
        img[64, 96] = v
        img[31, 31] = v                                # window extremes: the staged windows' first and last rows and bytes
        img[128 - 32, 192 - 32] = v

        def prove(r):
            for x, y in ((96, 64), (31, 31), (160, 96)):
                _kp_at(r, x, y)
            if bg == 255:
                p = np.pad(r["img"].astype(np.int64), 3, mode="reflect")
                hor = sum(orb_ref.GAUSS7[k] * p[3:-3, k:k + 192] for k in range(7))
                assert hor.max() == 65535                                   # the 16-bit horizontal pass is full
                ver = sum(orb_ref.GAUSS7[k] * np.pad(hor, ((3, 3), (0, 0)), mode="reflect")[k:k + 128] for k in range(7))
                assert ((ver + 32768) >> 16).max() == 257                   # and the clamp is taken
                assert orb_ref.blur(r["img"]).max() == 255
        return img, prove
    return fn


for _n, _bg, _v, _d in (("dark_dot_on_255", 255, 0, "a dark dot on an all-255 field: the horizontal blur pass sits at 65,535 and the clamp is taken"),
                        ("bright_dot_on_0", 0, 255, "a bright dot on an all-0 field")):
    _f = _saturated(_bg, _v)
    _f.__name__ = _n
    _f.__doc__ = _d + "; keypoints at (31, 31) and (w - 32, h - 32), the outermost windows k_describe ever reads"
    case(192, 128)(_f)


NAMES = list(CASES)
FAST_NAMES = [n for n in NAMES if CASES[n]["fast"]]


@functools.lru_cache(maxsize=None)
def image(name):
    c = CASES[name]
    img, _ = c["build"]()
    assert img.shape == (c["H"], c["W"]) and img.dtype == np.uint8
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def reference(name):
    """The twin's result for a case (computed once per session and shared; do not modify)."""
    r = orb_ref.extract(image(name), CASES[name]["max_kp"])
    r["img"] = image(name)
    return r


def prove(name):
    _, p = CASES[name]["build"]()
    p(reference(name))


def contexts():
    return sorted({(c["W"], c["H"], c["max_kp"]) for c in CASES.values()})
