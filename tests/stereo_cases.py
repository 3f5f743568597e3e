"""Hand-made inputs of the sparse stereo matcher, shared by tests/test_stereo_cpu.py (the twin tests/stereo_ref.py against
orc_stereo_match, and every case's CONDITIONS: the exits and ties it was made to reach) and tests/test_stereo_gpu.py
(svo_debug_stereo_match against both).  ORB never produces such keypoints: they sit on the limits of the SAD windows, of
the row bands and of the gates, share rows by the hundred, tie in Hamming distance and in SAD.

A case is a dict: W, H, max_kp, L, R (uint8 images), kpL, dL, kpR, dR, fx, bf, `need` ({reason or flag of stereo_ref.tally:
minimum count}), `partner` ({left index: right index the Hamming search must find}), `missed` ({left index: right index
it must NOT find}), `sads` (sorted best SADs of the accepted keypoints, or None).  A left keypoint's partner carries its
descriptor, or util.flip_bits of it; all other descriptors are random (unrelated pairs sit near 128 bits).
"""
import math

import numpy as np

import stereo_ref
import util

F = np.float32
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


class _Case:
    def __init__(self, name, W, H, L, R, fx=200.0, bf=386.1448, max_kp=64, seed=1):
        self.name, self.W, self.H, self.L, self.R = name, W, H, np.ascontiguousarray(L), np.ascontiguousarray(R)
        self.fx, self.bf, self.max_kp = fx, bf, max_kp
        self.rng = np.random.default_rng(seed)
        self.l, self.r, self.dl, self.dr = [], [], [], []
        self.need, self.partner, self.missed, self.sads = {}, {}, {}, None
        self.w, self.h, self.scale = stereo_ref.geometry(W, H)

    def desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def left(self, x, y, octave, d=None):
        self.l.append((x, y, octave)); self.dl.append(self.desc() if d is None else d)
        return len(self.l) - 1

    def right(self, x, y, octave, d=None):
        self.r.append((x, y, octave)); self.dr.append(self.desc() if d is None else d)
        return len(self.r) - 1

    def pair(self, xl, yl, ol, xr, yr=None, orr=None, bits=0, found=True):
        """A left keypoint and its partner (descriptor `bits` bits apart).  found: whether the gates let the search see it."""
        d = self.desc()
        i = self.left(xl, yl, ol, d)
        j = self.right(xr, yl if yr is None else yr, ol if orr is None else orr, util.flip_bits(d, bits, self.rng) if bits else d.copy())
        (self.partner if found else self.missed)[i] = j
        return i, j

    def at(self, coord, octave):
        """Level-0 coordinate of level coordinate `coord`: coord * scale[octave] (the twin confirms that it rounds back)."""
        v = F(coord) * self.scale[octave]
        assert stereo_ref.roundf(v * (F(1) / self.scale[octave])) == coord
        return v

    def done(self):
        def kps(lst):
            k = np.zeros(len(lst), KP_DTYPE)
            for i, (x, y, o) in enumerate(lst):
                k[i]["x"], k[i]["y"], k[i]["octave"] = x, y, o
                k[i]["size"], k[i]["angle"], k[i]["response"], k[i]["class_id"] = 31.0, 0.0, 1.0, -1
            return k
        assert len(self.l) <= self.max_kp and len(self.r) <= self.max_kp, self.name
        return dict(name=self.name, W=self.W, H=self.H, max_kp=self.max_kp, L=self.L, R=self.R, fx=self.fx, bf=self.bf,
                    kpL=kps(self.l), dL=np.array(self.dl, np.uint8).reshape(-1, 32),
                    kpR=kps(self.r), dR=np.array(self.dr, np.uint8).reshape(-1, 32),
                    need=self.need, partner=self.partner, missed=self.missed, sads=self.sads)


def _pair(seed, W, H, disparity):
    """util.shifted_pair with a few gray levels of noise on the right image: best SADs, and so the median, are above 0."""
    L, R = util.shifted_pair(seed, W, H, disparity=disparity)
    noise = np.random.default_rng(seed + 1000).integers(-2, 3, R.shape)
    return L, np.clip(R.astype(np.int64) + noise, 0, 255).astype(np.uint8)


# ---- borders ---------------------------------------------------------------------------------------------------------------------
def _borders(W):
    """Identical images.  On every level: the left window one off and one on each of its four limits (su, sv in {4, 5} and
    {l - 6, l - 5}), the right search band likewise (sr0 in {9, 10} and {lw - 11, lw - 10}).  W = 192: level 0 (192) and
    level 6 (64) have pitch == width, so the window loads of the last legal row run into what follows the level."""
    H = 128
    img = util.blocky_image(W + 3, W, H)
    c = _Case("borders_%d" % W, W, H, img, img, fx=400.0, max_kp=128, seed=W)
    for l in range(8):
        lw, lh = c.w[l], c.h[l]
        assert lw >= 23 and lh >= 12
        cu, cv = lw // 2, lh // 2
        for sv in (4, 5, lh - 6, lh - 5):           # partner in the same place: disparity 0 where the window is legal
            c.pair(c.at(cu, l), c.at(sv, l), l, c.at(cu, l))
        for su in (4, 5, lw - 6, lw - 5):           # partner 5 px to the left at the level (it has to be left of su)
            c.pair(c.at(su, l), c.at(cv, l), l, c.at(max(su - 5, 0), l))
        for sr0 in (9, 10):
            c.pair(c.at(cu, l), c.at(cv - 2, l), l, c.at(sr0, l))
        c.pair(c.at(lw - 6, l), c.at(cv + 2, l), l, c.at(lw - 11, l))
        c.pair(c.at(lw - 6, l), c.at(cv - 4, l), l, c.at(lw - 10, l))
        # the last legal row AND column at once: where the loads end furthest
        c.pair(c.at(lw - 6, l), c.at(lh - 6, l), l, c.at(lw - 11, l))
    c.need = dict(left_top=8, left_bottom=8, left_left=8, left_right=8, right_left=16, right_right=8, sad_min_last=16)
    return c.done()


# ---- band ------------------------------------------------------------------------------------------------------------------------
def _y_with(target, r, kind, lo, hi, last=False):
    """The first (last) y = k / 16 in [lo, hi) with ceil(y + r) == target (kind 'max') or floor(y - r) == target (kind 'min')."""
    ks = range(int(lo * 16), int(hi * 16))
    for k in (reversed(ks) if last else ks):
        y = F(k / 16.0)
        v = math.ceil(float(y + r)) if kind == "max" else math.floor(float(y - r))
        if v == target:
            return y
    raise AssertionError("no such row")


def _band():
    W, H = 160, 128
    L, R = _pair(41, W, H, 6)
    c = _Case("band", W, H, L, R, max_kp=256, seed=41)
    x = 30.0
    for l in range(8):
        row = 30 + 9 * l
        for ro in (l - 1, l, l + 1):                 # the band is the RIGHT keypoint's: 2 * scale[its octave]
            if not 0 <= ro <= 7 or (ro != l and l % 2):
                continue
            r = F(2.0) * c.scale[ro]
            for kind, target, found in (("max", row, True), ("max", row - 1, False), ("min", row, True), ("min", row + 1, False)):
                for yl in (float(row), row + 0.75):  # (int)y is the row
                    x += 3.0
                    if x > 150:
                        x = 33.0
                    c.pair(x, yl, l, x - 6.0, _y_with(target, r, kind, 0, H), ro, found=found)
    for l in range(8):                               # octaves levelL - 2 .. levelL + 2, in the middle of the band
        for ro in range(l - 2, l + 3):
            if 0 <= ro <= 7:
                x += 3.0
                if x > 150:
                    x = 33.0
                c.pair(x, 20.0 + l, l, x - 6.0, 20.0 + l, ro, found=abs(ro - l) <= 1)
    c.need = dict(accepted=20)
    return c.done()


# ---- gates -----------------------------------------------------------------------------------------------------------------------
def _gates():
    """fx = 20: maxD = 20.  Top half of the pair: true disparity -1 (a partner at u == uL refines to a negative disparity);
    bottom half: 21 (a partner at u == minU refines to a disparity >= maxD)."""
    W, H, fx = 160, 128, 20.0
    big = util.blocky_image(43, W + 64, H)
    L = big[:, 32:32 + W]
    R = L.copy()
    R[:64] = big[:64, 31:31 + W]                     # R[x] = L[x - 1]
    R[64:] = big[64:, 53:53 + W]                     # R[x] = L[x + 21]
    c = _Case("gates", W, H, L, R, fx=fx, max_kp=64, seed=43)
    uL = F(100.0)
    minU = uL - F(fx)
    up, dn = np.nextafter(uL, F(np.inf)), np.nextafter(minU, F(-np.inf))
    rows = iter(range(10, 64, 5))
    c.pair(uL, next(rows), 0, uL)                                  # disparity 0 at the gate, -1 after the parabola
    c.pair(uL, next(rows), 0, minU)
    c.pair(uL, next(rows), 0, up, found=False)
    c.pair(uL, next(rows), 0, dn, found=False)
    c.pair(uL, next(rows), 0, uL + F(10), found=False)
    c.pair(uL, next(rows), 0, minU - F(10), found=False)
    c.pair(F(-1.0), next(rows), 0, F(-1.0), found=False)           # maxU < 0
    c.pair(F(-0.0), next(rows), 0, F(0.0))                         # -0.0 is not < 0: searched, then the window leaves the level
    c.pair(F(30.0), next(rows), 0, F(30.0) - F(1.0))               # (the 0.01 substitution cannot follow a non-zero shift)
    rows = iter(range(72, 120, 5))
    c.pair(uL, next(rows), 0, minU)                                # disparity 20 at the gate, 21 after the parabola
    c.pair(uL, next(rows), 0, uL)
    c.pair(uL, next(rows), 0, up, found=False)
    c.pair(uL, next(rows), 0, dn, found=False)
    c.pair(uL, next(rows), 0, uL - F(19.0))                        # 19 -> 21 by the SAD search: still rejected
    c.pair(F(60.0), next(rows), 0, F(60.0) - F(17.0))
    c.need = dict(maxu_negative=1, left_left=1, no_candidate=6, disparity_range=3)
    return c.done()


# ---- hamming ---------------------------------------------------------------------------------------------------------------------
def _hamming():
    W, H = 160, 128
    L, R = _pair(47, W, H, 8)
    c = _Case("hamming", W, H, L, R, max_kp=256, seed=47)
    for k, bits in enumerate((0, 74, 75, 99, 100)):
        c.pair(60.0 + 7 * k, 12.0 + 4 * k, 0, 52.0 + 7 * k, bits=bits)
    # two candidates at the same distance; the HIGHER index in an EARLIER row bucket (rows 58 < 60), the lower index is the true match
    d = c.desc()
    i = c.left(90.0, 60.0, 0, d)
    lo = c.right(82.0, 61.0, 0, util.flip_bits(d, 10, c.rng))
    fill = [c.right(20.0, 100.0, 5) for _ in range(3)]
    hi = c.right(60.0, 59.0, 0, util.flip_bits(d, 10, c.rng))
    assert lo < fill[0] < hi
    c.partner[i] = lo
    # three equal candidates behind more than 64 entries of the same bucket scan (rows 85 .. 95 of a left keypoint in row 94): the wave
    # meets them in its second pass, in lanes of their own
    for _ in range(70):
        c.right(float(c.rng.integers(12, 150)), float(c.rng.integers(85, 91)), 4)
    d = c.desc()
    i = c.left(100.0, 94.0, 0, d)
    first = c.right(92.0, 94.0, 0, util.flip_bits(d, 20, c.rng))
    c.right(70.0, 95.0, 0, util.flip_bits(d, 20, c.rng))
    c.right(50.0, 95.5, 1, util.flip_bits(d, 20, c.rng))
    c.partner[i] = first
    c.need = dict(hamming_75_99=2, hamming_ge_100=1, ham_tie=2, accepted=3)
    return c.done()


# ---- crowded row -----------------------------------------------------------------------------------------------------------------
def _crowded(variant):
    """512 right keypoints with (int)y == 70: one bucket, eight passes of the wave; nL = 37 (no multiple of 4)."""
    W, H = 160, 128
    L, R = _pair(53, W, H, 8)
    c = _Case("crowded_row" + variant, W, H, L, R, max_kp=512, seed=53)
    nl = 0 if variant == "_nL0" else 37
    for i in range(nl):
        x = 24.0 + 3.0 * i
        c.pair(x, 69.0 + (i % 3), i % 2, x - 8.0, 70.0 + (i % 4) / 4.0, (i % 2) + (i % 3 == 0), bits=i % 11)
    want = 0 if variant == "_nR0" else 512
    if variant == "_nR0":
        c.r, c.dr, c.partner = [], [], {}
    while len(c.r) < want:
        c.right(float(c.rng.integers(0, 4 * W)) / 4.0, 70.0 + float(c.rng.integers(0, 8)) / 8.0, int(c.rng.integers(0, 4)))
    c.need = dict(no_candidate=37) if variant == "_nR0" else ({} if variant == "_nL0" else dict(accepted=12))
    return c.done()


# ---- SAD ties --------------------------------------------------------------------------------------------------------------------
def _sad_ties():
    """Rows 0 .. 63: columns of period 4, L == R - the SAD of shift inc is 0 wherever sr0 + inc - su is a multiple of 4: ties, the
    first of them must win.  Rows 64 ..: blocky, R = L shifted by 3 + noise - one minimum; one partner puts it at inc = +5."""
    W, H = 160, 128
    img = np.tile((np.arange(W) % 4 * 60).astype(np.uint8), (H, 1))
    img[64:] = util.blocky_image(59, W, H)[64:]
    R = img.copy()                                   # the blocky half: R[x] = L[x + 3] + noise - best SADs above 0, so that the median is and the ties survive the cut
    R[64:, :W - 3] = np.clip(img[64:, 3:].astype(np.int64) + np.random.default_rng(60).integers(-3, 4, (H - 64, W - 3)), 0, 255).astype(np.uint8)
    c = _Case("sad_ties", W, H, img, R, fx=30.0, max_kp=64, seed=59)
    for k in range(12):                              # partner k px to the left: zeros at inc = k (mod 4)
        c.pair(40.0 + 6 * k, 8.0 + 4 * k, 0, 40.0 + 6 * k - k)
    c.pair(80.0, 70.0, 0, 72.0)                      # the one minimum at inc = +5
    for k in range(12):
        c.pair(30.0 + 9 * k, 74.0 + 4 * k, 0, 27.0 + 9 * k)
    c.need = dict(sad_tie=12, sad_min_first=3, sad_min_last=1, accepted=21)
    return c.done()


# ---- zero disparity, zero median ---------------------------------------------------------------------------------------------------
def _zero_disparity(noisy):
    """L is its own mirror image about column 80 and R == L there: at x = 80 the SADs of +inc and -inc are equal, the parabola's
    vertex is exactly 0 and the disparity exactly 0 -> 0.01.  Alone (median_zero) every best SAD is 0, the median is 0 and the
    cut removes everything.  With 14 keypoints of disparity 4 in columns 15 .. 45, where R carries noise, the median is > 0."""
    W, H = 160, 128
    L = util.blocky_image(61, W, H)
    L[:, 81:] = L[:, 79:0:-1]
    R = L.copy()
    c = _Case("zero_disparity" if noisy else "median_zero", W, H, L, R, max_kp=64, seed=61)
    for k in range(11):
        c.pair(80.0, 8.0 + 11 * k, 0, 80.0)
    if noisy:
        noise = c.rng.integers(-3, 4, (H, 45))
        R[:, 5:50] = np.clip(L[:, 9:54].astype(np.int64) + noise, 0, 255).astype(np.uint8)     # R[x] = L[x + 4] + noise
        c.R = R
        for k in range(14):
            c.pair(22.0 + (k % 5) * 4, 9.0 + 8 * k, 0, 18.0 + (k % 5) * 4)
        c.need = dict(substituted=11, substituted_kept=11, accepted=25)
    else:
        c.need = dict(substituted=11, cut=11)
    return c.done()


# ---- median ----------------------------------------------------------------------------------------------------------------------
def _median(name, sads):
    """Keypoints whose best SADs are the given integers: R is L shifted by 6, and the partner's window has one pixel (not its
    centre) raised or lowered by the wanted SAD - the SAD at the true shift is that number, every other shift's is in the hundreds."""
    W, H = 160, 128
    L, R = util.shifted_pair(67, W, H, disparity=6)
    R = R.copy()
    c = _Case(name, W, H, L, R, max_kp=16, seed=67)
    slots = [(x, y) for y in (16, 44, 72, 100) for x in (40, 80, 120)]
    for (x, y), s in zip(slots, sads):
        c.pair(float(x), float(y), 0, float(x - 6))
        py, px = y - 3, x - 6 + 2
        v = int(R[py, px])
        R[py, px] = v + s if v + s <= 255 else v - s
    c.R = R
    c.sads = sorted(sads)
    c.need = dict(accepted=len(sads))
    return c


def _median_cases():
    out = []
    for name, sads, cut in (("median_nd1", [7], 0), ("median_nd2", [30, 10], 0), ("median_nd3", [5, 30, 10], 1),
                            ("median_even_equal", [9, 9, 9, 9], 0),
                            # median 10 (rank 4 of 8, equal SADs at ranks 2, 3, 4); 2.1f * 10.0f rounds to 21.0f: 20 stays, 21 and 22 go
                            ("median_edge", [21, 10, 4, 22, 10, 20, 5, 10], 2)):
        c = _median(name, sads)
        if cut:
            c.need["cut"] = cut
        out.append(c.done())
    return out


# ---- small contexts --------------------------------------------------------------------------------------------------------------
def _small_ctx(max_kp):
    """max_kp = 8 and 500: no multiple of 64 - the last workgroup of the grid is partial and its keypoint loads are clamped."""
    W, H = 160, 128
    L, R = _pair(71, W, H, 7)
    c = _Case("small_ctx_%d" % max_kp, W, H, L, R, max_kp=max_kp, seed=71 + max_kp)
    for i in range(max_kp - 1):
        o = int(c.rng.integers(0, 4))
        x = float(c.rng.integers(int(20 * c.scale[o]), int(W - 8 * c.scale[o])))
        y = float(c.rng.integers(int(7 * c.scale[o]), int(H - 8 * c.scale[o])))
        c.pair(x, y, o, x - 7.0, bits=int(c.rng.integers(0, 60)))
    c.right(50.0, 50.0, 2)
    c.need = dict(accepted=max_kp // 2)
    return c.done()


# ---- tall images -----------------------------------------------------------------------------------------------------------------
def _tall(W, H):
    """H >= 512: the 512 row buckets hold 2, 4, 8 rows (bshift 1, 2, 3).  Left keypoints of octave 6 in every row from 10 above
    to 10 below a bucket edge E, each with a partner of octave 7 (band 2 * 3.58) as far above or below as its band reaches - in
    the first and the last bucket the scan of that row covers; rows 0 and H - 1; right keypoints in the first and last bucket."""
    L, R = _pair(H, W, H, 8)
    c = _Case("tall_%d" % H, W, H, L, R, max_kp=128, seed=H)
    bshift = 0
    while (H >> bshift) >= 512:
        bshift += 1
    assert bshift == {600: 1, 1100: 2, 2100: 3}[H]
    E = (H // 2) >> bshift << bshift
    r7 = F(2.0) * c.scale[7]
    lw = c.w[6]
    xs = [c.at(su, 6) for su in range(14, lw - 6)]
    k = 0
    for rc in range(E - 10, E + 11):
        for kind in ("max", "min"):                   # partner above (its maxr == rc) and below (its minr == rc)
            x = xs[k % len(xs)]; k += 1
            c.pair(x, float(rc), 6, x - F(8.0), _y_with(rc, r7, kind, 0, H, last=kind == "min"), 7)     # rows rc - 9 and rc + 8
    for y in (0.0, 3.5, H - 1.0, H - 1.5):            # first and last row / bucket: searched, then the window leaves the level
        c.pair(40.0, y, 0, 32.0)
    c.pair(c.at(14, 6), float(H - 7), 6, c.at(14, 6) - F(8.0), H - 1.0, 7)
    c.pair(c.at(15, 6), 6.0, 6, c.at(15, 6) - F(8.0), 0.25, 7)
    c.need = dict(accepted=20, left_top=2, left_bottom=2)
    return c.done()


def _build():
    cases = [_borders(160), _borders(192), _band(), _gates(), _hamming(), _crowded(""), _crowded("_nR0"), _crowded("_nL0"),
             _sad_ties(), _zero_disparity(True), _zero_disparity(False)] + _median_cases() + \
            [_small_ctx(8), _small_ctx(500), _tall(160, 600), _tall(128, 1100), _tall(96, 2100)]
    return {c["name"]: c for c in cases}


CASES = _build()
NAMES = list(CASES)
# every exit of the matcher and every tie that the cases together must reach ("parabola" is unreachable: see the note at the branch)
ALL_REACHED = [r for r in stereo_ref.REASONS if r != "parabola"] + ["ham_tie", "sad_tie", "substituted", "substituted_kept", "cut"]

_REF = {}


def reference(name, orc):
    """(twin result, oracle uR, oracle depth) of a case, computed once per session and shared; callers leave it unchanged."""
    if name not in _REF:
        c = CASES[name]
        pL, pR = orc.build_pyramid(c["L"]), orc.build_pyramid(c["R"])
        twin = stereo_ref.match(stereo_ref.split_pyramid(pL, c["W"], c["H"]), stereo_ref.split_pyramid(pR, c["W"], c["H"]),
                                c["W"], c["H"], c["kpL"], c["dL"], c["kpR"], c["dR"], c["bf"], c["fx"])
        uR, depth, _ = orc.stereo_match(pL, pR, c["W"], c["H"], c["kpL"], c["dL"], c["kpR"], c["dR"], c["bf"], c["fx"])
        _REF[name] = (twin, uR, depth)
    return _REF[name]
