"""numpy twin of the ORB extraction (csrc/svo_orb.hip, oracle/orc_orb.c), written from the definitions in DESIGN.md section 3 and
SURVEY.md section 8 a-notes - not from either implementation.  Where those two use a closed form or a shortcut, this file uses
the definition: FAST by the literal arc test, retainBest by sorting, Harris in Python integers and one exact rational rounding,
the disc from its geometric construction, the Gaussian over the whole level with REFLECT_101.

Every stage function takes the previous stage's output as an argument, so a test can feed it the DEVICE's previous stage (which
names the stage that failed) as well as the twin's own (the whole chain): `extract` is nothing but their composition.

`Rules` holds the rules as switches.  The defaults are the documented ones; tests/test_orb_cpu.py flips one at a time and shows
that a named case of tests/orb_cases.py notices (a mutant that no case kills is a rule no case pins)."""
import os
import re
from fractions import Fraction

import numpy as np

NLEVELS = 8
FAST_THR = 20
EDGE = 31
CAP1 = 1024
HALF_PATCH = 15
UMAX_TABLE = (15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3)

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

# ring of radius 3, 16 pixels, clockwise from (0, 3) in image coordinates (y down)
RING_X = np.array([0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1])
RING_Y = np.array([3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3])


class Rules:
    """The rules of DESIGN.md section 3 as switches; every default is the documented rule."""
    arc = 9                  # contiguous ring pixels a corner needs
    contrast_strict = True   # ring > c + t  /  ring < c - t
    nms_strict = True        # a corner's eight neighbours must all score strictly less
    border_first = False     # the 31-pixel border filter comes AFTER the NMS
    border = EDGE
    keep_ties = True         # retainBest keeps everything that ties with the (2 * quota)-th score
    cap1 = True              # more than CAP1 survivors: raise the threshold until they fit
    tie_y_first = True       # equal Harris measure: raster order, y before x
    quota_extra = 0
    use_umax = True          # moments over the radius-15 disc, not the 31 x 31 square
    atan_ge = True           # fastAtan2 takes the first branch at ax == ay
    blur_clamp = True        # (sum + 2^15) >> 16 saturates at 255
    half_even = True         # cvRound: round half to even
    bit_strict = True        # bit = t0 < t1

    def __init__(self, **kw):
        for k, v in kw.items():
            assert hasattr(Rules, k), k
            setattr(self, k, v)


DEFAULT = Rules()
f32 = np.float32


# ---- geometry ------------------------------------------------------------------------------------------------------------------
def geometry(W, H, max_kp=500):
    """Level sizes cvRound(W / 1.2^l), scales 1.2^l and the per-level quotas n0 * f^l (last level: the remainder), all in the
    float arithmetic cv::ORB uses: scaleFactor is the float 1.2f, the powers are taken in double and stored as float."""
    sf = float(f32(1.2))
    scale = np.array([f32(sf ** l) for l in range(NLEVELS)], f32)
    w = np.array([int(np.rint(f32(W) * (f32(1) / s))) for s in scale], np.int32)
    h = np.array([int(np.rint(f32(H) * (f32(1) / s))) for s in scale], np.int32)
    factor = f32(1.0 / sf)
    nd = f32(max_kp) * (f32(1) - factor) / (f32(1) - f32(float(factor) ** NLEVELS))
    quota, total = [], 0
    for _ in range(NLEVELS - 1):
        quota.append(int(np.rint(nd)))
        total += quota[-1]
        nd = f32(nd * factor)
    quota.append(max(max_kp - total, 0))
    return w, h, scale, np.array(quota, np.int32)


# ---- pyramid -------------------------------------------------------------------------------------------------------------------
def _resize_taps(dn, sn):
    """Source index and the fractional position (float) of each of dn output samples over sn source samples (pixel centres
    aligned: (d + 0.5) * sn / dn - 0.5), clamped to the source as cv::resize does."""
    pos = ((np.arange(dn) + 0.5) * (float(sn) / dn) - 0.5).astype(f32)
    i0 = np.floor(pos).astype(np.int64)
    fr = (pos - i0.astype(f32)).astype(f32)
    lowc, highc = i0 < 0, i0 >= sn - 1
    fr = np.where(lowc | highc, f32(0), fr).astype(f32)
    i0 = np.where(lowc, 0, np.where(highc, sn - 1, i0))
    return i0, np.minimum(i0 + 1, sn - 1), fr


def resize_fixed(src, dw, dh):
    """cv::resize INTER_LINEAR on 8-bit: 11-bit coefficients cvRound(f * 2048), rows first:
    ((b0 * (S0 >> 4)) >> 16 + (b1 * (S1 >> 4)) >> 16 + 2) >> 2 with S = p0 * a0 + p1 * a1."""
    sh, sw = src.shape
    x0, x1, fx = _resize_taps(dw, sw)
    y0, y1, fy = _resize_taps(dh, sh)
    a0 = np.rint((f32(1) - fx) * f32(2048)).astype(np.int64); a1 = np.rint(fx * f32(2048)).astype(np.int64)
    b0 = np.rint((f32(1) - fy) * f32(2048)).astype(np.int64); b1 = np.rint(fy * f32(2048)).astype(np.int64)
    s = src.astype(np.int64)
    S0 = s[y0][:, x0] * a0 + s[y0][:, x1] * a1
    S1 = s[y1][:, x0] * a0 + s[y1][:, x1] * a1
    v = (((b0[:, None] * (S0 >> 4)) >> 16) + ((b1[:, None] * (S1 >> 4)) >> 16) + 2) >> 2
    return np.clip(v, 0, 255).astype(np.uint8)


def resize_exact(src, dw, dh):
    """Bilinear interpolation in float64 at the sample positions of resize_fixed (weights fx, 1 - fx as real numbers)."""
    sh, sw = src.shape
    x0, x1, fx = _resize_taps(dw, sw)
    y0, y1, fy = _resize_taps(dh, sh)
    fx = fx.astype(np.float64); fy = fy.astype(np.float64)[:, None]
    s = src.astype(np.float64)
    top = s[y0][:, x0] * (1 - fx) + s[y0][:, x1] * fx
    bot = s[y1][:, x0] * (1 - fx) + s[y1][:, x1] * fx
    return top * (1 - fy) + bot * fy


def resize_bound():
    """|resize_fixed - resize_exact| is at most this.  DERIVED, not measured:

    * coefficients: a = cvRound(f * 2048) is within e = 0.5 / 2048 of f; the float subtraction 1 - f adds at most 2^-25.  With
      e' = e + 2^-25, the four products of a y- and an x-weight differ from the exact ones by at most 2e' + e'^2 in sum per
      row pair and 4e' + 4e'^2 over the four taps (weights are non-negative and each pair sums to about 1): on pixels
      <= 255 that is 255 * (4e' + 4e'^2) = 0.2491.
    * S >> 4 drops less than 1 of S / 16; times b / 65536 <= 1/32 per row, 1/16 for both rows.
    * (b * (S >> 4)) >> 16 drops less than 1 per row, 2 for both.  The sum t of the two terms is therefore in
      (X - 2 - 1/16, X] with X the exact value of the coefficient form times 4.
    * (t + 2) >> 2 is t / 4 rounded half up on an integer t: it moves by -0.25 .. +0.5.
    So fixed - X / 4 lies in (-(2 + 1/16) / 4 - 0.25, +0.5] = (-0.765625, 0.5], and |fixed - exact| < 0.765625 + 0.2491 = 1.0147."""
    e = 0.5 / 2048 + 2.0 ** -25
    return (2 + 1 / 16) / 4 + 0.25 + 255 * (4 * e + 4 * e * e)


def build_pyramid(gray, rules=DEFAULT):
    """Level 0 is the image; level l is resize_fixed of level l - 1."""
    H, W = gray.shape
    w, h, _, _ = geometry(W, H)
    levels = [np.ascontiguousarray(gray, np.uint8)]
    for l in range(1, NLEVELS):
        levels.append(resize_fixed(levels[-1], int(w[l]), int(h[l])))
    return levels


# ---- FAST ----------------------------------------------------------------------------------------------------------------------
def _some_arc(c, ring, t, rules):
    """c: centres, ring: the 16 ring pixels of each (a list of arrays shaped like c), t: thresholds.  Spelled out: for every start
    s, do ring pixels s, s + 1, .. s + arc - 1 (mod 16) ALL exceed c + t, or ALL stay below c - t?"""
    if rules.contrast_strict:
        bright = [r > c + t for r in ring]; dark = [r < c - t for r in ring]
    else:
        bright = [r >= c + t for r in ring]; dark = [r <= c - t for r in ring]
    found = np.zeros(np.shape(c), bool)
    for passes in (bright, dark):
        for s in range(16):
            run = passes[s].copy()
            for k in range(1, rules.arc):
                run &= passes[(s + k) % 16]
            found |= run
    return found


def arc_test(img, xs, ys, t, rules=DEFAULT):
    """The definition, literally: is there a run of `arc` contiguous ring pixels that are all > c + t or all < c - t?
    xs, ys: pixel coordinates at least 3 away from every side; t: a scalar or one value per pixel.  Returns a bool per pixel."""
    xs = np.asarray(xs, np.int64); ys = np.asarray(ys, np.int64)
    im = img.astype(np.int16)
    ring = [im[ys + RING_Y[i], xs + RING_X[i]] for i in range(16)]
    return _some_arc(im[ys, xs], ring, np.asarray(t, np.int16), rules)


def fast_scores(img, rules=DEFAULT):
    """Score map of one level: S - 1 where S = (largest t for which the arc test holds) + 1 exceeds the threshold 20, else 0.
    The test can only turn from true to false as t grows, so the largest t is found by bisection - every probe is the literal
    test.  Pixels less than 3 from a side have no ring and score 0."""
    h, w = img.shape
    out = np.zeros((h, w), np.int32)
    if h < 7 or w < 7:
        return out
    im = img.astype(np.int16)
    ring = [im[3 + RING_Y[i]:h - 3 + RING_Y[i], 3 + RING_X[i]:w - 3 + RING_X[i]] for i in range(16)]
    ys, xs = np.nonzero(_some_arc(im[3:h - 3, 3:w - 3], ring, np.int16(FAST_THR), rules))       # the whole level at t = 20
    xs += 3; ys += 3
    lo = np.full(len(xs), FAST_THR, np.int64)          # holds at lo
    hi = np.full(len(xs), 256, np.int64)               # fails at hi (no difference of 8-bit pixels exceeds 255)
    while np.any(hi - lo > 1):
        mid = (lo + hi) // 2
        ok = arc_test(img, xs, ys, mid, rules)
        lo = np.where(ok, mid, lo); hi = np.where(ok, hi, mid)
    out[ys, xs] = lo                                   # S = lo + 1 > 20; score = S - 1
    return out


def fast_corners(img, rules=DEFAULT):
    """Corners of one level as rows {x, y, score} in raster order: strict 3 x 3 NMS on the score over the whole level, THEN the
    border filter (a stronger corner just outside the border still suppresses its neighbour inside)."""
    h, w = img.shape
    sc = fast_scores(img, rules)
    b = rules.border
    inside = np.zeros((h, w), bool)
    if h > 2 * b and w > 2 * b:
        inside[b:h - b, b:w - b] = True
    if rules.border_first:
        sc = np.where(inside, sc, 0)
    p = np.pad(sc, 1)
    keep = sc > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                nb = p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
                keep &= (nb < sc) if rules.nms_strict else (nb <= sc)
    keep &= inside
    ys, xs = np.nonzero(keep)
    return np.stack([xs, ys, sc[ys, xs]], 1).astype(np.int32).reshape(-1, 3)


def sort_corners(c):
    """Raster order of an unordered {x, y, score} list (the device's list is unordered)."""
    c = np.asarray(c, np.int32).reshape(-1, 3)
    return c[np.lexsort((c[:, 0], c[:, 1]))]


# ---- retainBest, Harris, the cut ---------------------------------------------------------------------------------------------
def retain_best(corners, quota, rules=DEFAULT):
    """Corners that go on to the Harris measure: everything scoring at least what the (2 * quota)-th best scores (ties kept);
    if more than CAP1 remain, the threshold goes up until they fit - which can leave nothing.  Returns (rows, threshold)."""
    corners = sort_corners(corners)
    n, target = len(corners), 2 * int(quota)
    score = corners[:, 2]
    T = 0
    if n > target and target > 0:
        order = np.lexsort((np.arange(n), -score))             # score descending, raster ascending
        if rules.keep_ties:
            T = int(score[order[target - 1]])
        else:
            return corners[np.sort(order[:target])], int(score[order[target - 1]])
    elif n > target:
        T = 256
    if rules.cap1:
        while int((score >= T).sum()) > CAP1:
            T += 1
    return corners[score >= T], T


def harris(img, xs, ys):
    """25 * (ab - c^2) - (a + b)^2 as Python integers; a = sum Ix^2, b = sum Iy^2, c = sum Ix Iy over the 7 x 7 block, Ix and Iy
    the 3 x 3 gradients with weights (1, 2, 1) across."""
    I = img.astype(np.int64)
    p = np.pad(I, 1)                                       # values outside are never used: blocks sit >= 27 px inside
    h, w = I.shape
    def sh(dy, dx):
        return p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    Ix = 2 * (sh(0, 1) - sh(0, -1)) + (sh(-1, 1) - sh(-1, -1)) + (sh(1, 1) - sh(1, -1))
    Iy = 2 * (sh(1, 0) - sh(-1, 0)) + (sh(1, -1) - sh(-1, -1)) + (sh(1, 1) - sh(-1, 1))
    xs = np.asarray(xs, np.int64); ys = np.asarray(ys, np.int64)
    o = np.arange(-3, 4)
    by = ys[:, None, None] + o[None, :, None]; bx = xs[:, None, None] + o[None, None, :]
    gx, gy = Ix[by, bx], Iy[by, bx]
    a = (gx * gx).sum(axis=(1, 2)); b = (gy * gy).sum(axis=(1, 2)); c = (gx * gy).sum(axis=(1, 2))
    return [25 * (int(ai) * int(bi) - int(ci) * int(ci)) - (int(ai) + int(bi)) ** 2 for ai, bi, ci in zip(a, b, c)]


def round_f32(q):
    """A rational rounded ONCE to the nearest float32 (ties to even), exactly."""
    q = Fraction(q)
    if q == 0:
        return f32(0)
    g = f32(float(q))                                     # within an ulp; the true nearest is g or a neighbour of g
    best = None
    for c in (np.nextafter(g, f32(-np.inf)), g, np.nextafter(g, f32(np.inf))):
        d = abs(Fraction(float(c)) - q)
        even = (int(np.asarray(c, f32).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even and not best[2]):
            best = (d, c, even)
    return f32(best[1])


RESPONSE_DEN = 25 * (4 * 7 * 255) ** 4


def response(R):
    """The Harris measure as OpenCV scales it: R * (1 / (4 * 7 * 255))^4 / 25, one rounding to float."""
    return round_f32(Fraction(int(R), RESPONSE_DEN))


def select(img, corners, quota, rules=DEFAULT):
    """One level's keypoints as rows (x, y, R): retainBest by FAST score, then (R descending, raster ascending), cut at quota."""
    cand, _ = retain_best(corners, quota, rules)
    if len(cand) == 0 or quota == 0:
        return []
    R = harris(img, cand[:, 0], cand[:, 1])
    rows = [(int(x), int(y), r) for (x, y, _), r in zip(cand, R)]
    if rules.tie_y_first:
        rows.sort(key=lambda v: (-v[2], v[1], v[0]))
    else:
        rows.sort(key=lambda v: (-v[2], v[0], v[1]))
    return rows[:int(quota) + rules.quota_extra]


# ---- orientation ---------------------------------------------------------------------------------------------------------------
def umax():
    """Half-widths of the radius-15 disc, row by row: round(sqrt(15^2 - v^2)) up to the row past the diagonal (v <= 11), the rest
    by reflecting that arc in the diagonal so that the disc is the same read by rows or by columns."""
    hp = HALF_PATCH
    vmax = int(np.floor(hp * np.sqrt(2.0) / 2 + 1))
    u = [0] * (hp + 1)
    for v in range(vmax + 1):
        u[v] = int(np.rint(np.sqrt(float(hp * hp - v * v))))
    for v in range(vmax + 1, hp + 1):
        u[v] = max(k for k in range(vmax + 1) if u[k] >= v)
    return u


def disc_mask(rules=DEFAULT):
    m = np.zeros((31, 31), bool)
    u = umax() if rules.use_umax else [HALF_PATCH] * 16
    for v in range(-15, 16):
        m[v + 15, 15 - u[abs(v)]:15 + u[abs(v)] + 1] = True
    return m


def moments(img, xs, ys, rules=DEFAULT):
    """(m10, m01) = sum of (u, v) * I over the disc around each point, in integers."""
    xs = np.asarray(xs, np.int64); ys = np.asarray(ys, np.int64)
    o = np.arange(-15, 16)
    win = img[ys[:, None, None] + o[None, :, None], xs[:, None, None] + o[None, None, :]].astype(np.int64)
    win = win * disc_mask(rules)[None]
    m10 = (win * o[None, None, :]).sum(axis=(1, 2))
    m01 = (win * o[None, :, None]).sum(axis=(1, 2))
    return m10, m01


def fast_atan2(y, x, rules=DEFAULT):
    """cv::fastAtan2 in degrees: a 7th-order odd polynomial in min / (max + eps), every operation rounded to float."""
    y = np.asarray(y, f32); x = np.asarray(x, f32)
    p1, p3, p5, p7 = f32(57.283627), f32(-18.667446), f32(8.9140005), f32(-2.5397246)
    eps = f32(2.220446e-16)
    ax, ay = np.abs(x), np.abs(y)
    first = (ax >= ay) if rules.atan_ge else (ax > ay)
    num = np.where(first, ay, ax).astype(f32); den = (np.where(first, ax, ay).astype(f32) + eps).astype(f32)
    c = (num / den).astype(f32)
    c2 = (c * c).astype(f32)
    a = (p7 * c2).astype(f32)
    a = (a + p5).astype(f32); a = (a * c2).astype(f32)
    a = (a + p3).astype(f32); a = (a * c2).astype(f32)
    a = (a + p1).astype(f32); a = (a * c).astype(f32)
    a = np.where(first, a, (f32(90) - a).astype(f32)).astype(f32)
    a = np.where(x < 0, (f32(180) - a).astype(f32), a).astype(f32)
    a = np.where(y < 0, (f32(360) - a).astype(f32), a).astype(f32)
    return a


def angles(img, xs, ys, rules=DEFAULT):
    m10, m01 = moments(img, xs, ys, rules)
    return fast_atan2(m01.astype(f32), m10.astype(f32), rules)


# ---- blur + descriptor ---------------------------------------------------------------------------------------------------------
GAUSS7 = np.array([18, 34, 49, 55, 49, 34, 18], np.int64)


def blur(img, rules=DEFAULT):
    """GaussianBlur 7 x 7, sigma 2, on 8-bit: separable 8-bit fixed-point kernel, BORDER_REFLECT_101, (sum + 2^15) >> 16,
    saturated - over the WHOLE level."""
    p = np.pad(img.astype(np.int64), 3, mode="reflect")
    h, w = img.shape
    hor = sum(GAUSS7[k] * p[:, k:k + w] for k in range(7))
    ver = sum(GAUSS7[k] * hor[k:k + h, :] for k in range(7))
    v = (ver + (1 << 15)) >> 16
    return (np.minimum(v, 255) if rules.blur_clamp else v & 255).astype(np.uint8)


def brief_pattern():
    """The 256 tests {x0, y0, x1, y1} of include/svo_brief_pattern.h."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svo_brief_pattern.h")
    rows = re.findall(r"\{\s*(-?\d+),\s*(-?\d+),\s*(-?\d+),\s*(-?\d+)\}", open(path).read())
    assert len(rows) == 256
    return np.array(rows, np.int64)


_PATTERN = None


def sincos_poly(angle_rad):
    """sin and cos of float angles by the fixed double polynomial (reduction by multiples of pi/2 in two parts, Taylor terms to
    r^15 / r^16 in Horner form), one rounding per operation; returned in double, the caller rounds to float."""
    x = np.asarray(angle_rad, f32).astype(np.float64)
    k = np.floor(x * 0.63661977236758134308 + 0.5)
    r = (x - k * 1.57079632679489655800e+00) - k * 6.12323399573676603587e-17
    r2 = r * r
    ps = np.full_like(r, -1.0 / 1307674368000.0)
    for d, sg in ((6227020800.0, 1), (39916800.0, -1), (362880.0, 1), (5040.0, -1), (120.0, 1), (6.0, -1)):
        ps = ps * r2 + sg * (1.0 / d)
    sr = r + r * (r2 * ps)
    pc = np.full_like(r, 1.0 / 20922789888000.0)
    for d, sg in ((87178291200.0, -1), (479001600.0, 1), (3628800.0, -1), (40320.0, 1), (720.0, -1), (24.0, 1)):
        pc = pc * r2 + sg * (1.0 / d)
    pc = pc * r2 - 0.5
    cr = 1.0 + r2 * pc
    q = k.astype(np.int64) & 3
    s = np.choose(q, [sr, cr, -sr, -cr])
    c = np.choose(q, [cr, -sr, -cr, sr])
    return s, c


def describe(blurred, xs, ys, angle_deg, rules=DEFAULT):
    """256 comparisons of blurred pixels at the pattern points rotated by the angle and rounded to the grid (cvRound); test
    8 * i + k is bit k of byte i.  Products and sums are float operations, never fused."""
    global _PATTERN
    if _PATTERN is None:
        _PATTERN = brief_pattern()
    xs = np.asarray(xs, np.int64); ys = np.asarray(ys, np.int64)
    ang = (np.asarray(angle_deg, f32) * f32(0.017453292)).astype(f32)
    s, c = sincos_poly(ang)
    a = c.astype(f32)[:, None]; b = s.astype(f32)[:, None]
    P = _PATTERN.astype(f32)

    def rot(px, py):
        rx = ((px[None, :] * a).astype(f32) - (py[None, :] * b).astype(f32)).astype(f32)
        ry = ((px[None, :] * b).astype(f32) + (py[None, :] * a).astype(f32)).astype(f32)
        if rules.half_even:
            return np.rint(rx).astype(np.int64), np.rint(ry).astype(np.int64)
        return np.floor(rx + f32(0.5)).astype(np.int64), np.floor(ry + f32(0.5)).astype(np.int64)

    x0, y0 = rot(P[:, 0], P[:, 1])
    x1, y1 = rot(P[:, 2], P[:, 3])
    v0 = blurred[ys[:, None] + y0, xs[:, None] + x0].astype(np.int64)
    v1 = blurred[ys[:, None] + y1, xs[:, None] + x1].astype(np.int64)
    bit = (v0 < v1) if rules.bit_strict else (v0 <= v1)
    return np.packbits(bit.reshape(len(xs), 32, 8), axis=2, bitorder="little").reshape(len(xs), 32)


# ---- the chain -----------------------------------------------------------------------------------------------------------------
def keypoints(levels, selected, scale, rules=DEFAULT):
    """Keypoint records and descriptors from the levels and the per-level selections (rows (x, y, R))."""
    kps, descs = [], []
    for l, rows in enumerate(selected):
        if not rows:
            continue
        img = levels[l]
        xs = np.array([r[0] for r in rows]); ys = np.array([r[1] for r in rows])
        ang = angles(img, xs, ys, rules)
        kp = np.zeros(len(rows), KP_DTYPE)
        kp["x"] = xs.astype(f32) * scale[l]; kp["y"] = ys.astype(f32) * scale[l]
        kp["size"] = f32(31.0) * scale[l]
        kp["angle"] = ang
        kp["response"] = [response(r[2]) for r in rows]
        kp["octave"] = l; kp["class_id"] = -1
        kps.append(kp)
        descs.append(describe(blur(img, rules), xs, ys, ang, rules))
    if not kps:
        return np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8)
    return np.concatenate(kps), np.concatenate(descs)


def extract(gray, max_kp=500, rules=DEFAULT):
    """The whole chain.  Returns a dict with every intermediate result: levels, corners (per level, raster order), selected
    (per level, rows (x, y, R) in Harris rank order), kp, desc."""
    H, W = gray.shape
    _, _, scale, quota = geometry(W, H, max_kp)
    levels = build_pyramid(gray, rules)
    corners = [fast_corners(lv, rules) for lv in levels]
    selected = [select(levels[l], corners[l], int(quota[l]), rules) for l in range(NLEVELS)]
    kp, desc = keypoints(levels, selected, scale, rules)
    return dict(levels=levels, corners=corners, selected=selected, kp=kp, desc=desc, quota=quota, scale=scale)
