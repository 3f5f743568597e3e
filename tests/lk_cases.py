"""Inputs of the Lucas-Kanade tests (tests/test_lk_cpu.py, tests/test_lk_gpu.py): smooth textures with planted translations,
and the pairs and points that drive the restatement (tests/lk_ref.py) through each of its exits.  The seeds and positions of
the oscillation and the 30-iteration cases were found by running the restatement on the CPU over candidate points."""
import numpy as np

# planted translations (dx, dy) in pixels: sub-pixel, mixed, multi-pixel
SHIFTS = ((0.3, -0.2), (-0.75, 0.5), (1.5, 2.25), (-3.2, 1.7), (5.0, -4.0), (8.4, 3.3), (11.5, 6.25))


def _binomial9(a, axis):
    k = np.array([1, 8, 28, 56, 70, 56, 28, 8, 1], np.float64) / 256.0
    return np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), axis, a)


def smooth_canvas(seed, W, H, margin=24):
    """Seeded noise blurred with the 9-tap binomial, stretched to 8 bits' range; float64, `margin` pixels larger on every side."""
    rng = np.random.default_rng(seed)
    a = rng.random((H + 2 * margin, W + 2 * margin))
    a = _binomial9(_binomial9(a, 0), 1)
    a = (a - a.min()) / (a.max() - a.min())
    return a * 255.0


def resample(canvas, W, H, dx, dy, margin=24):
    """The W x H view of the canvas moved by (dx, dy): out(x, y) = canvas(x - dx, y - dy), bilinear, rounded to uint8."""
    xs = np.arange(W) + margin - dx
    ys = np.arange(H) + margin - dy
    x0 = np.floor(xs).astype(int); y0 = np.floor(ys).astype(int)
    fx = (xs - x0)[None, :]; fy = (ys - y0)[:, None]
    c = canvas
    v = (c[np.ix_(y0, x0)] * (1 - fx) * (1 - fy) + c[np.ix_(y0, x0 + 1)] * fx * (1 - fy) +
         c[np.ix_(y0 + 1, x0)] * (1 - fx) * fy + c[np.ix_(y0 + 1, x0 + 1)] * fx * fy)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def planted_pair(seed, W, H, shift):
    """(prev, next): next is prev's texture moved by `shift`, so a point p of prev is at p + shift in next."""
    c = smooth_canvas(seed, W, H)
    return resample(c, W, H, 0.0, 0.0), resample(c, W, H, shift[0], shift[1])


def inner_grid(W, H, border=40, step=17):
    """Points at least `border` pixels from every edge, on a grid with fractional offsets that vary from point to point."""
    xs = np.arange(border, W - border, step); ys = np.arange(border, H - border, step)
    g = np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2).astype(np.float32)
    frac = (np.arange(len(g))[:, None] * np.array([0.37, 0.61])) % 1.0
    g = np.minimum(g + frac.astype(np.float32), np.float32([W - border, H - border]))
    return g.astype(np.float32)


def noise(seed, W, H):
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


# ---- the exits ------------------------------------------------------------------------------------------------------------------
OUTSIDE_POINT = (-30.0, 5.0)       # floor(x - 10) = -40 < -21 at level 0: range, status 0, err 0
FLAT_POINT = (90.0, 80.0)          # the middle of the constant patch: a zero normal matrix, minEig, status 0
DRIFT_POINT = (182.0, 66.0)        # 3 px from the right edge; follows the texture: floor(x - 10) >= cols after 3 iterations at level 0
EXITS_SIZE = (185, 177)


def exits_pair():
    """185 x 177: a smooth texture moved 12 px to the right, with a constant 60 x 60 patch at (60, 50) in both images and a
    50 x 50 block at (10, 120) that holds unrelated noise in the two images (the iterations wander there)."""
    W, H = EXITS_SIZE
    p, n = planted_pair(11, W, H, (12.0, 0.0))
    p = p.copy(); n = n.copy()
    p[50:110, 60:120] = 90; n[50:110, 60:120] = 90
    p[120:170, 10:60] = noise(100, 50, 50); n[120:170, 10:60] = noise(101, 50, 50)
    return p, n


def exits_points(n=300):
    """The three special points, 40 with integer coordinates (a = b = 0), 40 with x or y at .5 exactly (cvRound's ties), the
    rest uniform over the image and 25 px beyond it."""
    W, H = EXITS_SIZE
    rng = np.random.default_rng(5)
    special = np.array([OUTSIDE_POINT, FLAT_POINT, DRIFT_POINT])
    whole = rng.integers((0, 0), (W, H), (40, 2)).astype(np.float64)
    half = rng.integers((0, 0), (W, H), (40, 2)) + np.array([(0.5, 0.0), (0.0, 0.5), (0.5, 0.5), (0.5, 0.25)] * 10)
    rest = rng.uniform((-25, -25), (W + 15, H + 18), (n - 83, 2))
    return np.concatenate([special, whole, half, rest]).astype(np.float32)


def low_contrast_pair():
    """120 x 100, 16 gray levels of smooth texture moved by (0.4, 0.3): the quantised patch difference makes some points'
    steps alternate in sign."""
    c = smooth_canvas(30, 120, 100) * (16.0 / 255.0) + 100
    return resample(c, 120, 100, 0.0, 0.0), resample(c, 120, 100, 0.4, 0.3)


OSCILLATION_POINT = (82.0, 38.0)   # in low_contrast_pair(): ends by the oscillation rule at level 0 after 3 iterations


def wander_pair():
    """Two unrelated 40 x 40 noise images: one level, no correspondence."""
    return noise(100, 40, 40), noise(101, 40, 40)


MAX_COUNT_POINT = (8.0, 8.0)       # in wander_pair(): all 30 iterations at level 0, status stays 1
EPSILON_POINT = (100.0, 90.0)      # in planted_pair(11, 200, 180, SHIFTS[2]): converges by the epsilon rule at levels 1 and 0


def edge_points(W, H, n_inner=24, seed=3):
    """Points in the first and last 21 columns and rows, a few outside, and some inside."""
    rng = np.random.default_rng(seed)
    left = rng.uniform((0, 0), (21, H), (12, 2)); right = rng.uniform((W - 21, 0), (W, H), (12, 2))
    top = rng.uniform((0, 0), (W, 8), (6, 2)); bottom = rng.uniform((0, H - 8), (W, H), (6, 2))
    out = np.array([(-12.5, H / 2), (W + 9.0, H / 2), (W / 2, -11.0), (W / 2, H + 10.5), (0.0, 0.0), (W - 1.0, H - 1.0)])
    inner = rng.uniform((21, 0), (W - 21, H), (n_inner, 2))
    return np.concatenate([left, right, top, bottom, out, inner]).astype(np.float32)
