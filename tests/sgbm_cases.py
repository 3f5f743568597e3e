"""Inputs of the semi-global block matcher's suites and a census of what they exercise.

The stage cases (pairs the device is compared on, stage by stage, with the numpy restatement tests/sgbm_ref.py), the maps of
the speckle-filter tests, and census(): counts, read off the restatement alone, of how often each written rule of the winner
stage actually decides something on a case.  tests/test_sgbm_cpu.py asserts that every rule is live somewhere in the union of
the stage cases, so that the device tests cannot pass without having met it."""
import numpy as np

import sgbm_ref
import util

INVALID = sgbm_ref.INVALID


# ---- input recipes -----------------------------------------------------------------------------------------------------------
def noise_pair(seed, W, H):
    rng = np.random.default_rng(seed)
    L = rng.integers(0, 256, (H, W), dtype=np.uint8)
    R = np.roll(L, -5, axis=1)
    R[::3] = rng.integers(0, 256, R[::3].shape, dtype=np.uint8)     # two rows in three carry a true match, the others none
    return L, R


def saturating_pair(W=120, H=30):
    """No iid-noise pair of seeds 0..63 at 120 x 30 saturates S4 (the largest four-direction sum seen there is about 21 000;
    checked with the restatement), and two constant images with an offset cannot either: their gradient planes are equal, so the
    pixel cost stops at 255 >> 2 and C at 81 * 63 = 5103.  C > 8191 needs the gradient term: saw-tooth ramps of opposite slope
    (prefiltered gradients 0 against 126 nearly everywhere) under a little noise."""
    x = np.arange(W)
    rng = np.random.default_rng(7)
    L = np.tile(255 - 10 * (x % 24), (H, 1)) - rng.integers(0, 8, (H, W))
    R = np.tile(10 * (x % 24), (H, 1)) + rng.integers(0, 8, (H, W))
    return np.clip(L, 0, 255).astype(np.uint8), np.clip(R, 0, 255).astype(np.uint8)


def binary_pair(seed, W, H, lo=0, hi=255):
    """A two-level left image and an independent two-level right image.  Nothing matches, every cost is one of a few small
    integers, so equal S values - and with them equal bids for a right-image column - are common, and the winner is as often
    at an end of the disparity range as anywhere else."""
    rng = np.random.default_rng(seed)
    L = np.where(rng.integers(0, 2, (H, W)) == 1, hi, lo).astype(np.uint8)
    R = np.where(rng.integers(0, 2, (H, W)) == 1, hi, lo).astype(np.uint8)
    return L, R


def bars_pair(seed, W, H, lo=0, hi=255):
    """binary_pair's rows all equal: two-level vertical bars, left and right independent.  The rows then differ only through the
    paths that come from above, so a tie in one row tends to recur in the next: such pairs carry ten times the tied bids."""
    rng = np.random.default_rng(seed)
    L = np.tile(np.where(rng.integers(0, 2, W) == 1, hi, lo), (H, 1)).astype(np.uint8)
    R = np.tile(np.where(rng.integers(0, 2, W) == 1, hi, lo), (H, 1)).astype(np.uint8)
    return L, R


OLD_CASES = ("noise83x37", "urban200x26", "rows1241x12", "saturated120x30", "noise150x20d64", "noise120x30d32")
PORTRAIT_CASES = ("portrait41x90d16", "portrait57x75d32", "tall30x300d16", "portrait75x100d48")
EXTREME_CASES = ("wide3072x2d16",)
MINIMAL_CASES = ("minimal25x2d16", "minimal73x2d64")     # W = D + 9, H = 2: the smallest sizes the argument check admits
TIE_CASES = ("binary64x8s5348", "bars64x8s29", "bars64x8s70")
NEW_CASES = PORTRAIT_CASES + EXTREME_CASES + MINIMAL_CASES + TIE_CASES
STAGE_CASES = OLD_CASES + NEW_CASES

# name -> (seed, W, H, D) of the iid-noise recipe
_NOISE = {
    "noise83x37": (1, 83, 37, 16),            # odd width and height, every border rule live
    "noise150x20d64": (4, 150, 20, 64),       # the widest disparity range, all 64 lanes of a group in use
    "noise120x30d32": (2, 120, 30, 32),
    # H > W - D: max(H, W - D) = H sizes the launch of directions 0 / 2, so whole lane groups hold a direction-0 path and no
    # direction-2 path; diagonals that enter from a side column end at the other side column, not at the last row
    "portrait41x90d16": (3, 41, 90, 16),
    "portrait57x75d32": (3, 57, 75, 32),
    "tall30x300d16": (3, 30, 300, 16),        # H = 21 (W - D)
    "portrait75x100d48": (3, 75, 100, 48),     # the 64-lane group with 16 idle lanes and the 240-thread row block
    "wide3072x2d16": (3, 3072, 2, 16),        # the widest image: 61 440 bytes of dynamic LDS per row block
    "minimal25x2d16": (3, 25, 2, 16),
    "minimal73x2d64": (3, 73, 2, 64),
}
# name -> (recipe, seed, W, H, D): two-level pairs found by a seeded search with the restatement for tied right-image bids and
# winners at d = D - 1, which iid noise and real texture do not produce.  binary_pair, seeds 0 .. 9999 at 64 x 8, D = 16: 87
# seeds with a tied column (88 columns in all, never more than 2 in a pair; seed 5348 has 2), 6886 with a winner at D - 1.
# bars_pair, seeds 0 .. 999: 142 seeds with a tied column, 485 columns, up to 13 in a pair (seeds 29 and 70).
_TWO_LEVEL = {
    "binary64x8s5348": (binary_pair, 5348, 64, 8, 16),
    "bars64x8s29": (bars_pair, 29, 64, 8, 16),
    "bars64x8s70": (bars_pair, 70, 64, 8, 16),
}


def case(name):
    """(L, R, D) of a stage case."""
    if name in _NOISE:
        seed, W, H, D = _NOISE[name]
        return noise_pair(seed, W, H) + (D,)
    if name in _TWO_LEVEL:
        recipe, seed, W, H, D = _TWO_LEVEL[name]
        return recipe(seed, W, H) + (D,)
    if name == "urban200x26":         # real texture
        return util.urban_pair(200, 26, 400, 80) + (48,)
    if name == "rows1241x12":         # full-width rows, diagonals that enter from both side columns
        return util.shifted_pair(9, 1241, 12, disparity=17) + (48,)
    if name == "saturated120x30":
        return saturating_pair() + (16,)
    raise KeyError(name)


_refs = {}


def ref(name):
    """(L, R, D, restatement) of a stage case, computed once per session and never modified."""
    if name not in _refs:
        L, R, D = case(name)
        _refs[name] = (L, R, D, sgbm_ref.sgbm(L, R, D))
    return _refs[name]


# ---- the census --------------------------------------------------------------------------------------------------------------
CENSUS_KEYS = ("bid_ties", "best_first", "best_last", "negative_numerator_with_remainder", "uniqueness_rejections",
               "left_right_invalidated", "sum4_saturated", "sum5_saturated")


def _replay(out):
    """The winner loop of the restatement again, from out["S"], on whole arrays: per pixel x >= D the winning disparity, its
    S, whether the uniqueness test rejects it, and the subpixel terms before the clamp."""
    D = int(out["D"])
    S = out["S"][:, D:].astype(np.int64)                     # H x (W - D) x D
    best = S.argmin(axis=2)                                  # the first minimum over d ascending
    minS = np.take_along_axis(S, best[:, :, None], 2)[:, :, 0]
    dd = np.arange(D)
    far = np.abs(dd[None, None, :] - best[:, :, None]) > 1
    rejected = (far & (S * (100 - sgbm_ref.UNIQ) < minS[:, :, None] * 100)).any(axis=2)
    inner = ~rejected & (best > 0) & (best < D - 1)
    sm = np.take_along_axis(S, np.maximum(best - 1, 0)[:, :, None], 2)[:, :, 0]
    sp = np.take_along_axis(S, np.minimum(best + 1, D - 1)[:, :, None], 2)[:, :, 0]
    den_raw = sm + sp - 2 * minS
    den = np.maximum(den_raw, 1)
    num = (sm - sp) * 16 + den
    q = np.abs(num) // (2 * den)
    disp1 = np.where(rejected, INVALID, best * 16 + np.where(inner, np.where(num >= 0, q, -q), 0))
    return dict(D=D, best=best, minS=minS, rejected=rejected, inner=inner, den_raw=den_raw, den=den, num=num, disp1=disp1)


def census(out):
    """How often each written rule of the winner stage decides something, from the dict sgbm_ref.sgbm returned and nothing else:

      bid_ties                            right-image columns whose lowest minS was bid by two or more left pixels (the bid of
                                          the largest x must win: the restatement meets it first and replaces only on `>`)
      best_first, best_last               accepted winners at d = 0 and at d = D - 1 (no subpixel term on that side)
      negative_numerator_with_remainder   accepted inner winners whose subpixel numerator is negative and no multiple of
                                          2 den: C's truncating division and floor division give different answers
      uniqueness_rejections               pixels the uniqueness test rejects
      left_right_invalidated              pixels the left-right check takes away
      sum4_saturated, sum5_saturated      entries where L0 + .. + L3 > 32767, and where S4 + L4 leaves the int16 range

    Two further guards of the contract are not counted, because no input can reach them (impossible() counts them; both are 0
    on every stage case and were 0 on all 10 000 candidates of the search that found the tie cases):
      - the clamp max(S[best-1] + S[best+1] - 2 minS, 1): best is the FIRST minimum, so S[best-1] > minS strictly and
        S[best+1] >= minS, hence the denominator is at least 1 before the clamp;
      - the left-right probe's x - a < 0: a valid disp1 exists for x >= D only, and a <= D - 1, because the subpixel term is
        at most 8 sixteenths (|S[best-1] - S[best+1]| <= den, so |numerator| <= 17 den) and is added below best = D - 1 only."""
    r = _replay(out)
    D = r["D"]
    raw = out["disp1_raw"].astype(np.int64)
    assert np.array_equal(r["disp1"], raw[:, D:]) and np.all(raw[:, :D] == INVALID), "the replay is not the restatement's winner loop"
    H, nx = r["best"].shape
    W = nx + D
    ok = ~r["rejected"]
    ties = 0
    xs = np.arange(D, W)
    for y in range(H):
        x2 = (xs - r["best"][y])[ok[y]]
        ms = r["minS"][y][ok[y]]
        lowest = np.full(W, 1 << 30, np.int64)
        np.minimum.at(lowest, x2, ms)
        ties += int((np.bincount(x2[ms == lowest[x2]], minlength=W) >= 2).sum())
    sum5 = out["sum5"][:, D:]
    return dict(
        bid_ties=ties,
        best_first=int((ok & (r["best"] == 0)).sum()),
        best_last=int((ok & (r["best"] == D - 1)).sum()),
        negative_numerator_with_remainder=int((r["inner"] & (r["num"] < 0) & (r["num"] % (2 * r["den"]) != 0)).sum()),
        uniqueness_rejections=int(r["rejected"].sum()),
        left_right_invalidated=int(((raw != INVALID) & (out["disp1_lr"] == INVALID)).sum()),
        sum4_saturated=int((out["sum4"][:, D:] > 32767).sum()),
        sum5_saturated=int(((sum5 > 32767) | (sum5 < -32768)).sum()))


def impossible(out):
    """The two guards census() explains away: inner winners with a denominator <= 0 before the clamp, and left-right probes
    with x - a < 0."""
    r = _replay(out)
    D = r["D"]
    raw = out["disp1_raw"].astype(np.int64)
    x = np.arange(raw.shape[1])[None, :]
    valid = raw != INVALID
    probes = sum(int((valid & (x - a < 0)).sum()) for a in (raw >> 4, (raw + 15) >> 4))
    return dict(denominator_clamped=int((r["inner"] & (r["den_raw"] <= 0)).sum()), probe_left_of_image=probes)


def valid_fractions(out):
    """(before the speckle filter, final) fractions of valid pixels."""
    return float((out["disp1_lr"] != INVALID).mean()), float((out["disp16"] != INVALID).mean())


# ---- maps for the speckle filter ---------------------------------------------------------------------------------------------
def serpentine(W=600, H=64):
    """Every even row valid (values 160 + 16 (r mod 7), so rows two apart differ by at most 96), odd rows valid only at the
    end column that alternates right, left, right ..: one component of 32 * 600 + 32 = 19 232 pixels that winds through every
    256-column block of every row.  Consecutive pixels along it differ by at most 16 * 6 <= 512."""
    d = np.full((H, W), INVALID, np.int16)
    for r in range(H):
        v = 160 + 16 * (r % 7)
        if r % 2 == 0:
            d[r] = v
        else:
            d[r, W - 1 if (r // 2) % 2 == 0 else 0] = v
    return d


def comb(W=600, H=110):
    """Vertical bars one pixel wide on an invalid ground, 100 and 101 pixels long, in adjacent-but-one columns on both sides of
    x = 255 | 256 and x = 511 | 512, plus horizontal bars of 100 and 101 pixels that straddle those block boundaries.
    Returns (map, bars that must vanish, bars that must stay) as lists of (slice y, slice x)."""
    d = np.full((H, W), INVALID, np.int16)
    go, stay = [], []
    for x, n in ((253, 100), (255, 101), (256 + 1, 100), (256 + 3, 101), (509, 101), (511, 100), (512 + 1, 101), (512 + 3, 100)):
        s = (slice(2, 2 + n), slice(x, x + 1))
        d[s] = 800 + x
        (go if n == 100 else stay).append(s)
    for y, x0, n in ((104, 206, 100), (106, 206, 101), (104, 462, 101), (106, 462, 100)):
        s = (slice(y, y + 1), slice(x0, x0 + n))
        d[s] = 3000 + y
        (go if n == 100 else stay).append(s)
    return d, go, stay


def seeded_speckle_map(seed=11, W=333, H=129):
    """Multiples of 171 from 0 to 7 * 171 = 1197: neighbours differ by 0, 171, 342 or 513 .. 1197, so 513 = 3 * 171 lands one
    past the joining distance 512 and 342 well inside it.  10 % of the pixels are invalid."""
    rng = np.random.default_rng(seed)
    d = (171 * rng.integers(0, 8, (H, W))).astype(np.int16)
    # smooth it along the rows so that components of every size around 100 exist, not only dust
    run = rng.integers(0, 4, (H, W)) > 0
    for x in range(1, W):
        d[:, x] = np.where(run[:, x], d[:, x - 1], d[:, x])
    d[rng.random((H, W)) < 0.10] = INVALID
    return d
