"""Inputs of the colour (cn = 3) semi-global block matcher's suites: seeded constructors of 8UC3 pairs, the restatement
tests/sgbm_bgr_ref.py of each computed once per session, and a census, read off the restatement alone, of how often the two
rules that only exist with three channels - the block sum kept in a short, the carried step kept in a short - decide
something on a case."""
import numpy as np

import sgbm_bgr_ref


def noise_pair(seed, W, H):
    """sgbm_cases.noise_pair's recipe with independent noise in the three channels: two rows in three carry a true match."""
    rng = np.random.default_rng(seed)
    L = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    R = np.roll(L, -5, axis=1)
    R[::3] = rng.integers(0, 256, R[::3].shape, dtype=np.uint8)
    return L, R


def shifted_pair(seed=21, W=96, H=40, bands=(4, 9, 15), noise=(2, 6, 12)):
    """A noise texture; the right image is the left shifted by a disparity per band of rows (left x matches right x - d), plus
    uniform noise of another amplitude in every channel: the winners are real and the channels disagree about the cost."""
    rng = np.random.default_rng(seed)
    pad = max(bands)
    base = rng.integers(0, 256, (H, W + pad, 3)).astype(np.int64)
    L = base[:, :W]
    R = np.empty_like(L)
    edges = np.linspace(0, H, len(bands) + 1).astype(int)
    for d, y0, y1 in zip(bands, edges[:-1], edges[1:]):
        R[y0:y1] = base[y0:y1, d:d + W]
    for c, a in enumerate(noise):
        R[:, :, c] += rng.integers(-a, a + 1, (H, W))
    return L.astype(np.uint8), np.clip(R, 0, 255).astype(np.uint8)


def wrap_pair(W=80, H=12):
    """Rows are the sawtooth L(x) = (8 x) mod 256 and R(x) = 255 - L(x), the same in every row and channel: prefiltered
    gradients of opposite sign nearly everywhere, so three times the gray block sum peaks at 39 852 and exceeds 32 767 on
    27 % of the volume (the gray restatement says so: tests/test_sgbm_bgr_cpu.py)."""
    row = (8 * np.arange(W)) % 256
    L = np.tile(row[None, :, None], (H, 1, 3))
    return L.astype(np.uint8), (255 - L).astype(np.uint8)


def gray_pair(seed=33, W=64, H=20, disparity=6, lo=122, hi=134, noise=2, offset=36):
    """A gray pair with a true match whose sums, times three, stay inside int16 (the replicated-gray tests assert it from the
    gray restatement).  That needs moderate costs everywhere: low contrast keeps the block cost of a wrong disparity below
    2000, and a brightness offset in the right image keeps the cost of the right one above 600 - a perfect match costs
    nothing, its step is then -P2 in every direction, and 3 * 5 * 2592 is already past 32 767."""
    rng = np.random.default_rng(seed)
    base = rng.integers(lo, hi, (H, W + disparity)).astype(np.int64)
    L = base[:, :W]
    R = base[:, disparity:] + rng.integers(-noise, noise + 1, (H, W)) + offset
    return L.astype(np.uint8), np.clip(R, 0, 255).astype(np.uint8)


def replicate(g):
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, 2))


WRAP_CASE = "wrap80x12d16"
GRAY_CASE = "replicated64x20d16"
# name -> (constructor, arguments, D)
_CASES = {
    "minimal25x2d16": (noise_pair, (3, 25, 2), 16),            # W = D + 9, H = 2: the smallest sizes the argument check admits
    "shifted96x40d32": (shifted_pair, (), 32),
    WRAP_CASE: (wrap_pair, (), 16),
    "noise120x24d48": (noise_pair, (5, 120, 24), 48),          # the lane groups of 64, with 16 idle lanes and with none
    "noise120x24d64": (noise_pair, (5, 120, 24), 64),
    "portrait28x60d16": (noise_pair, (6, 28, 60), 16),         # H > W - D
    GRAY_CASE: (lambda: tuple(replicate(g) for g in gray_pair()), (), 16),
}
CASES = tuple(_CASES)


def case(name):
    """(L, R, D) of a case; L and R are H x W x 3 uint8."""
    make, args, D = _CASES[name]
    return make(*args) + (D,)


_refs = {}


def ref(name):
    """(L, R, D, restatement) of a case, computed once per session and never modified."""
    if name not in _refs:
        L, R, D = case(name)
        _refs[name] = (L, R, D, sgbm_bgr_ref.sgbm(L, R, D))
    return _refs[name]


def census(out):
    """From the dict sgbm_bgr_ref.sgbm returned and nothing else: block_sum_over = entries whose true block sum exceeds
    32 767 (C is then negative: the low 16 bits), carried_out = steps v of any direction that leave int16 (the successor then
    sees their low 16 bits), and the gray census's saturation counts."""
    D = int(out["D"])
    sum5 = out["sum5"][:, D:]
    return dict(block_sum_over=int((out["Ctrue"][:, D:] > 32767).sum()), carried_out=int(out["carried_out"]),
                sum4_saturated=int(((out["sum4"][:, D:] > 32767) | (out["sum4"][:, D:] < -32768)).sum()),
                sum5_saturated=int(((sum5 > 32767) | (sum5 < -32768)).sum()))


STAGE_KEYS = ("Ctrue", "C", "sum4", "S4", "sum5", "S", "disp2", "disp1_raw", "disp1_lr", "disp16", "disp")


def stage_hashes(out):
    """sha256 of every stage of a restatement (little-endian bytes of the arrays as sgbm_bgr_ref.sgbm types them): what
    tests/golden/sgbm_bgr_restatement_pins.json holds, so that the restatement cannot drift together with the kernels."""
    import hashlib
    return {k: hashlib.sha256(np.ascontiguousarray(out[k]).astype(out[k].dtype.newbyteorder("<")).tobytes()).hexdigest() for k in STAGE_KEYS}


if __name__ == "__main__":      # prints the pins file
    import json
    print(json.dumps({name: stage_hashes(ref(name)[3]) for name in CASES}, indent=1, sort_keys=True))
