"""ORB extraction without a GPU: the numpy twin (tests/orb_ref.py, written from the definitions) equals the oracle
(oracle/orc_orb.c, the closed forms) bit for bit on the hand-made cases of tests/orb_cases.py and on textured, noise and street
images; every case reaches the edge it was made for; every rule of the twin is pinned by a named case (flip the rule, the case
notices); and the twin itself is held to tests/golden/orb_restatement_pins.json.

`python tests/test_orb_cpu.py` rewrites the pins file from the twin (data only: counts, digests, measured figures)."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import orb_cases
import orb_ref
import util

PINS = os.path.join(util.GOLDEN, "orb_restatement_pins.json")


def _noise(seed, W, H):
    return np.random.default_rng(seed).integers(0, 256, size=(H, W), dtype=np.uint8)


IMAGES = {
    "blocky_96x96": lambda: util.blocky_image(21, 96, 96),
    "blocky_131x97": lambda: util.blocky_image(22, 131, 97),
    "blocky_352x330": lambda: util.blocky_image(23, 352, 330),
    "noise_96x96": lambda: _noise(31, 96, 96),
    "noise_131x97": lambda: _noise(32, 131, 97),
    "noise_352x330": lambda: _noise(33, 352, 330),
    "urban_640x240": lambda: util.urban_pair(640, 240, 300, 60)[0],
}


def assert_same_as_oracle(orc, img, max_kp, r):
    """Levels, corner sets and keypoints field by field as bit patterns, descriptors."""
    H, W = img.shape
    kp, desc, pyr = orc.orb_extract(img, max_kp, want_pyramid=True)
    levels = orc.pyramid_levels(pyr, W, H)
    for l in range(8):
        assert np.array_equal(levels[l], r["levels"][l]), ("level", l)
        assert np.array_equal(orc.fast_corners(levels[l]), r["corners"][l]), ("corners of level", l)
    assert len(kp) == len(r["kp"]), (len(kp), len(r["kp"]))
    for f in kp.dtype.names:
        assert np.array_equal(kp[f].view(np.uint32), r["kp"][f].view(np.uint32)), ("keypoint field", f)
    assert np.array_equal(desc, r["desc"])


@pytest.mark.parametrize("name", orb_cases.NAMES)
def test_twin_equals_oracle_on_case(orc, name):
    assert_same_as_oracle(orc, orb_cases.image(name), orb_cases.CASES[name]["max_kp"], orb_cases.reference(name))


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_twin_equals_oracle_on_image(orc, name):
    img = IMAGES[name]()
    r = orb_ref.extract(img)
    assert len(r["kp"]) > 30
    assert_same_as_oracle(orc, img, 500, r)


@pytest.mark.parametrize("name", orb_cases.NAMES)
def test_case_reaches_what_it_was_made_for(name):
    orb_cases.prove(name)


def _holds_literally(img, x, y, t):
    """FAST-9/16 at threshold t, spelled out: some 9 contiguous ring pixels are all > c + t or all < c - t."""
    c = int(img[y, x])
    ring = [int(img[y + dy, x + dx]) for dx, dy in zip(orb_ref.RING_X, orb_ref.RING_Y)]
    for s in range(16):
        arc = [ring[(s + k) % 16] for k in range(9)]
        if all(v > c + t for v in arc) or all(v < c - t for v in arc):
            return True
    return False


@pytest.mark.parametrize("name", orb_cases.NAMES)
def test_corner_scores_are_the_definition(name):
    """For the corners of every level of every case: the literal test holds at t = score and fails at t = score + 1."""
    r = orb_cases.reference(name)
    total = 0
    for l in range(8):
        c = r["corners"][l]
        if len(c) == 0:
            continue
        assert c[:, 2].min() >= orb_ref.FAST_THR
        assert orb_ref.arc_test(r["levels"][l], c[:, 0], c[:, 1], c[:, 2]).all()
        assert not orb_ref.arc_test(r["levels"][l], c[:, 0], c[:, 1], c[:, 2] + 1).any()
        for x, y, s in c[:: max(1, len(c) // 40)]:               # and in plain Python loops on a sample of them
            assert _holds_literally(r["levels"][l], x, y, s) and not _holds_literally(r["levels"][l], x, y, s + 1)
        total += len(c)
    assert total > 0


# ---- every rule is pinned by a case ---------------------------------------------------------------------------------------------
MUTANTS = [
    ("an arc of 8", dict(arc=8), "arc_lengths"),
    (">= in the contrast test", dict(contrast_strict=False), "ladder_bg100"),
    ("non-strict NMS", dict(nms_strict=False), "nms_pairs"),
    ("the border filter before NMS", dict(border_first=True), "border_w128"),
    ("a border of 30", dict(border=30), "border_w129"),
    ("a border of 32", dict(border=32), "border_w130"),
    ("ties dropped in retainBest", dict(keep_ties=False), "target_5_tied"),
    ("the CAP1 rule off", dict(cap1=False), "identical_1025"),
    ("the tie-break by x before y", dict(tie_y_first=False), "identical_64"),
    ("quota + 1", dict(quota_extra=1), "identical_65"),
    ("the moment mask without umax", dict(use_umax=False), "arc_lengths"),
    ("ax > ay", dict(atan_ge=False), "satellite_diagonal"),
    ("the blur without the clamp", dict(blur_clamp=False), "dark_dot_on_255"),
    ("round half-up", dict(half_even=False), "blocky_kp512"),
    ("t0 <= t1", dict(bit_strict=False), "lone_dot"),
]


def _digest(r):
    h = hashlib.sha256()
    for l in range(8):
        h.update(np.ascontiguousarray(r["corners"][l]).tobytes())
    h.update(r["kp"].tobytes()); h.update(np.ascontiguousarray(r["desc"]).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("what,flip,name", MUTANTS, ids=[m[0].replace(" ", "_") for m in MUTANTS])
def test_mutant_is_killed(what, flip, name):
    ref = orb_cases.reference(name)
    mut = orb_ref.extract(orb_cases.image(name), orb_cases.CASES[name]["max_kp"], orb_ref.Rules(**flip))
    assert _digest(mut) != _digest(ref), "%s: not noticed by %s" % (what, name)
    print("killed: %s by %s" % (what, name))


# ---- stages on their own ---------------------------------------------------------------------------------------------------------
def test_geometry_quotas_and_disc():
    assert orb_ref.geometry(352, 330, 8)[3].tolist() == [2, 1, 1, 1, 1, 1, 1, 0]
    assert orb_ref.geometry(352, 330, 9)[3].tolist() == [2, 2, 1, 1, 1, 1, 1, 0]
    assert orb_ref.geometry(352, 330, 512)[3].tolist() == [111, 93, 77, 64, 54, 45, 37, 31]
    assert tuple(orb_ref.umax()) == orb_ref.UMAX_TABLE
    m = orb_ref.disc_mask()
    assert np.array_equal(m, m.T) and np.array_equal(m, m[::-1]) and m.sum() == sum(2 * u + 1 for u in orb_ref.UMAX_TABLE) * 2 - 31


def test_geometry_equals_oracle(orc):
    for W, H, k in [(c["W"], c["H"], c["max_kp"]) for c in orb_cases.CASES.values()] + [(1241, 376, 500), (640, 240, 500)]:
        for a, b in zip(orb_ref.geometry(W, H, k), orc.geometry(W, H, k)):
            assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", ["noise_131x97", "blocky_352x330", "urban_640x240"])
def test_fixed_point_resize_is_within_its_derived_bound_of_exact_bilinear(name):
    img = IMAGES[name]()
    bound = orb_ref.resize_bound()
    assert 1.0 < bound < 1.02
    levels = orb_ref.build_pyramid(img)
    worst = 0.0
    for l in range(1, 8):
        h, w = levels[l].shape
        exact = orb_ref.resize_exact(levels[l - 1], w, h)
        worst = max(worst, float(np.abs(levels[l].astype(np.float64) - exact).max()))
    print(name, "worst |fixed - exact| = %.4f, bound %.4f" % (worst, bound))
    assert worst <= bound


def atan_sweep():
    """Worst |fastAtan2 - atan2| in degrees over every integer (m01, m10) with |m| <= 400 and the same grid scaled to the
    moments' range (x 997)."""
    v = np.arange(-400, 401)
    y, x = [a.ravel() for a in np.meshgrid(v, v, indexing="ij")]
    worst = 0.0
    for k in (1, 997):
        got = orb_ref.fast_atan2((y * k).astype(np.float32), (x * k).astype(np.float32)).astype(np.float64)
        want = np.degrees(np.arctan2(y.astype(np.float64), x.astype(np.float64))) % 360.0
        err = np.abs(got - want)
        err = np.minimum(err, 360.0 - err)
        worst = max(worst, float(err.max()))
    return worst


def sincos_sweep():
    """Number of float angles k * 0.001 degrees, k = 0 .. 360,000, at which the polynomial's sin / cos rounded to float differs
    from libm's rounded to float."""
    a = (np.arange(0, 360001).astype(np.float32) * np.float32(0.001)).astype(np.float32)
    rad = (a * np.float32(0.017453292)).astype(np.float32)
    s, c = orb_ref.sincos_poly(rad)
    ds = int((s.astype(np.float32) != np.sin(rad.astype(np.float64)).astype(np.float32)).sum())
    dc = int((c.astype(np.float32) != np.cos(rad.astype(np.float64)).astype(np.float32)).sum())
    return ds, dc


def test_fast_atan2_is_within_0p3_degrees_of_atan2():
    worst = atan_sweep()
    print("fastAtan2: worst error %.6f degrees" % worst)
    assert worst <= 0.3
    assert worst == json.load(open(PINS))["fast_atan2_worst_error_deg"]
    for y, x, want in ((0, 0, 0.0), (0, 5, 0.0), (5, 0, 90.0), (0, -5, 180.0), (-5, 0, 270.0)):
        assert float(orb_ref.fast_atan2(np.float32(y), np.float32(x))) == want


def test_sincos_polynomial_against_libm():
    ds, dc = sincos_sweep()
    print("sin differs at %d, cos at %d of 360,001 angles" % (ds, dc))
    pins = json.load(open(PINS))
    assert [ds, dc] == pins["sincos_float_differences_of_360001"]
    a = np.float32(np.arange(0, 360001) * 0.001)
    s, c = orb_ref.sincos_poly((a * np.float32(0.017453292)).astype(np.float32))
    rad = (a * np.float32(0.017453292)).astype(np.float32).astype(np.float64)
    assert np.abs(s - np.sin(rad)).max() < 1e-15 and np.abs(c - np.cos(rad)).max() < 1e-15    # in double it is libm's to an ulp or two


def test_blur_of_the_patch_equals_blur_of_the_level():
    """The device blurs a 31 x 31 patch from the 37 x 37 real pixels around a keypoint; the twin blurs the whole level with
    REFLECT_101.  Both are the same because a keypoint is at least 31 pixels inside: the outermost blurred pixel a descriptor
    reads is 15 away from it and its taps 18, and 18 < 31 - so no reflected pixel is ever used."""
    img = IMAGES["noise_131x97"]()
    whole = orb_ref.blur(img)
    for x, y in ((31, 31), (131 - 32, 97 - 32), (31, 97 - 32), (131 - 32, 31)):
        win = img[y - 18:y + 19, x - 18:x + 19]
        assert np.array_equal(orb_ref.blur(win)[3:-3, 3:-3], whole[y - 15:y + 16, x - 15:x + 16])


def test_response_is_rounded_once():
    from fractions import Fraction
    assert orb_ref.round_f32(Fraction(1, 3)) == np.float32(1 / 3)
    # 1 + 2^-24 + 2^-60 is above the tie between 1 and 1 + 2^-23: one rounding goes up, two (via double) stay at 1
    q = 1 + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 60)
    assert orb_ref.round_f32(q) == np.nextafter(np.float32(1), np.float32(2)) and np.float32(float(q)) == np.float32(1)
    assert orb_ref.round_f32(1 + Fraction(1, 2 ** 24)) == np.float32(1)          # the tie goes to even
    assert orb_ref.round_f32(-q) == -orb_ref.round_f32(q) and orb_ref.round_f32(0) == 0


# ---- the twin is held to its pins -------------------------------------------------------------------------------------------------
def case_pin(name):
    r = orb_cases.reference(name)
    return dict(corners_per_level=[int(len(c)) for c in r["corners"]],
                keypoints_per_level=np.bincount(r["kp"]["octave"], minlength=8).tolist(),
                keypoints_sha256=hashlib.sha256(r["kp"].tobytes()).hexdigest(),
                descriptors_sha256=hashlib.sha256(np.ascontiguousarray(r["desc"]).tobytes()).hexdigest())


@pytest.mark.parametrize("name", orb_cases.NAMES)
def test_twin_is_what_the_pins_say(name):
    pins = json.load(open(PINS))
    assert sorted(pins["cases"]) == sorted(orb_cases.NAMES)
    assert case_pin(name) == pins["cases"][name]


def make_pins():
    ds, dc = sincos_sweep()
    return dict(fast_atan2_worst_error_deg=atan_sweep(), sincos_float_differences_of_360001=[ds, dc],
                cases={n: case_pin(n) for n in orb_cases.NAMES})


if __name__ == "__main__":
    with open(PINS, "w") as f:
        json.dump(make_pins(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", PINS)
