"""CPU suite of the Lucas-Kanade restatement (tests/lk_ref.py) alone: the pyramid, the level rule, planted translations, and
every exit of the per-level loop.

pyrDown worked by hand on the 6 x 6 image I(y, x) = 16 x + y.  The kernel is separable and sums to 16 per axis, so the 5 x 5
sum is 16 H(x) + 16 V(y) with H over a row and V over a column, both read reflect-101:
  H(0): columns -2..2 -> 2 1 0 1 2 -> 32 16 0 16 32 -> 32 + 64 + 0 + 64 + 32    = 192
  H(1): columns  0..4                -> 0 16 32 48 64 -> 0 + 64 + 192 + 192 + 64   = 512
  H(2): columns  2..6 -> 2 3 4 5 4 -> 32 48 64 80 64 -> 32 + 192 + 384 + 320 + 64 = 992
  V(0): rows 2 1 0 1 2 -> 2 + 4 + 0 + 4 + 2 = 12;  V(1): rows 0..4 -> 0 + 4 + 12 + 12 + 4 = 32;  V(2): rows 2 3 4 5 4 -> 62
  out(y, x) = (16 H(x) + 16 V(y) + 128) >> 8:
    y = 0: (3072 + 192 + 128, 8192 + 192 + 128, 15872 + 192 + 128) >> 8 = 13 33 63
    y = 1: (3072 + 512 + 128, 8192 + 512 + 128, 15872 + 512 + 128) >> 8 = 14 34 64
    y = 2: (3072 + 992 + 128, 8192 + 992 + 128, 15872 + 992 + 128) >> 8 = 16 36 66
"""
import numpy as np
import pytest

import lk_cases
import lk_ref


def test_pyrdown_of_a_constant_is_that_constant():
    for v in (0, 1, 127, 255):
        for shape in ((6, 6), (23, 45), (50, 31)):
            assert np.all(lk_ref.pyr_down(np.full(shape, v, np.uint8)) == v)
    assert lk_ref.pyr_down(np.zeros((37, 83), np.uint8)).shape == (19, 42)


def test_pyrdown_hand_worked_example():
    img = (16 * np.arange(6)[None, :] + np.arange(6)[:, None]).astype(np.uint8)
    assert lk_ref.pyr_down(img).tolist() == [[13, 33, 63], [14, 34, 64], [16, 36, 66]]


def test_scharr_of_a_ramp_and_its_border():
    img = np.tile(3 * np.arange(30, dtype=np.uint8), (25, 1))
    d = lk_ref.scharr(img)
    assert d.dtype == np.int16 and d.shape == (25, 30, 2)
    assert np.all(d[:, 1:-1, 0] == 16 * 6) and np.all(d[:, :, 1] == 0)
    assert np.all(d[:, 0, 0] == 0) and np.all(d[:, -1, 0] == 0)        # reflect-101: both neighbours are the same pixel


@pytest.mark.parametrize("w,h,top,sizes", [
    (200, 180, 3, None), (185, 177, 3, [(93, 89), (47, 45), (24, 23)]), (120, 50, 1, None), (1241, 48, 1, None), (40, 40, 0, None),
    (83, 37, 0, None)])
def test_level_rule(w, h, top, sizes):
    got = lk_ref.level_sizes(w, h)
    assert len(got) - 1 == top
    if sizes:
        assert got[1:] == sizes
    levels, derivs = lk_ref.build_pyramid(np.zeros((h, w), np.uint8))
    assert [(l.shape[1], l.shape[0]) for l in levels] == got and [d.shape[:2] for d in derivs] == [l.shape for l in levels]
    assert len(lk_ref.level_sizes(w, h, max_level=0)) == 1


def test_planted_translations_are_recovered():
    """Points at least 40 px from every edge of a 200 x 180 smooth texture.  The restatement's largest error over the seven
    shifts, measured here on the CPU: 0.0436 px (at shift (1.5, 2.25); the images are rounded to 8 bits after the bilinear
    resampling).  The assertion is at twice that."""
    worst = 0.0
    for shift in lk_cases.SHIFTS:
        prev, nxt = lk_cases.planted_pair(11, 200, 180, shift)
        pts = lk_cases.inner_grid(200, 180)
        assert len(pts) >= 40 and pts.min() >= 40 and np.all(pts[:, 0] <= 160) and np.all(pts[:, 1] <= 140)
        r = lk_ref.track(prev, nxt, pts)
        assert r["top"] == 3 and np.all(r["status"] == 1)
        e = float(np.abs(r["next_pts"] - pts - np.float32(shift)).max())
        print("shift %s: largest error %.4f px" % (shift, e))
        worst = max(worst, e)
        assert np.all(r["err"] >= 0) and np.all(r["err"] < 8)
    assert worst < 0.0872          # measured 0.0436


def test_range_exit_outside_the_image():
    prev, nxt = lk_cases.exits_pair()
    r = lk_ref.track(prev, nxt, [lk_cases.OUTSIDE_POINT])
    assert r["exits"][0, 0] == lk_ref.EXIT_RANGE_PREV and r["status"][0] == 0 and r["err"][0] == 0


def test_min_eig_exit_in_a_constant_patch():
    prev, nxt = lk_cases.exits_pair()
    r = lk_ref.track(prev, nxt, [lk_cases.FLAT_POINT])
    assert r["exits"][0, 0] == lk_ref.EXIT_MIN_EIG and r["status"][0] == 0 and r["err"][0] == 0
    assert r["iterations"][0, 0] == 0


def test_drift_out_of_the_image_during_the_iterations():
    prev, nxt = lk_cases.exits_pair()
    assert lk_cases.DRIFT_POINT[0] == prev.shape[1] - 3
    r = lk_ref.track(prev, nxt, [lk_cases.DRIFT_POINT])
    assert r["exits"][0, 0] == lk_ref.EXIT_RANGE_NEXT and r["iterations"][0, 0] >= 1 and r["status"][0] == 0
    assert r["err"][0] == 0 and r["next_pts"][0, 0] >= prev.shape[1] + 10      # floor(x - 10) >= cols


def test_epsilon_exit():
    prev, nxt = lk_cases.planted_pair(11, 200, 180, lk_cases.SHIFTS[2])
    r = lk_ref.track(prev, nxt, [lk_cases.EPSILON_POINT])
    assert r["exits"][0, 0] == lk_ref.EXIT_EPSILON and r["status"][0] == 1 and 1 <= r["iterations"][0, 0] < 30
    assert r["err"][0] > 0


def test_oscillation_exit():
    prev, nxt = lk_cases.low_contrast_pair()
    r = lk_ref.track(prev, nxt, [lk_cases.OSCILLATION_POINT])
    assert r["exits"][0, 0] == lk_ref.EXIT_OSCILLATION and r["status"][0] == 1 and 2 <= r["iterations"][0, 0] < 30


def test_all_thirty_iterations():
    prev, nxt = lk_cases.wander_pair()
    r = lk_ref.track(prev, nxt, [lk_cases.MAX_COUNT_POINT])
    assert r["top"] == 0 and r["exits"][0, 0] == lk_ref.EXIT_MAX_COUNT and r["iterations"][0, 0] == 30 and r["status"][0] == 1


def test_the_gpu_suites_point_set_reaches_every_exit():
    prev, nxt = lk_cases.exits_pair()
    pts = lk_cases.exits_points(300)
    assert pts.shape == (300, 2) and pts.dtype == np.float32
    r = lk_ref.track(prev, nxt, pts)
    for code in range(1, 7):
        assert (r["exits"] == code).any(), code
    assert 0 < r["status"].sum() < 300
