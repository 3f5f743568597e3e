"""CPU suite of the colour Lucas-Kanade work: the four _bgr entries are declared and bound and answer their arguments on the
host; the colour restatement (tests/lk_ref.py) against the gray one on B = G = R input, on planted translations and on
the isoluminant pair, which a gray tracker cannot follow at all."""
import ctypes as C

import numpy as np
import pytest

import lk_bgr_cases
import lk_cases
import lk_ref
import test_abi

BGR_SYMBOLS = ("svo_lk_track_bgr", "svo_lk_batch_bgr_dev", "svo_lk_chain_bgr_dev", "svo_lk_debug_level_bgr")


def test_the_four_entries_are_declared_bound_and_listed(pkg):
    lib = pkg.load_library()
    declared = test_abi.declared_symbols()
    for name in BGR_SYMBOLS:
        assert name in declared and name in pkg.ABI_SYMBOLS and hasattr(lib, name), name
    for name in ("lk_track_bgr", "lk_batch_bgr_dev", "lk_chain_bgr_dev", "lk_debug_level_bgr"):
        assert callable(getattr(pkg.Svo, name)), name
    assert lib.svo_abi_version() == 8


def test_arguments_are_answered_on_the_host_without_a_context(pkg):
    lib = pkg.load_library()
    p = pkg.lk_default_params()
    track = lib.svo_lk_track_bgr
    assert track(None, None, None, 360, 120, 50, C.byref(p), None, 4097, None, None, None) == -5
    assert track(None, None, None, 3 * 4097, 4097, 50, C.byref(p), None, 10, None, None, None) == -5
    assert track(None, None, None, 63, 21, 50, C.byref(p), None, 10, None, None, None) == -1
    assert track(None, None, None, 359, 120, 50, C.byref(p), None, 10, None, None, None) == -1          # stride < 3 * width
    assert lib.svo_lk_batch_bgr_dev(None, None, 600, 200, 180, 4097, C.byref(p), None, None, 10, None, None, None) == -5
    assert lib.svo_lk_chain_bgr_dev(None, None, 600, 200, 180, 4097, C.byref(p), None, None, 10, 10, None, None, None) == -5
    assert lib.svo_lk_debug_level_bgr(None, 0, 0, 0, None, None, None, None) == -1


@pytest.fixture(scope="module")
def replicated():
    """The gray planted pair of tests/test_lk_cpu.py and its B = G = R copy through both restatements."""
    prev, nxt = lk_cases.planted_pair(11, 200, 180, lk_cases.SHIFTS[2])
    pts = np.concatenate([lk_cases.inner_grid(200, 180, 40, 40), lk_cases.edge_points(200, 180, 6)]).astype(np.float32)
    return prev, nxt, pts, lk_ref.track(prev, nxt, pts), lk_ref.track(lk_bgr_cases.replicate(prev), lk_bgr_cases.replicate(nxt), pts)


def test_replicated_gray_every_level_and_plane_equals_the_gray_restatement(replicated):
    _, _, _, g, c = replicated
    assert c["top"] == g["top"] == 3
    for name in ("prev", "next"):
        for level in range(4):
            img, der = c["levels_" + name][level], c["derivs_" + name][level]
            assert img.dtype == np.uint8 and der.dtype == np.int16 and der.shape == img.shape[:2] + (6,)
            for ch in range(3):
                assert np.array_equal(img[:, :, ch], g["levels_" + name][level]), (name, level, ch)
                assert np.array_equal(der[:, :, 2 * ch:2 * ch + 2], g["derivs_" + name][level]), (name, level, ch)


def _gray_sums(levels, derivs, pt, level):
    """The gray contract's integer sums of ix^2, ix iy, iy^2 at one point and level, from lk_ref's own helpers."""
    F = np.float32
    px, py = F(pt[0]) * F(1.0 / (1 << level)) - F(10), F(pt[1]) * F(1.0 / (1 << level)) - F(10)
    ipx, ipy = int(np.floor(px)), int(np.floor(py))
    iw = lk_ref._weights(px - F(ipx), py - F(ipy))
    d = (lk_ref._sample_deriv(derivs[level], ipx, ipy, iw) + (1 << 13)) >> 14
    return [int((d[:, 0] * d[:, 0]).sum()), int((d[:, 0] * d[:, 1]).sum()), int((d[:, 1] * d[:, 1]).sum())]


def test_replicated_gray_window_sums_are_three_times_the_gray_ones(replicated):
    _, _, pts, g, c = replicated
    ran = np.flatnonzero(c["sums_level"] >= 0)
    assert len(ran) >= 10 and (c["sums_level"][ran] == 3).any()
    for i in ran:
        level = int(c["sums_level"][i])
        assert g["exits"][i, level] != lk_ref.EXIT_RANGE_PREV and (g["exits"][i, level + 1:] <= lk_ref.EXIT_RANGE_PREV).all()
        want = _gray_sums(g["levels_prev"], g["derivs_prev"], pts[i], level)
        assert c["sums"][i].tolist() == [3 * v for v in want], (i, level)
        assert want[0] > 0 and want[2] > 0


def test_planted_translations_are_recovered_in_colour():
    """Points at least 40 px from every edge of a 200 x 180 colour texture (three uncorrelated smooth canvases).  The colour
    restatement's largest error over the seven shifts, measured here on the CPU: 0.0267 px (the images are rounded to 8 bits
    after the bilinear resampling).  The assertion is at twice that."""
    worst = 0.0
    for shift in lk_cases.SHIFTS:
        prev, nxt = lk_bgr_cases.colour_pair((11, 12, 13), 200, 180, shift)
        pts = lk_cases.inner_grid(200, 180)
        assert len(pts) >= 40 and pts.min() >= 40 and np.all(pts[:, 0] <= 160) and np.all(pts[:, 1] <= 140)
        r = lk_ref.track(prev, nxt, pts)
        assert r["top"] == 3 and np.all(r["status"] == 1)
        e = float(np.abs(r["next_pts"] - pts - np.float32(shift)).max())
        print("shift %s: largest error %.4f px" % (shift, e))
        worst = max(worst, e)
        assert np.all(r["err"] >= 0) and np.all(r["err"] < 8)
    print("largest error over the shifts %.4f px" % worst)
    assert worst < MEASURED_PLANTED * 2


def test_the_isoluminant_pair_is_invisible_in_gray_and_tracked_in_colour():
    """COLOR_BGR2GRAY of both images is 128 at every pixel (the builder asserts it).  The gray restatement has a zero normal
    matrix at every inner-grid point: status 0.  The colour restatement tracks every one of them; its largest error against
    the planted (1.5, 2.25), measured here on the CPU: 0.0294 px.  The assertion is at twice that."""
    prev, nxt = lk_bgr_cases.isoluminant_pair()
    W, H = lk_bgr_cases.ISO_SIZE
    assert np.all(lk_bgr_cases.gray_of(prev) == 128) and np.all(lk_bgr_cases.gray_of(nxt) == 128)
    assert prev[:, :, 0].std() > 5 and prev[:, :, 2].std() > 5
    pts = lk_cases.inner_grid(W, H)
    assert len(pts) >= 40
    g = lk_ref.track(lk_bgr_cases.gray_of(prev), lk_bgr_cases.gray_of(nxt), pts)
    assert not g["status"].any() and (g["exits"][:, 0] == lk_ref.EXIT_MIN_EIG).all()
    c = lk_ref.track(prev, nxt, pts)
    assert np.all(c["status"] == 1)
    e = float(np.abs(c["next_pts"] - pts - np.float32(lk_bgr_cases.ISO_SHIFT)).max())
    print("isoluminant pair: largest error %.4f px" % e)
    assert e < MEASURED_ISO * 2


def test_the_colour_cases_reach_every_exit():
    prev, nxt = lk_bgr_cases.exits_pair()
    pts = lk_bgr_cases.exits_points()
    assert pts.shape == (lk_bgr_cases.EXITS_N, 2) and pts.dtype == np.float32
    r = lk_ref.track(prev, nxt, pts)
    for code in range(1, 7):
        assert (r["exits"] == code).any(), code
    assert r["exits"][:3, 0].tolist() == [lk_ref.EXIT_RANGE_PREV, lk_ref.EXIT_MIN_EIG, lk_ref.EXIT_RANGE_NEXT]
    assert r["iterations"][2, 0] >= 1 and not r["status"][:3].any() and 0 < r["status"].sum() < len(pts)
    r = lk_ref.track(*lk_bgr_cases.low_contrast_pair(), [lk_bgr_cases.OSCILLATION_POINT])
    assert r["exits"][0, 0] == lk_ref.EXIT_OSCILLATION and r["status"][0] == 1 and 2 <= r["iterations"][0, 0] < 30
    r = lk_ref.track(*lk_bgr_cases.wander_pair(), [lk_bgr_cases.MAX_COUNT_POINT])
    assert r["top"] == 0 and r["exits"][0, 0] == lk_ref.EXIT_MAX_COUNT and r["iterations"][0, 0] == 30 and r["status"][0] == 1


def test_one_point_two_statuses():
    """The faint pair as gray and as B = G = R: the colour sums are three times the gray ones against the same 882, so the
    point fails the minimum-eigenvalue test as gray and passes it as colour."""
    prev, nxt = lk_bgr_cases.faint_pair()
    g = lk_ref.track(prev, nxt, [lk_bgr_cases.SPLIT_POINT])
    c = lk_ref.track(lk_bgr_cases.replicate(prev), lk_bgr_cases.replicate(nxt), [lk_bgr_cases.SPLIT_POINT])
    assert g["status"][0] == 0 and g["exits"][0, 0] == lk_ref.EXIT_MIN_EIG and g["err"][0] == 0
    assert c["status"][0] == 1 and c["exits"][0, 0] in (lk_ref.EXIT_EPSILON, lk_ref.EXIT_OSCILLATION, lk_ref.EXIT_MAX_COUNT)


MEASURED_PLANTED = 0.0267          # px, the docstring of the planted test
MEASURED_ISO = 0.0294              # px, the docstring of the isoluminant test
