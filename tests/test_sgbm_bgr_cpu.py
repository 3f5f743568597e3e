"""CPU suite of the colour (cn = 3) semi-global block matcher: the numpy restatement tests/sgbm_bgr_ref.py against its pinned
hashes, against the gray restatement on replicated gray, and a census of what the cases exercise; the host-only entries of
the library (parameter sets, argument checks that need no device)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import sgbm_bgr_cases as cases
import sgbm_bgr_ref
import sgbm_ref

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sgbm_bgr_restatement_pins.json")


@pytest.mark.parametrize("name", cases.CASES)
def test_restatement_equals_its_pins(name):
    """Every stage of every case hashes to what tests/golden/sgbm_bgr_restatement_pins.json recorded when the contract was
    written: a change of the restatement shows here, not as a silent change of what the device is compared against."""
    pins = json.load(open(PINS))
    assert sorted(pins) == sorted(cases.CASES)
    assert cases.stage_hashes(cases.ref(name)[3]) == pins[name]


def test_wrap16_and_parameters_of_the_restatement():
    assert (sgbm_bgr_ref.P1, sgbm_bgr_ref.P2) == (1944, 7776)
    a = np.array([0, 32767, 32768, 39852, 45927, 65535, 65536, -32768, -32769, -106079])
    assert sgbm_bgr_ref.wrap16(a).tolist() == [0, 32767, -32768, -25684, -19609, -1, 0, -32768, 32767, 24993]
    assert np.array_equal(sgbm_bgr_ref.wrap16(a), a.astype(np.int32).astype(np.int16))


def test_replicated_gray_is_three_times_the_gray_restatement():
    """On (g, g, g) every plane pair is the gray one, the pixel cost is three times gray's, and so are P1 and P2: while nothing
    wraps or saturates the recurrence is homogeneous (every v is three times gray's), the uniqueness test compares ratios and
    the parabola is a ratio (its clamp max(den, 1) never acts: the winner is the first minimum, so den >= 1) - disp16 is
    identical.  The precondition is read off the gray restatement."""
    gL, gR = cases.gray_pair()
    D = 16
    g = sgbm_ref.sgbm(gL, gR, D)
    assert 3 * int(np.abs(g["sum5"][:, D:]).max()) <= 32767
    assert 3 * int(np.abs(g["sum4"][:, D:]).max()) <= 32767 and 3 * int(g["C"].max()) <= 32767
    L, R, Dc, c = cases.ref(cases.GRAY_CASE)
    assert Dc == D and np.array_equal(L[:, :, 1], gL) and np.array_equal(R[:, :, 2], gR)
    assert np.array_equal(c["Ctrue"], 3 * g["C"].astype(np.int32)) and np.array_equal(c["C"], 3 * g["C"])
    assert np.array_equal(c["sum4"], 3 * g["sum4"]) and np.array_equal(c["sum5"], 3 * g["sum5"])
    assert np.array_equal(c["S"], 3 * g["S"])
    for k in ("disp2", "disp1_raw", "disp1_lr", "disp16"):
        assert np.array_equal(c[k], g[k]), k
    assert c["disp"].tobytes() == g["disp"].tobytes()
    valid = g["disp16"] != -16
    assert valid.mean() > 0.5 and len(np.unique(g["disp16"][valid])) >= 3     # a real map with subpixel terms


def test_wrap_case_is_what_the_gray_restatement_says_it_is():
    """Three times the gray block sum of one channel of the wrap pair peaks at 39 852 and exceeds 32 767 on 27 % of the volume."""
    L, R, D, c = cases.ref(cases.WRAP_CASE)
    assert L.shape == (12, 80, 3) and D == 16
    P = sgbm_ref.pixel_cost(L[:, :, 0], R[:, :, 0], D)
    H, W = P.shape[:2]
    Cg = np.zeros_like(P)
    xs, ys = np.arange(D, W), np.arange(H)
    for dy in range(-4, 5):
        for dx in range(-4, 5):
            Cg[:, D:] += P[np.clip(ys + dy, 0, H - 1)][:, np.clip(xs + dx, D, W - 1)]
    assert 3 * int(Cg.max()) == 39852 == int(c["Ctrue"].max())
    assert 0.26 < (3 * Cg > 32767).mean() < 0.28
    assert np.array_equal(c["Ctrue"], 3 * Cg)
    assert (c["C"] < 0).any() and np.array_equal(c["C"].astype(np.int64), sgbm_bgr_ref.wrap16(c["Ctrue"]))


def test_census_wrapping_is_live_on_the_wrap_case_and_nowhere_else():
    """Both rules that exist only with three channels decide something on the wrap case; on every other case the block sum
    fits a short and no carried step leaves it, so those cases isolate everything else."""
    for name in cases.CASES:
        cen = cases.census(cases.ref(name)[3])
        print(name, cen)
        if name == cases.WRAP_CASE:
            assert cen["block_sum_over"] > 0 and cen["carried_out"] > 0
            assert cen["sum4_saturated"] > 0 and cen["sum5_saturated"] > 0
        else:
            assert cen["block_sum_over"] == 0 and cen["carried_out"] == 0, name
    out = cases.ref("shifted96x40d32")[3]
    d16 = out["disp16"]
    for d, rows in zip((4, 9, 15), (slice(2, 11), slice(16, 24), slice(30, 38))):     # the bands' true disparities win
        band = d16[rows, 40:90]
        assert (np.abs(band[band != -16] - 16 * d) <= 8).mean() > 0.9 and (band != -16).mean() > 0.5, d


def test_parameter_sets_and_host_side_argument_checks(pkg):
    lib = pkg.load_library()
    g, c = pkg.sgbm_default_params(376), pkg.sgbm_default_params_bgr(376)
    assert (c.P1, c.P2) == (1944, 7776) == (3 * g.P1, 3 * g.P2)
    for f, _ in pkg.SgbmParams._fields_:
        if f not in ("P1", "P2"):
            assert getattr(g, f) == getattr(c, f), f
    assert c.numDisparities == 48
    assert lib.svo_sgbm_default_params_bgr(100, None) == -1 and lib.svo_sgbm_default_params_bgr(-1, C.byref(c)) == -1
    # sizes and parameters are answered on the host, before the context is looked at
    buf = np.zeros(16, np.uint8).ctypes.data_as(C.c_void_p)
    E_INVALID, E_CAPACITY = -1, lib.svo_sgbm_process(None, buf, buf, 3073, 3073, 100, C.byref(pkg.sgbm_default_params(100)), None, None)
    assert E_CAPACITY not in (0, E_INVALID)
    p = pkg.sgbm_default_params_bgr(100)
    assert lib.svo_sgbm_process_bgr(None, buf, buf, 3 * 3073, 3073, 100, C.byref(p), None, None) == E_CAPACITY
    assert lib.svo_sgbm_process_bgr(None, buf, buf, 3 * 100, 100, 4097, C.byref(pkg.sgbm_default_params_bgr(4097)), None, None) == E_INVALID   # D = 528
    assert lib.svo_sgbm_batch_bgr_dev(None, buf, buf, 3 * 3073, 3073, 100, 1, C.byref(p), buf) == E_CAPACITY
    assert lib.svo_sgbm_process_bgr(None, buf, buf, 300, 100, 100, C.byref(p), None, None) == E_INVALID          # no context
    assert lib.svo_sgbm_process_bgr(None, buf, buf, 3 * 3073, 3073, 100, C.byref(pkg.sgbm_default_params(100)), None, None) == E_INVALID   # gray's set
    assert lib.svo_sgbm_process(None, buf, buf, 3073, 3073, 100, C.byref(p), None, None) == E_INVALID            # colour's set
