"""CPU suite of the semi-global block matcher's eight-direction mode (MODE_HH): the numpy restatement tests/sgbm_hh_ref.py
against its pinned hashes, against the five-direction restatements in the directions they share, against itself upside down;
a census of what the cases exercise; the host-only argument checks of the four entries that take a mode."""
import ctypes as C
import json

import numpy as np
import pytest

import sgbm_bgr_cases
import sgbm_bgr_ref
import sgbm_cases
import sgbm_hh_cases as cases
import sgbm_hh_ref
import sgbm_ref

ALL = [("gray", n) for n in cases.GRAY_CASES] + [("bgr", n) for n in cases.BGR_CASES]


def _ref(kind, name):
    return cases.ref(name) if kind == "gray" else cases.ref_bgr(name)


def _old_ref(kind, name):
    return sgbm_cases.ref(name) if kind == "gray" else sgbm_bgr_cases.ref(name)


@pytest.mark.parametrize("kind,name", ALL)
def test_restatement_equals_its_pins(kind, name):
    """Every stage of every case hashes to what tests/golden/sgbm_hh_restatement_pins.json recorded when the contract was
    written: a change of the restatement shows here, not as a silent change of what the device is compared against."""
    pins = json.load(open(cases.PINS))
    assert sorted(pins) == sorted("%s/%s" % kn for kn in ALL)
    assert cases.stage_hashes(_ref(kind, name)[3]) == pins["%s/%s" % (kind, name)]


def _small_C(kind):
    """A block-cost volume small enough to walk 13 directions over: rows and columns cut out of a real case (the wrap case for
    colour, so that the carries wrap)."""
    if kind == "gray":
        _, _, D, out = cases.ref("noise83x37")
        return out["C"][:11, :40].astype(np.int64), D
    _, _, D, out = cases.ref_bgr(cases.WRAP_CASE)
    return out["C"][:, :44].astype(np.int64), D


@pytest.mark.parametrize("kind", ["gray", "bgr"])
def test_directions_0_to_4_are_the_five_direction_restatements(kind):
    C_, D = _small_C(kind)
    old = sgbm_ref.path_cost if kind == "gray" else sgbm_bgr_ref.path_cost
    for k in range(5):
        assert sgbm_hh_ref.DIRS8[k] == sgbm_ref.DIRS[k]
        got = sgbm_hh_ref.path_cost8(C_, D, k, cn=1 if kind == "gray" else 3)
        assert np.array_equal(got, old(C_.astype(np.int32) if kind == "gray" else C_, D, k)), k


@pytest.mark.parametrize("kind", ["gray", "bgr"])
def test_directions_5_6_7_mirror_3_2_1(kind):
    """The volumes of directions 5, 6 and 7 equal those of 3, 2 and 1 on the vertically flipped C, flipped back - computed with
    the five-direction restatements' own path functions."""
    C_, D = _small_C(kind)
    old = sgbm_ref.path_cost if kind == "gray" else sgbm_bgr_ref.path_cost
    flipped = np.ascontiguousarray(C_[::-1]).astype(np.int32 if kind == "gray" else np.int64)
    for new, mirror in ((5, 3), (6, 2), (7, 1)):
        got = sgbm_hh_ref.path_cost8(C_, D, new, cn=1 if kind == "gray" else 3)
        want = old(flipped, D, mirror)[::-1]
        assert np.array_equal(got, want), new
        if kind == "bgr":
            assert (np.abs(got) > 32767).any()       # the comparison covers wrapped carries


@pytest.mark.parametrize("kind,name", ALL)
def test_unreachable_guards_stay_unreached(kind, name):
    assert sgbm_cases.impossible(_ref(kind, name)[3]) == dict(denominator_clamped=0, probe_left_of_image=0)


def test_census_every_rule_of_the_winner_stage_is_live():
    cen = {name: sgbm_cases.census(cases.ref(name)[3]) for name in cases.GRAY_CASES}
    for name, c in cen.items():
        print(name, c)
    for key in sgbm_cases.CENSUS_KEYS:
        assert any(c[key] > 0 for c in cen.values()), key
    bars, noise, sat = cen["bars64x8s29"], cen["noise83x37"], cen["saturated120x30"]
    assert (bars["bid_ties"], bars["left_right_invalidated"], bars["sum5_saturated"]) == (10, 60, 600)
    assert (noise["best_first"], noise["best_last"], noise["sum5_saturated"]) == (15, 1, 243)
    assert (sat["uniqueness_rejections"], sat["sum4_saturated"], sat["sum5_saturated"]) == (2635, 24880, 48549)
    assert cen["binary64x8s5348"]["best_first"] > 0 and cen["binary64x8s5348"]["best_last"] > 0
    # the second pass's three new directions together leave int16 (an accumulator may hold two of them at most)
    out = cases.ref("saturated120x30")[3]
    assert out["second3_max"] == 37974 > 32767 and out["S"].shape == (30, 120, 16)


def test_colour_steps_leave_int16_in_each_new_direction():
    per_dir = cases.ref_bgr(cases.WRAP_CASE)[3]["carried_out_dir"]
    print(per_dir)
    assert per_dir[5:] == [3580, 3748, 3755] and all(n > 0 for n in per_dir)


def _sum8_sides(out):
    s8 = out["sum5"][:, int(out["D"]):]
    return int((s8 > 32767).sum()), int((s8 < -32768).sum())


def test_colour_sum8_saturates_high():
    assert _sum8_sides(cases.ref_bgr(cases.WRAP_CASE)[3])[0] == 4834


def test_colour_sum8_saturates_low():
    out = cases.ref_bgr(cases.GRAY_REPLICATED_CASE)[3]
    assert _sum8_sides(out) == (0, 984) and out["S"].size == 64 * 20 * 16 and (out["S"] == -32768).sum() == 984


@pytest.mark.parametrize("kind,name", ALL)
def test_the_mode_changes_the_map(kind, name):
    """The eight-direction map (before the left-right check) differs from the five-direction one on every case - a device that
    ignored the mode could pass none of them - while C and S4 are the five-direction restatement's."""
    new, old = _ref(kind, name)[3], _old_ref(kind, name)[3]
    for k in ("C", "sum4", "S4"):
        assert np.array_equal(new[k], old[k]), k
    assert (new["disp1_raw"] != old["disp1_raw"]).any() and (new["S"] != old["S"]).any()
    if (kind, name) == ("gray", "noise83x37"):
        assert int((new["disp1_raw"] != old["disp1_raw"]).sum()) == 269 and new["disp1_raw"].size == 3071


def test_host_side_argument_checks_of_the_mode_entries(pkg):
    """The four entries exist and answer a bad mode and an oversized image on the host, with a NULL context."""
    lib = pkg.load_library()
    for name in ("svo_sgbm_process_mode", "svo_sgbm_process_bgr_mode", "svo_sgbm_batch_mode_dev", "svo_sgbm_batch_bgr_mode_dev"):
        assert hasattr(lib, name) and name in pkg.ABI_SYMBOLS, name
    assert (pkg.SGBM_MODE_SGBM, pkg.SGBM_MODE_HH) == (0, 1)
    buf = np.zeros(16, np.uint8).ctypes.data_as(C.c_void_p)
    E_INVALID = -1
    E_CAPACITY = lib.svo_sgbm_process(None, buf, buf, 3073, 3073, 100, C.byref(pkg.sgbm_default_params(100)), None, None)
    assert E_CAPACITY not in (0, E_INVALID)
    g, c = pkg.sgbm_default_params(100), pkg.sgbm_default_params_bgr(100)
    for mode, want in ((2, E_INVALID), (-1, E_INVALID)):
        assert lib.svo_sgbm_process_mode(None, buf, buf, 100, 100, 100, C.byref(g), mode, None, None) == want
        assert lib.svo_sgbm_process_bgr_mode(None, buf, buf, 300, 100, 100, C.byref(c), mode, None, None) == want
        assert lib.svo_sgbm_batch_mode_dev(None, buf, buf, 100, 100, 100, 1, C.byref(g), mode, buf) == want
        assert lib.svo_sgbm_batch_bgr_mode_dev(None, buf, buf, 300, 100, 100, 1, C.byref(c), mode, buf) == want
        # (the mode is a parameter and is judged with the parameters, before the sizes: not the answer a NULL context gets anyway)
        assert lib.svo_sgbm_process_mode(None, buf, buf, 3073, 3073, 100, C.byref(g), mode, None, None) == want
        assert lib.svo_sgbm_batch_bgr_mode_dev(None, buf, buf, 3 * 3073, 3073, 100, 1, C.byref(c), mode, buf) == want
    for mode in (0, 1):
        assert lib.svo_sgbm_process_mode(None, buf, buf, 3073, 3073, 100, C.byref(g), mode, None, None) == E_CAPACITY
        assert lib.svo_sgbm_process_bgr_mode(None, buf, buf, 3 * 3073, 3073, 100, C.byref(c), mode, None, None) == E_CAPACITY
        assert lib.svo_sgbm_batch_mode_dev(None, buf, buf, 3073, 3073, 100, 1, C.byref(g), mode, buf) == E_CAPACITY
        assert lib.svo_sgbm_batch_bgr_mode_dev(None, buf, buf, 3 * 3073, 3073, 100, 1, C.byref(c), mode, buf) == E_CAPACITY
        # a good mode and a good size, and still no context
        assert lib.svo_sgbm_process_mode(None, buf, buf, 100, 100, 100, C.byref(g), mode, None, None) == E_INVALID
        # each entry keeps its own parameter set
        assert lib.svo_sgbm_process_mode(None, buf, buf, 3073, 3073, 100, C.byref(c), mode, None, None) == E_INVALID
        assert lib.svo_sgbm_process_bgr_mode(None, buf, buf, 3 * 3073, 3073, 100, C.byref(g), mode, None, None) == E_INVALID
