"""CPU suite of the semi-global block matcher: the C-ABI additions (symbols, default parameters, argument checks that come
before any device is touched) and the sanity of the numpy restatement tests/sgbm_ref.py, the yardstick the GPU tests compare
the device against."""
import ctypes as C

import numpy as np
import pytest

import sgbm_cases
import sgbm_ref
import test_abi


def test_abi_agreement_holds_with_the_sgbm_entries(pkg):
    names = {"svo_sgbm_default_params", "svo_sgbm_process", "svo_sgbm_batch_dev", "svo_sgbm_debug_volume", "svo_sgbm_filter_speckles"}
    assert names <= set(pkg.ABI_SYMBOLS) and names <= set(test_abi.declared_symbols())
    assert test_abi.declared_symbols() == sorted(pkg.ABI_SYMBOLS)
    lib = C.CDLL(pkg.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), n
    assert lib.svo_abi_version() == 8


def test_default_params_are_elasmatch_s(pkg):
    p = pkg.sgbm_default_params(376)
    got = {k: getattr(p, k) for k, _ in p._fields_}
    assert got == dict(minDisparity=0, numDisparities=48, blockSize=9, P1=648, P2=2592, disp12MaxDiff=1, preFilterCap=63,
                       uniquenessRatio=10, speckleWindowSize=100, speckleRange=32)
    assert pkg.sgbm_default_params(135).numDisparities == 16
    assert pkg.sgbm_default_params(136).numDisparities == 32
    for h in (2, 135, 136, 376, 511, 512):
        assert pkg.sgbm_default_params(h).numDisparities == sgbm_ref.default_D(h)
    assert pkg.load_library().svo_sgbm_default_params(376, None) == -1


def test_process_rejects_bad_arguments_before_any_device(pkg):
    """There is no device here, hence no context: every call below passes a NULL one.  The parameter and size checks are host
    arithmetic that comes first - an image beyond the capacity answers SVO_E_CAPACITY (-5) even without a context, which is
    what shows them at work; each unsupported parameter then turns that answer into SVO_E_INVALID (-1), and a supported call
    without a context is SVO_E_INVALID too."""
    lib = pkg.load_library()
    W, H = 96, 40
    img = np.zeros((H, W), np.uint8)
    out = np.zeros((H, W), np.int16)
    ip = img.ctypes.data_as(C.c_void_p)
    op = out.ctypes.data_as(C.c_void_p)
    p = pkg.sgbm_default_params(H)
    assert p.numDisparities == 16
    BIG = 5000   # rows: beyond the capacity, nothing else wrong
    assert lib.svo_sgbm_process(None, ip, ip, W, W, BIG, C.byref(p), op, None) == -5
    assert lib.svo_sgbm_process(None, ip, ip, 25, 25, BIG, C.byref(p), op, None) == -5        # W = D + 9: accepted
    assert lib.svo_sgbm_process(None, ip, ip, 24, 24, BIG, C.byref(p), op, None) == -1        # W = D + 8
    assert lib.svo_sgbm_process(None, ip, ip, W, W, 1, C.byref(p), op, None) == -1            # H < 2
    for change in (dict(numDisparities=24), dict(numDisparities=80), dict(numDisparities=0), dict(blockSize=7), dict(P1=600),
                   dict(P2=2000), dict(minDisparity=1), dict(uniquenessRatio=15), dict(speckleWindowSize=0),
                   dict(speckleRange=2), dict(disp12MaxDiff=-1), dict(preFilterCap=31)):
        q = pkg.sgbm_default_params(H)
        for k, v in change.items():
            setattr(q, k, v)
        assert lib.svo_sgbm_process(None, ip, ip, W, W, BIG, C.byref(q), op, None) == -1, change
        assert lib.svo_sgbm_batch_dev(None, ip, ip, W, W, BIG, 1, C.byref(q), op) == -1, change
    for D in (16, 32, 48, 64):
        q = pkg.sgbm_default_params(H)
        q.numDisparities = D
        assert lib.svo_sgbm_process(None, ip, ip, W, W, BIG, C.byref(q), op, None) == -5, D
    # a NULL ctx with everything else in order, and NULL parameters
    assert lib.svo_sgbm_process(None, ip, ip, W, W, H, C.byref(p), op, None) == -1
    assert lib.svo_sgbm_batch_dev(None, ip, ip, W, W, H, 1, C.byref(p), op) == -1
    assert lib.svo_sgbm_process(None, ip, ip, W, W, H, None, op, None) == -1
    assert lib.svo_sgbm_debug_volume(None, 0, op) == -1


def _shifted(k, W=96, H=40):
    L = np.random.default_rng(1234).integers(0, 256, (H, W), dtype=np.uint8)
    R = np.empty_like(L)
    R[:, :W - k] = L[:, k:]
    R[:, W - k:] = np.random.default_rng(5).integers(0, 256, (H, k), dtype=np.uint8)
    return L, R


@pytest.mark.parametrize("k", [3, 11])
def test_restatement_finds_a_planted_shift(k):
    """iid bytes shifted by k: every right pixel is a byte-identical copy of its left match, the pixel cost is 0 at d = k.
    Every valid interior pixel must land within the subpixel formula's range around k, and most of the interior is valid."""
    W, H, D = 96, 40, 16
    L, R = _shifted(k, W, H)
    o = sgbm_ref.sgbm(L, R, D)
    inner = o["disp16"][5:H - 5, D + k + 5:W - 5].astype(np.int32)
    valid = inner != -16
    assert valid.mean() > 0.5
    assert inner[valid].min() >= 16 * k - 7 and inner[valid].max() <= 16 * k + 8
    assert np.all(o["disp16"][:, :D] == -16)
    assert np.array_equal(o["disp"], o["disp16"].astype(np.float32) / np.float32(16)) and np.all(o["disp"][o["disp16"] == -16] == -1.0)


def test_restatement_flat_cost_keeps_disparity_zero():
    """Constant images, 12 rows: every cost is 0, so S is the same for every d (planted ties).  The first minimum is d = 0 and
    the uniqueness test (S[d] * 90 < minS * 100 on signed ints, S negative) must not reject: S * 90 > S * 100 for S < 0."""
    L = np.full((12, 64), 100, np.uint8)
    o = sgbm_ref.sgbm(L, L.copy(), 16)
    assert np.all(o["C"] == 0)
    S = o["S"][:, 16:].astype(np.int32)
    assert np.all(S == S[:, :, :1]) and S.max() < 0
    raw = o["disp1_raw"]
    assert np.all(raw[:, 16:] == 0) and np.all(raw[:, :16] == -16)
    assert np.all(o["disp2"][:, 16:] == 0)   # column x2 = x is bid for by x itself only


def test_subpixel_division_truncates_toward_zero():
    """S[best-1] = 10, S[best] = 0, S[best+1] = 14: den = 24, numerator = (10 - 14) * 16 + 24 = -40, -40 / 48 = 0 in C
    (numpy's // gives -1).  And one that does not vanish: S = (10, 0, 90): den = 100, numerator = -1180, / 200 = -5 in C
    (floor: -6)."""
    S = np.full(16, 1000, np.int64)
    S[4:7] = (10, 0, 14)
    assert sgbm_ref.subpixel(S, 5, 16) == 5 * 16
    S[4:7] = (10, 0, 90)
    assert sgbm_ref.subpixel(S, 5, 16) == 5 * 16 - 5
    S[4:7] = (90, 0, 10)                       # positive side: (80 * 16 + 100) / 200 = 6
    assert sgbm_ref.subpixel(S, 5, 16) == 5 * 16 + 6
    assert sgbm_ref.subpixel(S, 0, 16) == 0 and sgbm_ref.subpixel(S, 15, 16) == 240   # no neighbours on one side: no fraction


def test_restatement_speckle_sizes():
    d = np.full((30, 60), 160, np.int16)
    d[2:11, 2:13] = 2000            # 99 pixels
    d[2:12, 20:30] = 2000           # 100 pixels
    d[15:16, 2:52] = 2000; d[16:17, 2:53] = 2000   # 101 pixels
    out = sgbm_ref.speckles(d)
    assert np.all(out[2:11, 2:13] == -16) and np.all(out[2:12, 20:30] == -16)
    assert np.all(out[15, 2:52] == 2000) and np.all(out[16, 2:53] == 2000)
    assert (out == 160).sum() == d.size - 300


# ---- what the device's stage cases exercise ----------------------------------------------------------------------------------
def _census_case(out, **planted):
    """census() on a hand-made S volume (x < D empty); disp1_raw comes from the restatement's own winner loop."""
    raw, disp2 = sgbm_ref.winner(out["S"].astype(np.int32), out["D"])
    full = dict(out, disp1_raw=raw, disp1_lr=planted.get("disp1_lr", raw), sum4=out["S"].astype(np.int32), sum5=out["S"].astype(np.int32))
    return sgbm_cases.census(full), disp2


def test_census_counts_planted_rules():
    """One row, D = 16, W = 40, S = 1000 everywhere but for planted minima.  Pixels 30 (best 5) and 27 (best 2) both bid 77 for
    column 25: one tie, and the larger x keeps the column.  Pixel 20 wins at d = 15, pixel 22 at d = 0; pixel 35 has the
    numerator (10 - 14) * 16 + 24 = -40, no multiple of 48; pixel 33 has a rival at d = 9 within 10 % and is rejected, as
    is every untouched pixel."""
    D, W = 16, 40
    S = np.full((1, W, D), 1000, np.int16)
    S[0, :D] = 0
    S[0, 30, 5] = 77; S[0, 27, 2] = 77
    S[0, 20, 15] = 500; S[0, 22, 0] = 500
    S[0, 35, 4:7] = (510, 500, 514)
    S[0, 33, 3] = 600; S[0, 33, 9] = 660
    c, disp2 = _census_case(dict(D=D, S=S))
    assert disp2[0, 25] == 5, "the restatement keeps the bid of the largest x"
    assert c["bid_ties"] == 1 and c["best_first"] == 1 and c["best_last"] == 1 and c["negative_numerator_with_remainder"] == 1
    flat = (W - D) - 6                       # the untouched pixels: all S equal and positive, 1000 * 90 < 1000 * 100 rejects them
    assert c["uniqueness_rejections"] == flat + 1
    assert c["left_right_invalidated"] == 0 and c["sum4_saturated"] == 0 and c["sum5_saturated"] == 0
    S[0, 27, 2] = 78                         # no tie any more: the lower bid wins whatever the order
    c, disp2 = _census_case(dict(D=D, S=S))
    assert c["bid_ties"] == 0 and disp2[0, 25] == 5


def test_every_written_rule_is_live_in_the_union_of_the_stage_cases():
    """The device is compared with the restatement on sgbm_cases.STAGE_CASES.  A rule that never decides anything there is a
    rule the device could have wrong unnoticed, so each count of the census must be at least 1 over the union of the cases, and
    tied right-image bids at least 8: one lucky ordering of the device's atomics must not be enough."""
    total = dict.fromkeys(sgbm_cases.CENSUS_KEYS, 0)
    for name in sgbm_cases.STAGE_CASES:
        c = sgbm_cases.census(sgbm_cases.ref(name)[3])
        assert tuple(c) == sgbm_cases.CENSUS_KEYS
        print("%-20s valid %.2f / %.2f  %s" % ((name,) + sgbm_cases.valid_fractions(sgbm_cases.ref(name)[3]) + (list(c.values()),)))
        for k, v in c.items():
            total[k] += v
    print("union", total)
    for k, v in total.items():
        assert v >= (8 if k == "bid_ties" else 1), (k, v)
    tie_total = sum(sgbm_cases.census(sgbm_cases.ref(n)[3])["bid_ties"] for n in sgbm_cases.TIE_CASES)
    assert tie_total >= 8, "the pairs the search found carry the ties"


def test_two_guards_of_the_contract_can_never_fire():
    """The denominator clamp and the left-right probe's x - a < 0 (see sgbm_cases.census for why): 0 on every stage case."""
    for name in sgbm_cases.STAGE_CASES:
        assert sgbm_cases.impossible(sgbm_cases.ref(name)[3]) == dict(denominator_clamped=0, probe_left_of_image=0), name


def test_stage_cases_are_the_shapes_they_claim():
    for name in sgbm_cases.PORTRAIT_CASES:
        L, _, D = sgbm_cases.case(name)
        assert L.shape[0] > L.shape[1] - D, name
    assert sgbm_cases.case("tall30x300d16")[0].shape == (300, 30)
    assert sgbm_cases.case("portrait75x100d48")[2] == 48
    assert sgbm_cases.case("wide3072x2d16")[0].shape == (2, 3072)
    for name in sgbm_cases.MINIMAL_CASES:
        L, _, D = sgbm_cases.case(name)
        out = sgbm_cases.ref(name)[3]
        assert L.shape == (2, D + 9)
        assert (out["disp1_lr"] != -16).any() and np.all(out["disp16"] == -16)
    for name in sgbm_cases.STAGE_CASES:
        if name not in sgbm_cases.MINIMAL_CASES:
            assert sgbm_cases.valid_fractions(sgbm_cases.ref(name)[3])[1] > 0.2, name


def test_speckle_maps_are_what_the_device_tests_need():
    d = sgbm_cases.serpentine()
    assert d.shape == (64, 600) and (d != -16).sum() == 19232
    assert np.array_equal(sgbm_ref.speckles(d.astype(np.int32)), d), "one component, far above 100 pixels"
    cut = d.copy(); cut[31, :] = -16         # (row 31 holds the one pixel that joins the upper and the lower half)
    assert (sgbm_ref.speckles(cut.astype(np.int32)) != -16).sum() == 19231
    d, go, stay = sgbm_cases.comb()
    out = sgbm_ref.speckles(d.astype(np.int32))
    assert all(d[s].size == 100 and np.all(d[s] != -16) and np.all(out[s] == -16) for s in go)
    assert all(d[s].size == 101 and np.array_equal(out[s], d[s]) for s in stay)
    assert any(s[1].start <= 255 and s[1].stop > 256 for s in go + stay) and any(s[1].start <= 511 and s[1].stop > 512 for s in go + stay)
    d = sgbm_cases.seeded_speckle_map()
    assert d.shape == (129, 333) and 0.08 < (d == -16).mean() < 0.12 and np.all(d[d != -16] % 171 == 0)
    both = (d[:, 1:] != -16) & (d[:, :-1] != -16)
    dif = np.abs(np.diff(d.astype(np.int32), axis=1))[both]
    assert (dif == 342).sum() > 100 and (dif == 513).sum() > 100
