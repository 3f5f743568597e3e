"""CPU suite of the semi-global block matcher: the C-ABI additions (symbols, default parameters, argument checks that come
before any device is touched) and the sanity of the numpy restatement tests/sgbm_ref.py, the yardstick the GPU tests compare
the device against."""
import ctypes as C

import numpy as np
import pytest

import sgbm_ref
import test_abi


def test_abi_agreement_holds_with_the_sgbm_entries(pkg):
    names = {"svo_sgbm_default_params", "svo_sgbm_process", "svo_sgbm_batch_dev", "svo_sgbm_debug_volume", "svo_sgbm_filter_speckles"}
    assert names <= set(pkg.ABI_SYMBOLS) and names <= set(test_abi.declared_symbols())
    assert test_abi.declared_symbols() == sorted(pkg.ABI_SYMBOLS)
    lib = C.CDLL(pkg.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), n
    assert lib.svo_abi_version() == 7


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
