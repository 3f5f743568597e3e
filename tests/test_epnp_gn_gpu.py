"""epnp::gauss_newton with one column of the 6 x 4 system per lane on the device: svo_debug_epnp_gn - one launch of one wave, the
three candidates in its three DPP rows, the wave's own gauss_newton (csrc/svo_epnp_ord_dev.h) - reproduces every record of
tests/golden/epnp_gn_cases.npy (tools/make_epnp_gn_cases.py; what it covers: tests/test_epnp_gn_cpu.py) bit for bit."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return np.load(os.path.join(ROOT, "tests", "golden", "epnp_gn_cases.npy"))


def check(pkg, cases):
    svo = pkg.Svo(640, 240, max_batch=1)
    try:
        for i, c in enumerate(cases):
            got = svo.debug_epnp_gn(c["L"], c["rho"], c["bin"])
            ref = np.ascontiguousarray(c["bout"])
            key = (i, int(c["kind"]))
            nan = np.isnan(ref)
            assert np.array_equal(nan, np.isnan(got)), (key, got, ref)
            assert np.array_equal(ref.view(np.uint64)[~nan], got.view(np.uint64)[~nan]), (key, got, ref)
    finally:
        svo.close()


@pytest.mark.gpu
def test_fixture_records_are_bit_identical_to_the_recorded_oracle_results(pkg, cases):
    check(pkg, cases)


@pytest.mark.gpu
def test_library_built_with_the_scalar_routine_gives_the_same_bytes(pkg, cases):
    """A/B: with SVO_LIB_PATH pointing at a build of the library with -DEO_GN_SCALAR (the routine before the columns went to the
    lanes) the probe gives the recorded bytes too.  Without such a build there is nothing to compare."""
    own = os.path.join(ROOT, "stereo-semantic-vo_amd", "libsvo_hip.so")
    other = os.environ.get("SVO_LIB_PATH")
    if not other or os.path.realpath(other) == os.path.realpath(own):
        pytest.skip("SVO_LIB_PATH does not point at another build of the library")
    assert os.path.realpath(pkg.LIB_PATH) == os.path.realpath(other)
    check(pkg, cases)
