"""The 12 x 12 step loop of the order-preserving EPnP on the device, alone: svo_debug_jacobi12 - one launch of one wave, jacobi_rows<12>
(csrc/svo_epnp_ord_dev.h, block EO_JACOBI_ASM_12) on a given matrix - reproduces what JacobiSVDImpl_'s sequential sweeps make of every
matrix of tests/golden/jacobi12_cases.npy (tools/make_jacobi12_cases.py; what the groups are there for: tests/test_jacobi12_resched_cpu.py):
the rows scaled by 1 / W, W and the number of steps, bit for bit.  Group g (a NaN; a singular value below 2^-100) is outside the
range in which the loop's unscaled divisions are IEEE's: there the probe must report what the solver acts on - the flag, or a W
outside [2^-100, 2^100]."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def cases():
    return np.load(os.path.join(ROOT, "tests", "golden", "jacobi12_cases.npy"))


def check(pkg, cases):
    import gen_jacobi_schedule
    _, pro, per = gen_jacobi_schedule.table(12, 12)
    svo = pkg.Svo(640, 240, max_batch=1)
    try:
        for i, c in enumerate(cases):
            key = (i, c["group"].decode())
            rows, w, steps, flag = svo.debug_jacobi12(c["At"])
            if c["group"] == b"g":
                in_range = bool(np.all((w >= 2.0 ** -100) & (w <= 2.0 ** 100)))      # (False for a NaN)
                assert flag == 1 or not in_range, key
                continue
            assert flag == 0, key
            assert steps == pro + per * int(c["sweeps"]), (key, steps, int(c["sweeps"]))
            assert np.array_equal(w.view(np.uint64), np.ascontiguousarray(c["W"]).view(np.uint64)), (key, w, c["W"])
            assert np.array_equal(rows.view(np.uint64), np.ascontiguousarray(c["rows"]).view(np.uint64)), key
    finally:
        svo.close()


@pytest.mark.gpu
def test_fixture_matrices_are_bit_identical_to_the_sequential_sweeps(pkg, cases):
    assert len(cases) >= 40 and set(cases["group"].tolist()) == set(b"a b c d e f g".split())
    check(pkg, cases)


@pytest.mark.gpu
def test_library_built_with_the_former_step_body_gives_the_same_bytes(pkg, cases):
    """A/B: with SVO_LIB_PATH pointing at a build of the library with -DEO_JACOBI12_PREV (the step body in its former instruction
    order) the probe gives the recorded bytes too.  Without such a build there is nothing to compare."""
    own = os.path.join(ROOT, "stereo-semantic-vo_amd", "libsvo_hip.so")
    other = os.environ.get("SVO_LIB_PATH")
    if not other or os.path.realpath(other) == os.path.realpath(own):
        pytest.skip("SVO_LIB_PATH does not point at another build of the library")
    assert os.path.realpath(pkg.LIB_PATH) == os.path.realpath(other)
    check(pkg, cases)
