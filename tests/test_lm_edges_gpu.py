"""The pose-only LM at its edges on the device (svo_pose_opt, all three "pose_mfma" modes) against tests/golden/lm_edge_cases.npz
(tools/make_lm_edge_cases.py; what the fixture holds and why: tests/test_lm_edges_cpu.py): the retry loop with 2 .. 10 trials, every
stopping rule, the theta < 1e-5 and "largest diagonal" branches, Huber's linear branch on every edge, points behind the camera,
n = 2, 3 and the chunk boundaries of build_system_ordered - bit for bit -, starts whose steps take libm's sin / cos - within the
distance the numpy twin keeps from the restatement -, and a depth of exactly zero - the pose stays."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_lm_edge_cases as mk             # noqa: E402

pytestmark = pytest.mark.gpu
CASES = mk.unpack(np.load(mk.PATH))
MODES = (1, 2, 0)       # the sums over the edges on the matrix core, one lane per quantity, the whole loop by one lane


def lm_bits(T, stats_i, stats_f):
    """everything the LM leaves behind, as bits (test_gpu_parity.lm_bits on the fixture's arrays)"""
    return (np.ascontiguousarray(T, np.float64).tobytes(), tuple(int(v) for v in stats_i), np.ascontiguousarray(stats_f, np.float64).tobytes())


def run(svo, c):
    T, st = svo.pose_opt(c["Xw"], c["obs"], c["K"], c["T0"])
    return T, np.array([st.n_edges, st.iterations, st.trials_total, st.terminated], np.int32), np.array([st.chi2_initial, st.chi2_final, st.lambda_final])


@pytest.fixture(scope="module")
def svo_modes(pkg):
    ctx = {}
    for mode in MODES:
        ctx[mode] = pkg.Svo(640, 240, max_batch=1)
        ctx[mode].set_option("pose_mfma", mode)
    yield ctx
    for s in ctx.values():
        s.close()


@pytest.mark.parametrize("mode", MODES)
def test_bitwise_cases(svo_modes, mode):
    """lm_bits - pose, counters, chi2 at both ends, lambda - equal to the restatement's on every case that stays off libm."""
    bad = []
    for i, c in enumerate(CASES):
        if c["kind"] != mk.BITWISE:
            continue
        T, si, sf = run(svo_modes[mode], c)
        if lm_bits(T, si, sf) != lm_bits(c["T"], c["stats_i"], c["stats_f"]):
            bad.append((i, c["tag"], len(c["Xw"]), si.tolist(), c["stats_i"].tolist(), float(np.abs(T - c["T"]).max()), (sf - c["stats_f"]).tolist()))
    assert not bad, bad


def test_large_rotation_cases(svo_modes):
    """A step of 0.5 rad or more takes sin / cos from the device's math library where the restatement takes glibc's: pose and final
    chi2 within 10 x the distance the numpy twin (numpy's sin / cos) keeps from the restatement on the same case, at least 1e-12 -
    both distances are the rounding of sin / cos, and the margin covers that the two need not be equal.  The three modes agree
    with each other bit for bit."""
    for c in CASES:
        if c["kind"] != mk.LARGE_ROTATION:
            continue
        got = {mode: run(svo_modes[mode], c) for mode in MODES}
        T, si, sf = got[1]
        dT, dchi = float(np.abs(T - c["T"]).max()), float(abs(sf[1] - c["stats_f"][1]))
        print("large rotation: |dT| %.3e (twin %.3e), |dchi2| %.3e (twin %.3e)" % (dT, c["twin_dT"], dchi, c["twin_dchi"]))
        assert np.array_equal(si, c["stats_i"])
        assert dT <= max(10 * c["twin_dT"], 1e-12) and dchi <= max(10 * c["twin_dchi"], 1e-12), (dT, dchi)
        for mode in MODES[1:]:
            assert lm_bits(*got[mode]) == lm_bits(*got[1]), mode


@pytest.mark.parametrize("mode", MODES)
def test_depth_zero_keeps_the_pose(svo_modes, mode):
    """A point at depth exactly 0 under the start pose (0 / 0 at the camera centre, 1 / 0 beside it): what the comment at edge_error
    promises and no more - the pose comes back as the restatement's (within 1e-12), the counters stay in their ranges.  (No address
    and no loop bound of pose_opt_block depends on the data, only on n.)  What the statistics are: DESIGN.md."""
    for c in CASES:
        if c["kind"] != mk.DEPTH_ZERO:
            continue
        T, si, sf = run(svo_modes[mode], c)
        print(c["tag"], "device", si.tolist(), sf.tolist(), "restatement", c["stats_i"].tolist(), c["stats_f"].tolist())
        assert np.abs(T - c["T"]).max() < 1e-12, c["tag"]
        assert si[0] == len(c["Xw"]) and si[1] <= 10 and si[2] <= 100, c["tag"]
