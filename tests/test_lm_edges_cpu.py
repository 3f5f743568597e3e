"""The pose-only LM at its edges, the part that needs no GPU: the fixture tests/golden/lm_edge_cases.npz (tools/make_lm_edge_cases.py)
reproduces on the CPU restatement (oracle/orc_pose.c), holds every path it was made for - proven from the restatement's own
statistics and branch counters (orc_pose_last_counts) -, and the restatement agrees on it with the independent numpy twin of
tests/golden/make_golden.py.

Why the fixture exists: the seeded problems of tests/test_gpu_parity.py (test_pose_opt_against_oracle and the matrix-core twin of it)
take ONE trial per iteration from both of their starts - the last test here states that -, so the retry loop of pose_opt_block
(lambda *= ni; ni *= 2, the solve's x kept, est0 kept while the trial estimate moves, the stop on ten rejections) had one witness,
the golden case lm2, compared with tolerances.  These cases are not duplicates of those."""
import os
import sys

import numpy as np
import pytest

import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_lm_edge_cases as mk             # noqa: E402


@pytest.fixture(scope="module")
def cases():
    return mk.unpack(np.load(mk.PATH))


def test_fixture_reproduces_on_the_restatement(cases, orc):
    """Bit for bit where the LM stays on the fixed series (and in the depth-zero cases, NaN for NaN); where a step takes libm's
    sin / cos, to 1e-12 (the same libm gives the same bits, another one its last-bit differences)."""
    assert os.path.getsize(mk.PATH) <= mk.MAX_BYTES
    for c in cases:
        w = mk.walk(orc, c["Xw"], c["obs"], c["K"], c["T0"])
        key = c["tag"]
        assert np.array_equal(w["stats_i"], c["stats_i"]) and np.array_equal(w["trials"], c["trials"]), key
        assert w["stop"] == c["stop"] and w["failed_solves"] == c["failed_solves"] and np.array_equal(w["counts"], c["counts"]), key
        if c["kind"] == mk.LARGE_ROTATION:
            assert np.abs(w["T"] - c["T"]).max() < 1e-12 and np.allclose(w["stats_f"], c["stats_f"], rtol=1e-12, atol=0), key
        else:
            for k in ("T", "stats_f"):
                a, b = np.ascontiguousarray(w[k]), np.ascontiguousarray(c[k])
                nan = np.isnan(b)
                assert np.array_equal(nan, np.isnan(a)) and np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan]), (key, k)


def test_fixture_holds_every_path_it_was_made_for(cases):
    """At least two cases each (from the restatement's trials per iteration, stop reason and counters): 2, 3..5, 6..9 trials in one
    iteration; the stops on qmax == 10, on nBad >= 3, on rho == 0 from exact dyadic data (1 iteration, 1 trial, chi2 0); ten
    iterations without termination; a restart with theta < 1e-5; starts turned by +-170 degrees with the largest diagonal 0 / 1 / 2
    (trace below -0.9) and at least one q.w < 0 flip; every edge on Huber's linear branch; a fifth of the points behind the camera;
    n = 2, 3, 127, 128, 129, 192, 193, 256, 320, 321; none of these on libm and none beyond 64 edges without need; three
    large-rotation cases on libm with the twin's distance recorded; the two depth-zero cases."""
    figures = mk.coverage(cases)
    print(figures)
    zero = [c for c in cases if c["kind"] == mk.DEPTH_ZERO]
    print([(c["tag"], c["stats_i"].tolist(), c["stats_f"].tolist(), int(c["failed_solves"]), float(np.abs(c["T"] - c["T0"]).max())) for c in zero])
    centre = [c for c in zero if c["tag"] == "depth zero centre"][0]
    # what the restatement does with 0 / 0: every solve fails (NaN in H), every trial is rejected with DBL_MAX, the pose stays
    assert centre["stats_i"].tolist() == [16, 10, 10, 0] and centre["failed_solves"] == 10
    assert np.abs(centre["T"] - centre["T0"]).max() < 1e-15


def test_restatement_agrees_with_the_numpy_twin(cases, orc):
    """On every finite case, with the tolerances of test_oracle_golden.test_lm_trace (make_lm_edge_cases.twin_difference): the same
    branch sequence, lambda / chi2 / rho of every trial to 1e-7, the pose to 1e-8, chi2 to 1e-10 at the start and 1e-7 at the end."""
    for c in cases:
        if c["kind"] == mk.DEPTH_ZERO:
            continue
        same, dT, dchi = mk.twin_difference(c["Xw"], c["obs"], c["K"], c["T0"], mk.walk(orc, c["Xw"], c["obs"], c["K"], c["T0"]))
        assert same, (c["tag"], dT, dchi)


def test_the_seeded_parity_problems_take_one_trial_per_iteration(orc):
    """test_pose_opt_against_oracle's and test_pose_opt_matrix_core_sums_equal_the_one_lane_loop's problems, from each of their
    starts: never a second trial in an iteration (a rejection only with rho == 0, which leaves the loop)."""
    plain = [(7, 500), (8, 37), (9, 5), (10, 1), (11, 512), (12, 64), (13, 65), (14, 63), (15, 257), (16, 700)]
    mfma = [(7, 500), (8, 37), (9, 5), (10, 1), (11, 512), (17, 130)]
    for seed, n, frac, starts in [(s, n, 0.2, 2) for s, n in plain] + [(s, n, 0.3, 1) for s, n in mfma]:
        Xw, obs, K, T_true = util.pose_problem(seed, n=n, outlier_frac=frac)
        for T0 in (np.eye(4), T_true)[:starts]:
            _, st, trace = orc.pose_opt(Xw, obs, K, T0)
            assert st.trials_total == st.iterations == len(trace), (seed, n)
