"""RANSAC's stopping rule and consensus count, the part that needs no GPU: the references the device tests compare against
(tests/pnp_rule_ref.py) are themselves checked here.

RANSACUpdateNumIters ends in two discrete steps - the comparison -num >= maxIters * (-denom) and (int)rint(num / denom) - behind
pow and log, which the CPU restatement takes from libm and the device from its own math library.  The margin study shows that
they have room: over all 129,285 pairs 5 <= g <= n, 6 <= n <= 512 the exact quotient comes no closer than 5.0e-7 (relative) to a tie
of rint and 3.9e-7 to an integer bound, so ANY pow / log good to 1e-9 gives the same integers - and a device that does not is wrong."""
import numpy as np
import pytest

import pnp_rule_ref as ref
import util


@pytest.fixture(scope="module")
def study():
    pytest.importorskip("mpmath")
    return ref.margin_study()


def test_margins_are_the_recorded_ones_and_wide(study):
    rec = ref.load_margins()
    assert rec["pairs"] == len(study["g"]) == 129285 and rec["pairs_with_g_equal_n"] == int((study["g"] == study["n"]).sum()) == 507
    for key in ("tie", "cmp"):
        print(key, study[key])
        assert list(study[key][1][:2]) == rec[key]["at"][:2] and np.isclose(study[key][0], rec[key]["relative_margin"], rtol=1e-6)
        assert study[key][0] > 1e-9
    assert rec["tie"]["at"][:2] == [286, 357] and rec["cmp"]["at"] == [28, 51, 90]


def test_float64_integers_equal_the_200_bit_ones(study, orc):
    """The restatement's RANSACUpdateNumIters (glibc's pow / log) against the exact quotient, on every pair: for every maxIters
    1 .. 100, and the rounded quotient itself wherever it can be returned (<= 100)."""
    g, n, q, r = study["g"], study["n"], study["q"], study["r"]
    ep = (n - g) / n
    for niters in range(1, 101):
        got = orc.ransac_update_num_iters_batch(ep, niters)
        assert np.array_equal(got, ref.integers_from_quotient(q, r, niters)), niters
    raw = orc.ransac_update_num_iters_batch(ep, ref.INT_MAX)
    small = r <= 100
    assert np.array_equal(raw[small], r[small]) and (raw[~small] > 100).all()
    assert np.array_equal(raw == 0, g == n)
    assert orc.ransac_update_num_iters(ep[7], 100) == orc.ransac_update_num_iters_batch(ep[7:8], 100)[0]


def test_reference_loop_on_the_hand_made_vectors(orc):
    """run_rule does on each hand-made vector what the vector was made to show."""
    res = {name: (ref.run_rule(c, o, n, orc.ransac_update_num_iters), c, o, n) for name, c, o, n in ref.hand_made(orc.ransac_update_num_iters)}
    (best, good, iters, bounds), *_ = res["nothing ok"]
    assert (best, good, iters) == (-1, 0, 100) and bounds == [100] * 101
    (best, good, iters, _), c, o, n = res["a not-ok sample with the largest count"]
    assert best != 17 and good == max(c[k] for k in range(iters) if o[k]) < 60
    assert res["counts <= 4 only"][0][:3] == (-1, 0, 100)
    (best, good, iters, _), *_ = res["count 5 at n = 6"]
    assert (best, good) == (3, 5) and iters > 4
    assert res["equal counts: the earlier one stays"][0][0] == 2
    for k in (0, 1, 37, 99):
        (best, good, iters, bounds), *_ = res["g == n at sample %d" % k]
        assert (best, good, iters) == (k, 64, k + 1) and bounds[k + 1] == 0 and bounds[100] == 0
    assert res["n == 5, ok"][0][:3] == (0, 5, 1) and res["n == 5, not ok"][0][:3] == (-1, 0, 1)
    visited = [v for k, v in res.items() if k.endswith("(visited)")][0]
    skipped = [v for k, v in res.items() if k.endswith("(not visited)")][0]
    assert visited[0][0] == visited[0][2] - 1 and visited[0][1] == 50 and skipped[0][:2] == (0, 40) and skipped[0][2] == skipped[0][3][1]
    assert len(res) == 15


def test_seeded_vectors_reach_the_rule_from_many_sides(orc):
    cnt, ok, n = ref.seeded()
    assert len(n) == 2000 and set(n.tolist()) == {6, 7, 51, 64, 357, 512}
    iters = np.array([ref.run_rule(cnt[i], ok[i], int(n[i]), orc.ransac_update_num_iters)[2] for i in range(0, 2000, 5)])
    assert (iters == 100).sum() > 20 and (iters < 10).sum() > 20 and ((iters > 10) & (iters < 100)).sum() > 20


@pytest.mark.parametrize("seed,n,outliers", [(7, 500, 0.2), (21, 200, 0.5)])
def test_inlier_twin_equals_the_restatements_mask(orc, seed, n, outliers):
    """PnPRansacCallback::computeError with explicit float32 steps in numpy against the mask of one seeded cv::solvePnPRansac run of
    the restatement (the pose it returns is the winner's rotation as its consensus was counted with)."""
    Xw, obs, K, _ = util.pose_problem(seed, n=n, outlier_frac=outliers)
    T, mask, st = orc.pnp_ransac(Xw, obs, K, np.eye(4))
    flags = ref.inlier_flags(Xw, obs, K, T[:3, :3], T[:3, 3])
    assert st.ok and 0 < mask.sum() < n and np.array_equal(flags, mask) and flags.sum() == st.n_inliers
