"""RANSAC's stopping rule and consensus count on the device, through the probes svo_debug_pnp_rule and svo_debug_pnp_consensus.

The rule - RANSACPointSetRegistrator::run's loop around RANSACUpdateNumIters - is one walker (pnp_walk, svo_pose_dev.h) with these
instantiations: the plain pnp_select of svo_pnp_ransac (bound from pnp_update_iters), and what the tracker runs: pnp_update_terms
(tabulated per frame, then looked up), pnp_select_pre (bound from those terms), the same walk cut at the first m samples (the fused
tail's early decision), pnp_bound_after (the bound after m samples).  All of them stand on the device's pow / log where the
CPU restatement stands on glibc's; tests/test_pnp_rule_cpu.py shows that the integers behind them have a relative margin of
3.9e-7, so a correct device math library must give the restatement's integers on EVERY pair (g, n) - the table test - and the
instantiations must agree with the reference loop (tests/pnp_rule_ref.py) on every vector of samples.

The consensus count (pnp_consensus_wave, the function every sample kernel counts with: pnp_inlier + the wave's sum over e = lane,
lane + 64, ...) is placed on its threshold on purpose: identity
rotation, a dyadic camera and dyadic points make the projection exact, so err == 64.0f and its float32 neighbours are met
exactly."""
import numpy as np
import pytest

import pnp_rule_ref as ref

pytestmark = pytest.mark.gpu
K_DYADIC = np.array([512.0, 512.0, 320.0, 240.0])


@pytest.fixture(scope="module")
def svo(pkg):
    s = pkg.Svo(640, 240, max_batch=1)
    yield s
    s.close()


# ---- the table: every pair 5 <= g <= n, 6 <= n <= 512, one launch per n ------------------------------------------------------------
@pytest.fixture(scope="module")
def table(svo):
    ld, r, it100, n_all, g_all, logs = [], [], [], [], [], set()
    for n in ref.NS_ALL:
        d, ri, ii, l001 = svo.debug_pnp_rule_table(n)
        assert not d[:5].any() and not ri[:5].any() and not ii[:5].any()
        ld.append(d[5:]); r.append(ri[5:]); it100.append(ii[5:]); logs.add(l001)
        n_all.append(np.full(n - 4, n)); g_all.append(np.arange(5, n + 1))
    return {"ld": np.concatenate(ld), "r": np.concatenate(r), "it100": np.concatenate(it100), "n": np.concatenate(n_all),
            "g": np.concatenate(g_all), "logs": logs}


def test_table_integers_equal_the_restatements(table, orc):
    g, n, ld, r = table["g"], table["n"], table["ld"], table["r"]
    assert len(g) == 129285 and len(table["logs"]) == 1
    num = table["logs"].pop()
    assert abs(num - np.log(0.01)) < 1e-15 * abs(num) * 4          # log(1 - 0.99): 1 - 0.99 is not 0.01 to the last bit, hence not ==
    ep = (n - g) / n
    # pnp_update_iters(ep, 100)
    assert np.array_equal(table["it100"], orc.ransac_update_num_iters_batch(ep, 100))
    # r = rint(log(0.01) / ld): the restatement's rounded quotient wherever ANY maxIters <= 100 can return it; beyond that only "above
    # 100" (up there ld = log(1 - 1e-10) moves by 1e-5 relative with the last bit of pow, and the quotient with it: the rule never
    # reads it, the comparison in front returns maxIters)
    raw = orc.ransac_update_num_iters_batch(ep, ref.INT_MAX)
    small = raw <= 100
    assert np.array_equal(r[small], raw[small]) and (r[~small] > 100).all()
    # ld == 1.0 marks "denominator below DBL_MIN": exactly where the restatement returns 0 (g == n)
    assert np.array_equal(ld == 1.0, raw == 0) and np.array_equal(raw == 0, g == n) and (ld[ld != 1.0] < 0).all()
    # the decision of pnp_walk<PREPARED> with the device's ld and log(0.01), for every bound it can be asked with
    for niters in range(1, 101):
        dec = np.where((ld >= 0) | (-num >= niters * (-ld)), niters, r)
        dec = np.where(ld == 1.0, 0, dec)
        assert np.array_equal(dec, orc.ransac_update_num_iters_batch(ep, niters)), niters
    # how far the device's log(1 - (g / n)^5) is from glibc's, in ulps (not bounded: where (g / n)^5 is tiny a last-bit difference of
    # pow moves 1 - pow by one ulp of 1.0 and the logarithm of that by 1e-5 relative)
    fin = ld != 1.0
    ref_ld = orc.ransac_log_denom_batch(ep[fin])
    ulps = np.abs(ld[fin].view(np.int64) - ref_ld.view(np.int64))
    worst = int(np.argmax(ulps))
    print("ld: largest distance %d ulp at (g, n) = (%d, %d); %d of %d pairs differ, %d by more than 1 ulp" %
          (ulps[worst], g[fin][worst], n[fin][worst], int((ulps > 0).sum()), int(fin.sum()), int((ulps > 1).sum())))


# ---- the rule on vectors of samples --------------------------------------------------------------------------------------------------
def check_vectors(svo, orc, names, cnt, ok, n):
    out = svo.debug_pnp_rule(cnt, ok, n)
    m = np.arange(101)
    for i in range(len(n)):
        best, good, iters, bounds = ref.run_rule(cnt[i], ok[i], int(n[i]), orc.ransac_update_num_iters)
        key = (names[i] if names else i, int(n[i]))
        sel = tuple(out["select"][i])
        assert sel == (best, good, iters), (key, sel, (best, good, iters))                     # pnp_select = the reference loop
        assert tuple(out["select_pre"][i]) == sel, key                                          # pnp_select_pre = pnp_select
        per = out["per_m"][i]
        assert np.array_equal(per[:, 0], np.where(iters <= m, iters, m + 1)), key               # the walk cut at m: samples visited, or m + 1
        assert np.array_equal(per[:, 1], per[:, 0]), key                                        # (its second column: the same value)
        ended = per[:, 0] <= m
        assert (per[ended, 2] == best).all() and (per[ended, 3] == good).all(), key             # ... and pnp_select's winner where it ended
        assert np.array_equal(per[:, 4], np.array(bounds)), key                                 # pnp_bound_after(m)
        # ... and it never cuts off a sample the rule visits: before the rule has ended (m < iters) it is at least iters.  (Once the
        # rule has ended it may be lower - 0 after a full consensus -: the samples from m on are the ones it then excludes.)
        assert (per[:iters, 4] >= iters).all() and (np.maximum(per[:, 4], m) >= iters).all(), key


def test_rule_on_hand_made_vectors(svo, orc):
    vecs = ref.hand_made(orc.ransac_update_num_iters)
    check_vectors(svo, orc, [v[0] for v in vecs], np.stack([v[1] for v in vecs]), np.stack([v[2] for v in vecs]), np.array([v[3] for v in vecs], np.int32))


def test_rule_on_seeded_vectors(svo, orc):
    cnt, ok, n = ref.seeded()
    for a in range(0, len(n), 500):
        check_vectors(svo, orc, None, cnt[a:a + 500], ok[a:a + 500], n[a:a + 500])


# ---- the consensus count -------------------------------------------------------------------------------------------------------------
def at_pixel(u, v, z=2.0):
    """the point that projects exactly to (u, v) under the identity pose and the dyadic camera (u, v multiples of 2^-30 or so)"""
    return [(u - K_DYADIC[2]) / K_DYADIC[0] * z, (v - K_DYADIC[3]) / K_DYADIC[1] * z, z]


def consensus(svo, Xw, obs):
    Xw = np.array(Xw, np.float64); obs = np.array(obs, np.float64)
    want = ref.inlier_flags(Xw, obs, K_DYADIC, np.eye(3), np.zeros(3))
    cnt, flags = svo.debug_pnp_consensus(Xw, obs, K_DYADIC, np.eye(3), np.zeros(3))
    assert np.array_equal(flags, want) and cnt == int(want.sum()), (cnt, flags.tolist(), want.tolist())
    return want


def test_consensus_threshold_on_purpose(svo):
    up = float(np.nextafter(np.float32(8.0), np.float32(9.0)))        # the next float32 above 8
    X, o = [], []
    # an offset of exactly 8 px (err == 64.0f: an inlier), the next float32 above (an outlier); the projection is the pixel (0, 0)
    X += [at_pixel(0, 0)] * 4; o += [(8.0, 0.0), (up, 0.0), (0.0, -8.0), (0.0, -up)]
    # the same split over dx and dy: dy = 4, dx the float32 pair around sqrt(48) whose rounded sum of squares is 64.0f / the next above
    dx = np.float32(np.sqrt(48.0))
    err = lambda a: np.float32(np.float32(a * a) + np.float32(16.0))
    while err(dx) > np.float32(64.0):
        dx = np.nextafter(dx, np.float32(0))
    while err(np.nextafter(dx, np.float32(9))) <= np.float32(64.0):
        dx = np.nextafter(dx, np.float32(9))
    X += [at_pixel(0, 0)] * 2; o += [(float(dx), 4.0), (float(np.nextafter(dx, np.float32(9))), 4.0)]
    # a projection whose double value lies between the float32 neighbours 8 and 8 + 2^-20, on either side of their midpoint: rounded
    # once to float it is 8 (inlier) or the next float32 (outlier); the observation is the pixel (0, 0)
    X += [at_pixel(8 + 2.0 ** -21 - 2.0 ** -40, 0, 1.0), at_pixel(8 + 2.0 ** -21 + 2.0 ** -40, 0, 1.0)]; o += [(0.0, 0.0)] * 2
    # z == 0: projected with scale 1 - x, y themselves go through the camera matrix
    X += [[(8.0 - 320) / 512, -240.0 / 512, 0.0], [(up - 320) / 512, -240.0 / 512, 0.0]]; o += [(0.0, 0.0)] * 2
    # z < 0: the division goes through - the point lands mirrored through the principal point
    X += [[0.25, 0.125, -2.0], [0.25, 0.125, -2.0]]; o += [(320 - 64.0, 240 - 32.0 + 8.0), (320 + 64.0, 240 + 32.0)]
    want = consensus(svo, X, o)
    assert want.tolist() == [1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0]      # (the numpy twin itself lands where the cases were aimed)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 511, 512])
def test_consensus_lane_strides(svo, n):
    """n around the wave's width and at the capacity: inliers at the first and last index of every lane stride (lane 0 and lane 63 of
    every pass, and the last point), each exactly on the threshold; everything else 100 px off."""
    rng = np.random.default_rng(n)
    uv = np.stack([rng.integers(0, 640, n), rng.integers(0, 480, n)], 1).astype(np.float64)
    X = [at_pixel(u, v, float(2 ** rng.integers(0, 5))) for u, v in uv]
    inl = sorted({e for e in list(range(0, n, 64)) + list(range(63, n, 64)) + [n - 1]})
    obs = uv + [100.0, 0.0]
    obs[inl] = uv[inl] + [0.0, 8.0]
    want = consensus(svo, X, obs)
    assert np.flatnonzero(want).tolist() == inl
