"""Named, seeded cases of loop verification for tests/test_loop_cpu.py and tests/test_loop_gpu.py.  A builder returns a dict
(scene, pairs, P, and for the solver cases match); its `prove` checks on the twin's intermediates that the case reaches the edge
it is named after."""
import math

import numpy as np

import loop_ref as R

CAM = dict(fx=718.856, fy=718.856, cx=607.1928, cy=185.2157)


# ---- building blocks ----------------------------------------------------------------------------------------------------------------
def scene(F, S, So=None):
    So = So or S
    kp = np.zeros((F, S), R.KP)
    kp["class_id"] = -1
    return dict(desc=np.zeros((F, S, 32), np.uint8), kp=kp, n=np.zeros(F, np.int32), fv=np.zeros((F, S), R.FEATURE),
                fv_n=np.zeros(F, np.int32), obs=np.zeros((F, So), R.MAP_OBS), obs_n=np.zeros(F, np.int32),
                Tcw=np.tile(np.eye(4, dtype=np.float32).ravel(), (F, 1)))


def flip(d, bits):
    """a copy of descriptor d with the listed bit positions (0 .. 255) flipped"""
    d = d.copy()
    for b in bits:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def set_fv(sc, f, nodes):
    """nodes[i]: the node of feature i, or -1 for a feature outside the FeatureVector"""
    pairs = sorted((int(nd), i) for i, nd in enumerate(nodes) if nd >= 0)
    sc["fv_n"][f] = len(pairs)
    for p, (nd, i) in enumerate(pairs):
        sc["fv"][f][p] = (nd, i)


def set_obs(sc, f, kps, X):
    kps = np.asarray(kps, np.int64)
    order = np.argsort(kps, kind="stable")
    sc["obs_n"][f] = len(kps)
    for p, j in enumerate(order):
        o = sc["obs"][f][p]
        o["gid"], o["kp"], o["depth"] = 1000 * f + p, kps[j], 1.0
        o["X"], o["Y"], o["Z"] = X[j]
        o["u"], o["v"] = sc["kp"][f][kps[j]]["x"], sc["kp"][f][kps[j]]["y"]


def rot_axis(axis, deg):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    a = math.radians(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)


def pose(Rm, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rm, t
    return T


def to_world(Tcw32, Xc):
    """world positions (float32) that the float32 pose takes to about Xc"""
    T = Tcw32.astype(np.float64).reshape(4, 4)
    return ((Xc - T[:3, 3]) @ T[:3, :3]).astype(np.float32)


def project(Xc):
    return np.stack([CAM["fx"] * Xc[:, 0] / Xc[:, 2] + CAM["cx"], CAM["fy"] * Xc[:, 1] / Xc[:, 2] + CAM["cy"]], 1)


# ---- matching: planted frames -------------------------------------------------------------------------------------------------------
# (features of the node in a, in b): 0, 1, 2, 63, 64, 65 and 130 on either side, a node in only one frame
SIZES = [(130, 65), (65, 130), (64, 63), (63, 64), (2, 1), (1, 2), (1, 0), (0, 1), (64, 64), (2, 2), (0, 2), (2, 0)]


def planted(seed, sizes=SIZES, S=None, frac_mp=0.8, noise=24, rot=45.0, T12=None, n_pairs=1, pad=8, geometry=True, stop=0.0):
    """n_pairs pairs of frames (2 p, 2 p + 1).  Per node min(sA, sB) features are noisy copies of one another (up to `noise` bits),
    the rest is random; a copy's angle differs by about `rot`; frac_mp of the keypoints have a map point; a share `stop` of the
    features is left out of the FeatureVector (stop words), so with stop = 0 the node sizes are exactly `sizes`.  With geometry the
    shared features see one 3-D point, b's camera coordinates taken to a's by T12."""
    rng = np.random.default_rng(seed)
    nA, nB = sum(s[0] for s in sizes), sum(s[1] for s in sizes)
    S = S or max(nA, nB) + pad
    sc = scene(2 * n_pairs, S)
    if T12 is None:
        T12 = pose(rot_axis([0.1, 1.0, 0.05], 20.0), [0.5, -0.1, 1.0])
    for p in range(n_pairs):
        fa, fb = 2 * p, 2 * p + 1
        Ta = pose(rot_axis(rng.normal(size=3), rng.uniform(0, 180)), rng.uniform(-5, 5, 3)).astype(np.float32)
        Tb = pose(rot_axis(rng.normal(size=3), rng.uniform(0, 180)), rng.uniform(-5, 5, 3)).astype(np.float32)
        sc["Tcw"][fa], sc["Tcw"][fb] = Ta.ravel(), Tb.ravel()
        permA, permB = rng.permutation(nA), rng.permutation(nB)
        nodesA, nodesB = np.zeros(nA, np.int64), np.zeros(nB, np.int64)
        XcA, XcB = np.zeros((nA, 3)), np.zeros((nB, 3))
        ia = ib = 0
        for k, (sA, sB) in enumerate(sizes):
            node = 10 + 3 * k
            shared = min(sA, sB)
            base = rng.integers(0, 256, (max(sA, sB), 32), dtype=np.uint8)
            ang = rng.uniform(0, 360, max(sA, sB))
            Xb = np.stack([rng.uniform(-8, 8, max(sA, sB)), rng.uniform(-3, 3, max(sA, sB)), rng.uniform(6, 30, max(sA, sB))], 1)
            for j in range(sA):
                i = permA[ia]; ia += 1
                nodesA[i] = node
                sc["desc"][fa][i] = flip(base[j], rng.choice(256, rng.integers(0, noise + 1), replace=False)) if j < shared else \
                    rng.integers(0, 256, 32, dtype=np.uint8)
                sc["kp"][fa][i]["angle"] = ang[j] if j < shared else rng.uniform(0, 360)
                sc["kp"][fa][i]["octave"] = rng.integers(0, 8)
                XcA[i] = T12[:3, :3] @ Xb[j] + T12[:3, 3] if j < shared else [rng.uniform(-8, 8), rng.uniform(-3, 3), rng.uniform(6, 30)]
            for j in range(sB):
                i = permB[ib]; ib += 1
                nodesB[i] = node
                sc["desc"][fb][i] = flip(base[j], rng.choice(256, rng.integers(0, noise + 1), replace=False))
                sc["kp"][fb][i]["angle"] = (ang[j] - rot + rng.uniform(-10, 10)) % 360.0 if rng.random() < 0.8 else rng.uniform(0, 360)
                sc["kp"][fb][i]["octave"] = rng.integers(0, 8)
                XcB[i] = Xb[j]
        for f, n, nodes, Xc, T in ((fa, nA, nodesA, XcA, Ta), (fb, nB, nodesB, XcB, Tb)):
            sc["n"][f] = n
            uv = project(Xc)
            sc["kp"][f]["x"][:n], sc["kp"][f]["y"][:n] = uv[:, 0], uv[:, 1]
            out = rng.random(n) < stop            # features the vocabulary stopped
            set_fv(sc, f, np.where(out, -1, nodes))
            kps = np.flatnonzero(rng.random(n) < frac_mp)
            set_obs(sc, f, kps, to_world(T, Xc[kps]) if geometry else rng.normal(size=(len(kps), 3)).astype(np.float32))
    pairs = np.array([(2 * p, 2 * p + 1) for p in range(n_pairs)], np.int32)
    return dict(scene=sc, pairs=pairs, P=R.params(), T12=T12)


def prove_planted(case):
    """exactly the node sizes of SIZES are walked - 1, 2, 63, 64, 65 and 130 features on either side -, nodes in one frame only
    exist (the 0 sizes), and matches come out"""
    sc = case["scene"]
    m, n, info = R.match_pair(sc, 0, 1, case["P"])
    seen = sorted((a, b) for _, a, b in info["nodes"])
    assert seen == sorted(s for s in SIZES if s[0] and s[1]), seen
    for want in (1, 2, 63, 64, 65, 130):
        assert any(a == want for a, _ in seen) and any(b == want for _, b in seen), (want, seen)
    na, _ = R.node_runs(sc["fv"][0][:sc["fv_n"][0]])
    nb, _ = R.node_runs(sc["fv"][1][:sc["fv_n"][1]])
    assert len(set(na) - set(nb)) == sum(1 for a, b in SIZES if a and not b) > 0
    assert len(set(nb) - set(na)) == sum(1 for a, b in SIZES if b and not a) > 0
    assert n > 50 and (info["before"] >= 0).sum() > n      # the orientation check took some away
    return info


def root(seed, n):
    """one node - the root - holding every feature (Tracking's levelsup 4 on an L = 4 tree)"""
    c = planted(seed, sizes=[(n, n)], S=n, frac_mp=0.9, pad=0)
    for f in (0, 1):
        c["scene"]["fv"][f]["node"] = 0
    return c


def prove_root(case, n):
    sc = case["scene"]
    for f in (0, 1):      # every feature of either frame, in one node: n / 64 chunks on b's side, all of them live
        assert sc["n"][f] == sc["fv_n"][f] == n == sc["desc"].shape[1] and set(sc["fv"][f]["node"]) == {0}
        assert sorted(sc["fv"][f]["feature"]) == list(range(n))


# ---- matching: hand-made single-node frames ---------------------------------------------------------------------------------------
def micro(descA, descB, mpA=None, mpB=None, angA=None, angB=None, S=None, P=None, seed=0):
    """one node holding every feature of both frames; mp*: which keypoints have a map point (default all)"""
    nA, nB = len(descA), len(descB)
    S = S or max(nA, nB) + 3
    sc = scene(2, S)
    rng = np.random.default_rng(seed)
    for f, D, mp, ang in ((0, descA, mpA, angA), (1, descB, mpB, angB)):
        n = len(D)
        sc["n"][f] = n
        sc["desc"][f][:n] = np.array(D, np.uint8).reshape(n, 32)
        if ang is not None:
            sc["kp"][f]["angle"][:n] = ang
        set_fv(sc, f, [7] * n)
        kps = np.arange(n) if mp is None else np.flatnonzero(np.asarray(mp))
        set_obs(sc, f, kps, rng.normal(size=(len(kps), 3)).astype(np.float32) + [0, 0, 10])
    return dict(scene=sc, pairs=np.array([(0, 1)], np.int32), P=P or R.params(check_orientation=0))


def _far(rng, m):
    return [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(m)]


def _bits(k, start=0):
    return list(range(start, start + k))


def threshold_49_50():
    rng = np.random.default_rng(11)
    a = _far(rng, 2)
    return micro(a, [flip(a[0], _bits(49)), flip(a[1], _bits(50))])      # -> [0, -1]


def ratio_30_40():
    rng = np.random.default_rng(12)
    a = _far(rng, 1)
    return micro(a, [flip(a[0], _bits(30)), flip(a[0], _bits(40, 100))])      # 30 < 0.75f * 40 is false -> [-1]


def ratio_29_40():
    rng = np.random.default_rng(12)
    a = _far(rng, 1)
    return micro(a, [flip(a[0], _bits(40, 100)), flip(a[0], _bits(29))])      # -> [1]


def ratio_f32_edge():
    """best 33, second 50, nn_ratio 0.66: the float32 product is 33.000000 (not < ), the float64 one 33.00000131 (<)"""
    rng = np.random.default_rng(13)
    a = _far(rng, 1)
    assert not np.float32(33) < np.float32(np.float32(0.66) * np.float32(50)) and 33.0 < float(np.float32(0.66)) * 50.0
    return micro(a, [flip(a[0], _bits(33)), flip(a[0], _bits(50, 100))], P=R.params(check_orientation=0, nn_ratio=0.66))


def tied_best():
    rng = np.random.default_rng(14)
    a = _far(rng, 1)
    return micro(a, [flip(a[0], _bits(10)), flip(a[0], _bits(10, 100))])      # best1 = best2 = 10 -> [-1]


def compete(k):
    """k i1 with one descriptor, close to b's feature 1 (distance 5) and less so to feature 0 (distance 20): the first takes 1, the
    second then sees best 20 against ~128 and takes 0, a third finds only far ones"""
    rng = np.random.default_rng(15)
    d = _far(rng, 1)[0]
    return micro([d] * k, [flip(d, _bits(20)), flip(d, _bits(5, 100))] + _far(rng, 2))


def second_taken():
    """i1 = 0 takes b's 0; for i1 = 1, b's 0 (distance 12) is gone, so 1 (distance 14) stands against ~128 and is accepted; with
    matched2 ignored 14 would never win"""
    rng = np.random.default_rng(16)
    d = _far(rng, 1)[0]
    return micro([flip(d, _bits(2)), flip(d, _bits(12, 50))], [flip(d, _bits(0)), flip(d, _bits(12, 50) + _bits(14, 100))] + _far(rng, 1))


def no_mp_second():
    """b's feature 1 has no map point and lies at distance 12 of a's 0, feature 0 at 10: skipped, 10 stands against ~128"""
    rng = np.random.default_rng(17)
    a = _far(rng, 1)
    return micro(a, [flip(a[0], _bits(10)), flip(a[0], _bits(12, 100))] + _far(rng, 1), mpB=[1, 0, 1])


def no_map_points(which):
    rng = np.random.default_rng(18)
    a = _far(rng, 6)
    c = micro(a, [flip(x, _bits(3)) for x in a])
    for f in which:
        c["scene"]["obs_n"][f] = 0
    return c


def _identity_frames(n, seed):
    rng = np.random.default_rng(seed)
    a = _far(rng, n)
    return a, [flip(x, _bits(1)) for x in a]


def angles(diffs, seed=19, **kw):
    """feature i of a matches feature i of b, its angle ahead by diffs[i] degrees"""
    n = len(diffs)
    a, b = _identity_frames(n, seed)
    angB = np.full(n, 0.0, np.float32)
    return micro(a, b, angA=np.asarray(diffs, np.float32), angB=angB, P=R.params(**kw))


def half_bins():
    """differences of exactly 15 (x = 0.5 -> bin 1, to even: 0) and 45 (1.5 -> 2), 359.9 (-> 12): bins 1: 3, 2: 2, 12: 2, 0: 1"""
    return angles([15, 15, 15, 45, 45, 359.9, 359.9, 1.0])


def wrap_30():
    """a difference of 900 degrees is bin 30 -> 0, where it joins three others; bins 3, 4, 5 hold two each"""
    return angles([900, 2, 3, 4, 90, 91, 120, 121, 150, 151])


def maxima_ties():
    """bins 1, 2, 3, 4 hold two matches each: the three earlier ones stay"""
    return angles([30, 31, 60, 61, 90, 91, 120, 121])


def tenth():
    """bin 1 holds ten, bin 3 one: (float)1 < 0.1f * (float)10 = 1.0f is false, the second stays; bin 5 holds none"""
    return angles([30] * 10 + [90])


MATCH_MICRO = dict(threshold_49_50=(threshold_49_50, [0, -1]), ratio_30_40=(ratio_30_40, [-1]), ratio_29_40=(ratio_29_40, [1]),
                   ratio_f32_edge=(ratio_f32_edge, [-1]), tied_best=(tied_best, [-1]), compete2=(lambda: compete(2), [1, 0]),
                   compete3=(lambda: compete(3), [1, 0, -1]), second_taken=(second_taken, [0, 1]), no_mp_second=(no_mp_second, [0]),
                   no_mp_a=(lambda: no_map_points([0]), [-1] * 6), no_mp_both=(lambda: no_map_points([0, 1]), [-1] * 6),
                   half_bins=(half_bins, [0, 1, 2, 3, 4, 5, 6, -1]), wrap_30=(wrap_30, [0, 1, 2, 3, 4, 5, 6, 7, -1, -1]),
                   maxima_ties=(maxima_ties, [0, 1, 2, 3, 4, 5, -1, -1]), tenth=(tenth, list(range(11))))


def prove_micro(name):
    """the twin gives the hand-computed matches"""
    build, want = MATCH_MICRO[name]
    c = build()
    m, n, info = R.match_pair(c["scene"], 0, 1, c["P"])
    assert list(m[:len(want)]) == want and n == sum(w >= 0 for w in want), (name, m, info["log"], info["hist"])
    return c


# ---- the solver ------------------------------------------------------------------------------------------------------------------------
def solve_case(seed, N, n_out=0, rot_deg=30.0, axis=(0.2, 1.0, 0.1), t12=(0.4, -0.2, 0.8), P=None, n_pairs=1, extra=3, identity=False,
               octaves=None, behind=0, zero_z=0):
    """n_pairs pairs of frames with N matched keypoints each: b's points taken to a's camera by the planted T12, n_out of them
    replaced by gross outliers; `behind` of the outliers stand behind a's camera and `zero_z` have z = 0 in b's (needs identity
    poses, where the world is the camera)."""
    rng = np.random.default_rng(seed)
    S = N + extra
    sc = scene(2 * n_pairs, S)
    T12 = pose(rot_axis(axis, rot_deg), t12)
    match = np.full((n_pairs, S), -1, np.int32)
    for p in range(n_pairs):
        fa, fb = 2 * p, 2 * p + 1
        if not identity:
            sc["Tcw"][fa] = pose(rot_axis(rng.normal(size=3), rng.uniform(0, 180)), rng.uniform(-5, 5, 3)).astype(np.float32).ravel()
            sc["Tcw"][fb] = pose(rot_axis(rng.normal(size=3), rng.uniform(0, 180)), rng.uniform(-5, 5, 3)).astype(np.float32).ravel()
        Xb = np.stack([rng.uniform(-4, 4, S), rng.uniform(-3, 3, S), rng.uniform(8, 30, S)], 1)
        Xa = Xb @ T12[:3, :3].T + T12[:3, 3]
        out = rng.choice(N, n_out, replace=False) if n_out else np.zeros(0, np.int64)
        Xa[out] += rng.choice([-1, 1], (len(out), 3)) * rng.uniform(1.0, 3.0, (len(out), 3))
        for j in out[:behind]:
            Xa[j, 2] = -abs(Xa[j, 2])
        for j in out[behind:behind + zero_z]:
            Xb[j, 2] = 0.0
        perm = rng.permutation(S)                 # keypoint i of a <-> keypoint perm[i] of b
        sc["n"][fa] = sc["n"][fb] = S
        match[p, :N] = perm[:N]
        sc["kp"][fa]["octave"] = rng.integers(0, 8, S) if octaves is None else octaves[0]
        sc["kp"][fb]["octave"] = rng.integers(0, 8, S) if octaves is None else octaves[1]
        with np.errstate(all="ignore"):
            uva, uvb = project(Xa), project(Xb)
        sc["kp"][fa]["x"], sc["kp"][fa]["y"] = uva[:, 0], uva[:, 1]
        sc["kp"][fb]["x"][perm], sc["kp"][fb]["y"][perm] = uvb[:, 0], uvb[:, 1]
        set_obs(sc, fa, np.arange(S), to_world(sc["Tcw"][fa], Xa))
        set_obs(sc, fb, perm, to_world(sc["Tcw"][fb], Xb))
    pairs = np.array([(2 * p, 2 * p + 1) for p in range(n_pairs)], np.int32)
    return dict(scene=sc, pairs=pairs, P=P or R.params(), match=match, T12=T12)


def run_solve(case, p=0, **kw):
    a, b = case["pairs"][p]
    return R.solve_pair(case["scene"], int(a), int(b), case["match"][p], CAM, case["P"], **kw)


def prove_orders(case):
    """the discrete results are the same in the twin's three summation orders, the poses agree to rounding"""
    for p in range(len(case["pairs"])):
        r0 = run_solve(case, p, order=0)[0]
        for o in (1, 2):
            r = run_solve(case, p, order=o)[0]
            for k in ("status", "n_matches", "bound", "visited", "winner", "n_inliers"):
                assert r[k] == r0[k], (k, o, r, r0)
            assert list(r["sample"]) == list(r0["sample"])
            if r0["status"] in (R.OK, R.REJECTED) and r0["n_inliers"] > 3:
                assert np.abs(r["T12"] - r0["T12"]).max() < 1e-9
    return True


WINNER_LAST_SEED, REJECTED_EQUAL_SEED = 402, 1      # found once by a search over the seeds; a changed twin fails loudly here


def winner_last():
    """N = 25 with 4 gross outliers and min_inliers 20: bound 7; with this seed only the last admissible sample is clean"""
    c = solve_case(31, 25, n_out=4, P=R.params(seed=WINNER_LAST_SEED))
    r, _, info = run_solve(c, all_counts=True)
    assert r["status"] == R.OK and r["winner"] == r["bound"] - 1 == 6 and all(x <= 20 for x in info["counts"][:6]), (r, info["counts"])
    return c


def rejected_equal():
    """N = 25 with 7 outliers: no sample reaches more than 20 inliers; the later of the equal bests is reported"""
    c = solve_case(32, 25, n_out=7, P=R.params(seed=REJECTED_EQUAL_SEED))
    r, _, info = run_solve(c, all_counts=True)
    cn = info["counts"]
    assert r["status"] == R.REJECTED and cn.count(max(cn)) >= 2, (r, cn)
    assert r["winner"] == max(i for i, x in enumerate(cn) if x == max(cn)) and r["visited"] == r["bound"] == len(cn)
    return c


def degenerate(kind):
    """N = 3 with min_inliers 3 (bound 1): three equal points (R = I) or three collinear ones"""
    c = solve_case(33, 3, P=R.params(min_inliers=3), identity=True, extra=0)
    sc = c["scene"]
    for f in (0, 1):
        for k, ax in enumerate(("X", "Y", "Z")):
            base = (1.0, -0.5, 12.0)[k] + (0.25 if f else 0.0)
            sc["obs"][f][ax][:3] = base if kind == "equal" else base + np.arange(3) * (0.5, 0.25, 1.0)[k]
    r, _, _ = run_solve(c)
    assert r["bound"] == 1 and r["n_matches"] == 3 and np.isfinite(r["T12"]).all()
    if kind == "equal":
        assert np.array_equal(r["T12"].reshape(4, 4)[:3, :3], np.eye(3))
    return c


def ulp_case(octave, side):
    """One correspondence (keypoint 5 of a) is off by about a pixel; chi2 is then chosen so that its maxerr1 is the float64 next
    above its error e1 (side +1: inlier), e1 itself (0: not) or the one below (-1: not).  Everything else is exact to rounding
    and wins at iteration 0 either way."""
    N = 30
    octs = (np.full(N + 3, octave), np.full(N + 3, 7))
    c = solve_case(34, N, P=R.params(chi2=1e6), octaves=octs, identity=True)
    sc = c["scene"]
    o = sc["obs"][0][5]      # (identity poses: the world is the camera) moved along b's ray, so that only a's image sees it
    X1 = np.array([o["X"], o["Y"], o["Z"]], np.float64)
    d = X1 - c["T12"][:3, 3]
    o["X"], o["Y"], o["Z"] = X1 + 0.3 * d / np.linalg.norm(d)
    r, _, info = run_solve(c)
    assert r["status"] == R.OK and r["winner"] == 0
    j = int(np.flatnonzero(info["corr"]["i1"] == 5)[0])
    assert j not in list(r["sample"])
    e1, e2 = info["e_winner"][0][j], info["e_winner"][1][j]
    s2 = R.sigma2_table(1.2)[octave]
    want = np.nextafter(e1, np.inf) if side > 0 else (e1 if side == 0 else np.nextafter(e1, -np.inf))
    chi2 = want / s2
    for _ in range(64):      # the float64 chi2 whose product with sigma2 is `want`
        if chi2 * s2 == want:
            break
        chi2 = np.nextafter(chi2, np.inf if chi2 * s2 < want else -np.inf)
    assert chi2 * s2 == want, (chi2 * s2, want)
    c["P"] = R.params(chi2=float(chi2))
    r2, inl, info2 = run_solve(c)
    assert r2["status"] == R.OK and r2["winner"] == 0 and info2["corr"]["maxerr1"][j] == want
    assert e2 < info2["corr"]["maxerr2"][j] * 0.9 and inl[5] == (1 if side > 0 else 0), (e1, e2, inl[5])
    assert r2["n_inliers"] == N - (0 if side > 0 else 1)
    return c
