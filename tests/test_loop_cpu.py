"""Loop verification without a GPU: the symbols, every argument check, the twin on a hand-computed pair, the twin's Horn against an
independent Kabsch solve, the bound table against the library's, the sample rule against the device's array-free form, and the
mutant table: every rule of the contract (DESIGN.md section 8 "Loop verification") has a named case that tells it from its
neighbour."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import loop_cases as Cs
import loop_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
PINS = os.path.join(ROOT, "tests", "golden", "loop_restatement_pins.json")

LOOP_SYMBOLS = ["svo_loop_default_params", "svo_loop_create", "svo_loop_destroy", "svo_loop_sync", "svo_loop_stream",
                "svo_loop_last_error", "svo_loop_wait", "svo_loop_bounds", "svo_loop_pairs_dev", "svo_loop_match_dev",
                "svo_loop_solve_dev", "svo_loop_verify_dev", "svo_loop_verify"]


def pins():
    return json.load(open(PINS))


# ---- symbols ------------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "svo.h")).read()
    lib = pkg.load_library()
    for name in LOOP_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in pkg.ABI_SYMBOLS and hasattr(lib, name), name
    assert lib.svo_abi_version() == 8
    for name in ("wait", "pairs_dev", "match_dev", "solve_dev", "verify_dev", "verify", "sync", "stream"):
        assert hasattr(pkg.LoopVerifier, name), name
    assert pkg.LOOP_RESULT_DTYPE == R.RESULT and pkg.LOOP_RESULT_DTYPE.itemsize == 168
    assert pkg.KP_DTYPE == R.KP and pkg.MAP_OBS_DTYPE == R.MAP_OBS and pkg.BOW_FEATURE_DTYPE == R.FEATURE and pkg.BOW_CAND_DTYPE == R.CAND
    assert C.sizeof(pkg.LoopParams) == 56
    assert (pkg.LOOP_OK, pkg.LOOP_FEW, pkg.LOOP_REJECTED, pkg.LOOP_SKIPPED) == (R.OK, R.FEW, R.REJECTED, R.SKIPPED)
    p = pkg.LoopParams.default()
    got = {k: getattr(p, k) for k, _ in pkg.LoopParams._fields_}
    want = dict(R.PARAMS, nn_ratio=float(np.float32(0.75)), scale_factor=float(np.float32(1.2)))
    assert got == want


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_argument_checks_answer_without_a_device(pkg):
    """every check answers SVO_E_INVALID with its message before a device is touched: pointers are never followed, so made-up
    addresses do"""
    lib = pkg.LoopVerifier._bind()
    h = C.c_void_p()
    for dev, kp, pr, needle in ((-1, 64, 1, "device"), (0, 0, 1, "max_kp"), (0, 2049, 1, "max_kp"), (0, 64, 0, "max_pairs"),
                                (0, 64, 65536, "max_pairs")):
        assert lib.svo_loop_create(dev, kp, pr, C.byref(h)) == E_INVALID
        assert needle in lib.svo_loop_last_error(None).decode()
    assert lib.svo_loop_create(0, 64, 1, None) == E_INVALID
    ver = pkg.LoopVerifier(max_kp=64, max_pairs=4)
    h = ver.h
    A = 0x10000          # aligned to everything
    cam = pkg.Camera(fx=700.0, fy=700.0, cx=600.0, cy=180.0, bf=0.0)

    def ok_match():
        return dict(params=pkg.LoopParams.default(), d_desc=A, d_kp=A, d_n=A, kp_stride=64, d_fv=A, d_fv_n=A, d_obs=A, d_obs_n=A,
                    obs_stride=64, d_pairs=A, n_pairs=1, d_match=A, d_match_n=A)

    def ok_solve():
        return dict(cam=cam, params=pkg.LoopParams.default(), d_kp=A, d_obs=A, d_obs_n=A, obs_stride=64, d_Tcw=A, pose_stride_bytes=64,
                    d_pairs=A, n_pairs=1, d_match=A, kp_stride=64, d_result=A, d_inliers=None)

    def refused(fn, kw, needle):
        with pytest.raises(pkg.SvoError) as e:
            fn(**kw)
        assert "invalid" in str(e.value).lower() or "bad argument" in str(e.value), str(e.value)
        assert needle in str(e.value), str(e.value)

    def P(**kw):
        return pkg.LoopParams.default(**kw)
    nan, inf = float("nan"), float("inf")
    match_bad = [(dict(d_desc=None), "d_desc is NULL"), (dict(d_kp=None), "d_kp is NULL"), (dict(d_n=None), "d_n is NULL"),
                 (dict(d_fv=None), "d_fv is NULL"), (dict(d_fv_n=None), "d_fv_n is NULL"), (dict(d_obs=None), "d_obs is NULL"),
                 (dict(d_obs_n=None), "d_obs_n is NULL"), (dict(d_pairs=None), "d_pairs is NULL"), (dict(d_match=None), "d_match is NULL"),
                 (dict(d_match_n=None), "d_match_n is NULL"), (dict(d_obs=A + 8), "16-byte"), (dict(d_desc=A + 2), "4-byte"),
                 (dict(d_fv=A + 4), "8-byte"), (dict(kp_stride=0), "kp_stride"), (dict(kp_stride=65), "kp_stride"),
                 (dict(obs_stride=0), "obs_stride"), (dict(obs_stride=65), "obs_stride"), (dict(n_pairs=0), "n_pairs"),
                 (dict(n_pairs=5), "n_pairs"), (dict(params=P(th_low=0)), "th_low"), (dict(params=P(th_low=257)), "th_low"),
                 (dict(params=P(nn_ratio=0.0)), "nn_ratio"), (dict(params=P(nn_ratio=1.5)), "nn_ratio"),
                 (dict(params=P(nn_ratio=nan)), "nn_ratio")]
    for change, needle in match_bad:
        refused(ver.match_dev, dict(ok_match(), **change), needle)
    solve_bad = [(dict(d_kp=None), "d_kp is NULL"), (dict(d_obs=None), "d_obs is NULL"), (dict(d_obs_n=None), "d_obs_n is NULL"),
                 (dict(d_Tcw=None), "d_Tcw is NULL"), (dict(d_pairs=None), "d_pairs is NULL"), (dict(d_match=None), "d_match is NULL"),
                 (dict(d_result=None), "d_result is NULL"), (dict(d_obs=A + 4), "16-byte"), (dict(kp_stride=65), "kp_stride"),
                 (dict(obs_stride=0), "obs_stride"), (dict(n_pairs=5), "n_pairs"), (dict(n_pairs=0), "n_pairs"),
                 (dict(pose_stride_bytes=60), "pose_stride_bytes"), (dict(pose_stride_bytes=66), "pose_stride_bytes"),
                 (dict(params=P(min_inliers=2)), "min_inliers"), (dict(params=P(max_iterations=0)), "max_iterations"),
                 (dict(params=P(max_iterations=1025)), "max_iterations"), (dict(params=P(prob=0.0)), "prob"),
                 (dict(params=P(prob=1.0)), "prob"), (dict(params=P(prob=nan)), "prob"), (dict(params=P(chi2=inf)), "chi2"),
                 (dict(params=P(chi2=nan)), "chi2"), (dict(params=P(scale_factor=inf)), "scale_factor"),
                 (dict(cam=pkg.Camera(fx=0.0, fy=700.0, cx=1.0, cy=1.0, bf=0.0)), "fx and fy"),
                 (dict(cam=pkg.Camera(fx=700.0, fy=-1.0, cx=1.0, cy=1.0, bf=0.0)), "fx and fy"),
                 (dict(cam=pkg.Camera(fx=700.0, fy=700.0, cx=nan, cy=1.0, bf=0.0)), "not finite")]
    for change, needle in solve_bad:
        refused(ver.solve_dev, dict(ok_solve(), **change), needle)
    both = dict(ok_match(), **ok_solve())
    for change, needle in match_bad[:3] + solve_bad[-6:] + [(dict(params=P(th_low=0)), "th_low")]:
        refused(ver.verify_dev, dict(both, **change), needle)
    refused(ver.pairs_dev, dict(d_cand=None, d_cand_n=A, q0=0, Q=1, top_k=1, d_pairs=A), "d_cand is NULL")
    refused(ver.pairs_dev, dict(d_cand=A, d_cand_n=None, q0=0, Q=1, top_k=1, d_pairs=A), "d_cand_n is NULL")
    refused(ver.pairs_dev, dict(d_cand=A, d_cand_n=A, q0=0, Q=1, top_k=1, d_pairs=None), "d_pairs is NULL")
    refused(ver.pairs_dev, dict(d_cand=A, d_cand_n=A, q0=-1, Q=1, top_k=1, d_pairs=A), "q0")
    refused(ver.pairs_dev, dict(d_cand=A, d_cand_n=A, q0=0, Q=3, top_k=2, d_pairs=A), "max_pairs")
    refused(ver.pairs_dev, dict(d_cand=A, d_cand_n=A, q0=0, Q=1, top_k=17, d_pairs=A), "top_k")
    with pytest.raises(pkg.SvoError) as e:
        ver.wait(None)
    assert "stream is NULL" in str(e.value)
    assert lib.svo_loop_verify(h, None, None, *([None] * 3), 64, *([None] * 4), 64, *([None] * 4)) == E_INVALID
    assert lib.svo_loop_match_dev(None, *([None] * 4), 64, *([None] * 4), 64, None, 1, None, None) == E_INVALID
    assert b"loop is NULL" in lib.svo_loop_last_error(None)
    with pytest.raises(pkg.SvoError):
        pkg.loop_bounds(P(min_inliers=1), 10)
    ver.sync()      # nothing was made: no device was touched
    ver.close()


# ---- the twin by hand ---------------------------------------------------------------------------------------------------------------
def test_twin_by_hand_two_nodes_five_features():
    """a: features 0, 1 in node 3, feature 2 in node 8; b: features 0, 1 in node 3, 2 in node 5 (not in a), 3, 4 in node 8.
    Node 3: a0 sees b0 at 4 and b1 at 28 -> b0; a1 sees only b1 left, at 20 (b0, at 12, is taken) against 256 -> b1.
    Node 8: a2 sees b3 at 30 and b4 at 41: 30 < 0.75 * 41 = 30.75 -> b3.  b2 is never looked at, though it equals a2."""
    rng = np.random.default_rng(1)
    d = [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(3)]
    sc = Cs.scene(2, 6)
    sc["n"][:] = (3, 5)
    a1 = Cs.flip(d[0], range(100, 108))
    sc["desc"][0][:3] = [d[0], a1, d[2]]
    sc["desc"][1][:5] = [Cs.flip(d[0], range(4)), Cs.flip(a1, range(200, 220)), d[2], Cs.flip(d[2], range(30)), Cs.flip(d[2], range(50, 91))]
    assert list(R.hamming(sc["desc"][0][0], sc["desc"][1][:2])) == [4, 28] and list(R.hamming(sc["desc"][0][1], sc["desc"][1][:2])) == [12, 20]
    Cs.set_fv(sc, 0, [3, 3, 8])
    Cs.set_fv(sc, 1, [3, 3, 5, 8, 8])
    for f, n in ((0, 3), (1, 5)):
        Cs.set_obs(sc, f, np.arange(n), np.ones((n, 3), np.float32))
    P = R.params(check_orientation=0)
    m, n, info = R.match_pair(sc, 0, 1, P)
    assert list(m) == [0, 1, 3, -1, -1, -1] and n == 3
    assert info["nodes"] == [(3, 2, 2), (8, 1, 2)]
    assert info["log"][0][:2] == (0, 4) and info["log"][1] == (1, 20, 256, 1) and info["log"][2] == (2, 30, 41, 3)
    # the histogram by hand: differences 10 (x = 0.33 -> bin 0), 100 (3.33 -> 3), -20 + 360 = 340 (11.33 -> 11)
    sc["kp"][0]["angle"][:3] = (10, 100, 0)
    sc["kp"][1]["angle"][[0, 1, 3]] = (0, 0, 20)
    m, n, info = R.match_pair(sc, 0, 1, R.params())
    assert list(info["hist"][[0, 3, 11]]) == [1, 1, 1] and info["hist"].sum() == 3 and info["keep"] == (0, 3, 11) and n == 3
    # the pairs of the candidates
    cand = np.zeros((2, 2), R.CAND)
    cand["frame"] = [[4, 1], [-1, 7]]
    assert R.pairs_of(cand, [2, 1], 10, 2).tolist() == [[10, 4], [10, 1], [-1, -1], [-1, -1]]


def test_fast_scan_is_the_literal_scan():
    c = Cs.root(2, 300)
    a = R.match_pair(c["scene"], 0, 1, c["P"], fast=True)
    b = R.match_pair(c["scene"], 0, 1, c["P"], fast=False)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] > 100 and a[2]["log"] == b[2]["log"]


def test_cases_reach_their_edges():
    for name in Cs.MATCH_MICRO:
        Cs.prove_micro(name)
    Cs.prove_planted(Cs.planted(1))
    for kind in ("equal", "line"):
        Cs.degenerate(kind)
    Cs.prove_orders(Cs.winner_last())
    Cs.prove_orders(Cs.rejected_equal())
    for octave in (0, 7):
        for side in (1, 0, -1):
            Cs.ulp_case(octave, side)


# ---- Horn against Kabsch ------------------------------------------------------------------------------------------------------------
def kabsch(P1, P2):
    """R, t with P1 ~ R P2 + t through numpy.linalg.svd"""
    P1, P2 = np.asarray(P1), np.asarray(P2)
    c1, c2 = P1.mean(0), P2.mean(0)
    H = (P2 - c2).T @ (P1 - c1)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    Rm = Vt.T @ D @ U.T
    return Rm, c1 - Rm @ c2


def horn_vs_kabsch():
    rng = np.random.default_rng(77)
    worst = 0.0
    for trial in range(200):
        n = 3 if trial < 120 else int(rng.integers(4, 60))
        Rt = Cs.rot_axis(rng.normal(size=3), rng.uniform(0, 179))
        t = rng.uniform(-3, 3, 3)
        P2 = rng.uniform(-5, 5, (n, 3)) + [0, 0, 12]
        P1 = P2 @ Rt.T + t + rng.normal(scale=1e-3, size=(n, 3))
        # (triples: well spread ones; a near-collinear triple is ill-conditioned for both solvers)
        if n == 3 and np.linalg.norm(np.cross(P2[1] - P2[0], P2[2] - P2[0])) < 5.0:
            continue
        Rh, th, _ = R.horn(P1.tolist(), P2.tolist(), n == 3)
        Rk, tk = kabsch(P1, P2)
        worst = max(worst, np.abs(np.array(Rh) - Rk).max(), np.abs(np.array(th) - tk).max())
        assert abs(np.linalg.det(np.array(Rh)) - 1.0) < 1e-12
    return worst


def test_horn_against_kabsch():
    worst = horn_vs_kabsch()
    pinned = pins()["horn_vs_kabsch_worst"]
    assert worst <= 10 * pinned, (worst, pinned)
    assert pinned < 1e-10


def test_jacobi_properties():
    """eigenvector of the LARGEST eigenvalue, the lower index among equal ones; R = I for M = 0; at most SWEEPS sweeps"""
    Rm, info = R.quat_rot([[0.0] * 3 for _ in range(3)])
    assert Rm == [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]] and info["col"] == 0 and info["sweeps"] == 1
    rng = np.random.default_rng(3)
    most = 0
    for _ in range(200):
        M = rng.normal(size=(3, 3)) * 10.0 ** rng.uniform(-6, 6)
        Rm, info = R.quat_rot(M.tolist())
        N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                      [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                      [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                      [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
        N = N + np.triu(N, 1).T
        w = np.linalg.eigvalsh(N)
        assert abs(max(info["eig"]) - w[-1]) <= 1e-12 * np.abs(w).max() and info["eig"][info["col"]] == max(info["eig"])
        assert info["sweeps"] < R.SWEEPS
        most = max(most, info["sweeps"])
    assert most <= 8


# ---- bounds and samples ---------------------------------------------------------------------------------------------------------------
def test_bound_table_is_the_librarys(pkg):
    for P in (R.params(), R.params(prob=0.5, min_inliers=3, max_iterations=1024), R.params(prob=0.999999, min_inliers=100, max_iterations=7)):
        lib = pkg.loop_bounds(pkg.LoopParams.default(**P), 2048)
        assert np.array_equal(lib, R.bounds(P, 2048))
        assert (lib[:P["min_inliers"]] == 0).all() and lib[P["min_inliers"]] == 1 and lib.max() <= P["max_iterations"]
    assert R.bounds(R.params(), 25)[25] == 7 and R.bounds(R.params(), 2048)[2048] == 300


def sample_closed_form(seed, it, N):
    """the device's form of the three draws: no array, the two overwritten slots followed by hand"""
    r = [(R.splitmix64((seed + 3 * it + d) & R.MASK) * (N - d)) >> 64 for d in range(3)]
    v0 = N - 1
    v1 = v0 if N - 2 == r[0] else N - 2
    return [r[0], v0 if r[1] == r[0] else r[1], v1 if r[2] == r[1] else (v0 if r[2] == r[0] else r[2])]


def test_samples():
    assert R.splitmix64(0) == 0xE220A8397B1DCDAF and R.splitmix64(1) == 0x910A2DEC89025CC1      # the published first outputs
    seen = set()
    for N in (3, 4, 5, 7, 20, 500, 2048):
        for it in range(400 if N < 8 else 60):
            for seed in (0, R.PARAMS["seed"], R.MASK):
                s = R.sample(seed, it, N)
                assert len(set(s)) == 3 and all(0 <= x < N for x in s)
                assert s == sample_closed_form(seed, it, N), (seed, it, N)
                if N == 4:
                    seen.add(tuple(s))
    assert len(seen) == 24      # every ordered triple of 0 .. 3 comes up
    assert pins()["samples_seed_default_N20"] == [R.sample(R.PARAMS["seed"], i, 20) for i in range(4)]


def test_sigma2_is_pinned():
    assert R.sigma2_table(1.2) == pins()["sigma2_scale_1.2"]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()      # the contract states the same eight values
    at = design.index("for `scale_factor` 1.2f:")
    listed = [float(x) for x in re.findall(r"\d+(?:\.\d+)?", design[at + 24:at + 260])[:8]]
    assert listed == R.sigma2_table(1.2), listed
    assert R.sigma2_table(1.2)[0] == 1.0 and R.sigma2_table(1.2)[1] == float(np.float32(np.float32(1.2) * np.float32(1.2)))


def test_case_pins():
    """the twin's results on the named cases are the pinned ones (tools/make_loop_pins.py)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_loop_pins", os.path.join(ROOT, "tools", "make_loop_pins.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.case_pins() == pins()["cases"]


# ---- the mutant table -----------------------------------------------------------------------------------------------------------------
def _match(case, **mut):
    m, n, _ = R.match_pair(case["scene"], 0, 1, case["P"], R.rules(**mut))
    return list(m[:case["scene"]["n"][0]])


MATCH_MUTANTS = [("tie_second", False, "tied_best"), ("th_le", True, "threshold_49_50"), ("ratio_f64", True, "ratio_f32_edge"),
                 ("use_matched2", False, "second_taken"), ("use_matched2", False, "compete2"), ("nomp_in_best2", True, "no_mp_second"),
                 ("round_even", True, "half_bins"), ("wrap30", False, "wrap_30"), ("maxima_later", True, "maxima_ties"),
                 ("tenth_le", True, "tenth")]


@pytest.mark.parametrize("rule,value,name", MATCH_MUTANTS, ids=["%s-%s" % (r, n) for r, _, n in MATCH_MUTANTS])
def test_match_mutant_is_killed(rule, value, name):
    c = Cs.MATCH_MICRO[name][0]()
    assert _match(c) == Cs.MATCH_MICRO[name][1]
    assert _match(c, **{rule: value}) != Cs.MATCH_MICRO[name][1], (rule, name)


def test_le_on_the_best_distance_cannot_be_told_apart():
    """`<=` on the best distance takes the later of two tied i2 - and makes the earlier the second best at the same distance, so
    the ratio test (nn_ratio <= 1) refuses either way: this mutant is equivalent, no case can kill it.  What the rule protects is
    seen next to its neighbour: once a tie does not become the second best, `<` accepts the earlier i2 and `<=` still refuses."""
    c = Cs.tied_best()
    assert _match(c) == _match(c, best_le=True) == [-1]
    assert _match(c, tie_second=False) == [0] and _match(c, tie_second=False, best_le=True) == [-1]
    for name in sorted(Cs.MATCH_MICRO):
        c = Cs.MATCH_MICRO[name][0]()
        assert _match(c) == _match(c, best_le=True), name


def _solve(case, **mut):
    r, inl, info = Cs.run_solve(case, R=R.rules(**mut))
    return (int(r["status"]), int(r["winner"]), int(r["visited"]), int(r["n_inliers"]), list(r["sample"]), inl.tobytes())


def test_solve_mutants_are_killed():
    c = Cs.rejected_equal()
    assert _solve(c) != _solve(c, best_gt=True)                 # the later of two equal bests
    c = Cs.solve_case(3, 40, P=R.params(min_inliers=40))         # every sample gives exactly min_inliers inliers: never "more than"
    assert _solve(c)[0] == R.REJECTED and _solve(c, stop_ge=True)[0] == R.OK
    c = Cs.solve_case(3, 5, P=R.params(min_inliers=3))
    assert any(len(set(R.sample(c["P"]["seed"], i, 5, True))) < 3 for i in range(20))
    assert [R.sample(c["P"]["seed"], i, 5) for i in range(20)] != [R.sample(c["P"]["seed"], i, 5, True) for i in range(20)]
    c = Cs.solve_case(40, 30)
    c["scene"]["kp"][0]["x"][:30] += 40.0                      # the keypoints are somewhere else than the projected map points
    assert _solve(c)[0] == R.OK and _solve(c, use_keypoint=True) != _solve(c)
    c = Cs.solve_case(41, 30, identity=True, octaves=(0, 0))    # a's image agrees, b's does not: 6 points moved along a's rays
    sc = c["scene"]
    for j in range(6):
        o = sc["obs"][0][j]
        o["X"], o["Y"], o["Z"] = 1.5 * o["X"], 1.5 * o["Y"], 1.5 * o["Z"]
    assert _solve(c) != _solve(c, one_sided=True)
    c = Cs.ulp_case(0, 0)                                       # a's octave 0, b's 7: maxerr taken from the other frame
    assert _solve(c) != _solve(c, wrong_octave=True)
