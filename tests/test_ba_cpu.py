"""CPU suite of the windowed bundle adjustment (svo_ba_*; DESIGN.md section 8 "Windowed bundle adjustment"): the ABI and the host-side
argument checks of the library, and the numpy twin (tests/ba_ref.py) against things that are not the twin - central differences,
a dense solve of the full damped system, hand-made records for the edge-list rules - plus its pins and the scatter between its
summation orders, the yardstick of tests/test_ba_gpu.py."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import ba_cases  # noqa: E402
import ba_ref  # noqa: E402
import test_abi  # noqa: E402

BA_NAMES = ["svo_ba_default_params", "svo_ba_create", "svo_ba_destroy", "svo_ba_sync", "svo_ba_stream", "svo_ba_last_error",
            "svo_ba_windows_dev", "svo_ba_window"]


# ---- the library without a device ------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound(pkg):
    lib = pkg.load_library()
    for name in BA_NAMES:
        assert name in test_abi.declared_symbols(), name
        assert name in pkg.ABI_SYMBOLS, name
        assert hasattr(lib, name), name
    for name in ("windows_dev", "window", "sync", "stream"):
        assert hasattr(pkg.BundleAdjuster, name)
    assert lib.svo_abi_version() == 8
    assert pkg.BA_STATS_DTYPE.itemsize == 48 and pkg.BA_POINT_DTYPE.itemsize == 32
    assert C.sizeof(pkg.BaParams) == 40


def test_default_params(pkg):
    p = pkg.BaParams.default()
    assert (p.window, p.n_fixed, p.iterations, p.stereo) == (8, 1, 10, 1)
    assert p.huber_mono == float(np.float32(math.sqrt(5.991))) == ba_ref.HUBER_MONO
    assert p.huber_stereo == float(np.float32(math.sqrt(7.815))) == ba_ref.HUBER_STEREO
    assert p.lambda_init == 0.0
    assert pkg.load_library().svo_ba_default_params(None) == -1
    d = ba_ref.default_params()
    assert all(getattr(p, k) == v for k, v in d.items())


def test_argument_checks_answer_without_a_device(pkg):
    """Every refusal is SVO_E_INVALID with a message that names the argument, before a device is touched: the pointers below are
    host memory (or made up) and are never followed."""
    lib = pkg.load_library()
    ba = pkg.BundleAdjuster(max_kp=64, max_windows=3)      # touches no device
    cam = pkg.Camera(**pkg.KITTI_00_02)
    par = pkg.BaParams.default()
    buf = np.zeros(1 << 12, np.uint8)
    base = (buf.ctypes.data + 63) & ~63
    good = dict(ba=ba.h, cam=C.addressof(cam), params=C.addressof(par), d_obs=base, d_counts=base, obs_stride=64, d_Tcw=base,
                pose_stride_bytes=64, first=0, n_windows=1, step=1, d_Tcw_out=base, d_points=None, d_stats=base, producer=None)
    order = list(good)
    keep = []

    def call(**kw):
        a = dict(good)
        a.update(kw)
        rc = lib.svo_ba_windows_dev(*[a[k] for k in order])
        return rc, lib.svo_ba_last_error(a["ba"]).decode()

    def params(**kw):
        q = pkg.BaParams.default(**kw)
        keep.append(q)
        return C.addressof(q)

    def camera(**kw):
        d = dict(pkg.KITTI_00_02)
        d.update(kw)
        c = pkg.Camera(**d)
        keep.append(c)
        return C.addressof(c)

    cases = [
        (dict(ba=None), "ba"), (dict(cam=None), "cam"), (dict(params=None), "params"), (dict(d_obs=None), "d_obs"),
        (dict(d_counts=None), "d_counts"), (dict(d_Tcw=None), "d_Tcw"), (dict(d_Tcw_out=None), "d_Tcw_out"), (dict(d_stats=None), "d_stats"),
        (dict(params=params(window=1)), "window"), (dict(params=params(window=9)), "window"),
        (dict(params=params(n_fixed=0)), "n_fixed"), (dict(params=params(window=4, n_fixed=4)), "n_fixed"),
        (dict(params=params(iterations=0)), "iterations"), (dict(params=params(iterations=21)), "iterations"),
        (dict(params=params(huber_mono=float("nan"))), "huber_mono"), (dict(params=params(huber_stereo=float("inf"))), "huber_stereo"),
        (dict(params=params(lambda_init=float("-inf"))), "lambda_init"),
        (dict(cam=camera(cx=float("nan"))), "camera"), (dict(cam=camera(bf=float("inf"))), "camera"),
        (dict(cam=camera(fx=0.0)), "fx"), (dict(cam=camera(fy=-1.0)), "fy"),
        (dict(obs_stride=65), "obs_stride"), (dict(obs_stride=0), "obs_stride"),
        (dict(n_windows=4), "n_windows"), (dict(n_windows=0), "n_windows"),
        (dict(first=-1), "first"), (dict(step=0), "step"), (dict(d_obs=base + 8), "d_obs"),
        (dict(pose_stride_bytes=60), "pose_stride_bytes"),
    ]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == -1, (kw, rc)
        assert msg.startswith("svo_ba_windows_dev: ") and word in msg, (kw, msg)
    # the host-to-host entry shares the checks
    lib.svo_ba_window.argtypes = [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 5
    q = pkg.BaParams.default(window=9)
    assert lib.svo_ba_window(ba.h, C.addressof(cam), C.addressof(q), base, base, 64, base, base, None, None, base) == -1
    assert "window" in lib.svo_ba_last_error(ba.h).decode()
    assert lib.svo_ba_window(ba.h, C.addressof(cam), C.addressof(par), None, base, 64, base, base, None, None, base) == -1
    assert lib.svo_ba_window(None, C.addressof(cam), C.addressof(par), base, base, 64, base, base, None, None, base) == -1
    # svo_ba_create
    h = C.c_void_p()
    for dev, kp, nw in ((0, 0, 1), (0, 4097, 1), (0, 64, 0), (-1, 64, 1)):
        assert lib.svo_ba_create(dev, kp, nw, C.byref(h)) == -1 and not h.value
        assert lib.svo_ba_last_error(None).decode().startswith("svo_ba_create: ")
    assert lib.svo_ba_create(0, 64, 1, None) == -1
    ba.close()


# ---- the twin against things that are not the twin ---------------------------------------------------------------------------------
def _problem(name):
    c = ba_cases.case(name)
    return c, ba_ref.Problem(c["obs"], c["counts"], c["Tcw"], c["cam"], c["params"])


# measured on the cases below: largest |analytic - central difference| / max(1, |analytic|) 1.07e-7 (mono), 2.02e-7 (stereo), with
# steps of 1e-6 (the difference quotient's own error: h^2 x third derivative + 1e-16 x |e| / h); a margin of 10
JAC_TOL = 2.1e-6


@pytest.mark.parametrize("kind", ["mono", "stereo"])
def test_jacobians_against_central_differences(kind):
    """Both edge types' Jacobians (points and poses) against central differences of the twin's own residual: the mono edge's
    residual as it is, the stereo edge's with a double 1 / z (the float invz of cam_project is a staircase at this scale).
    Tolerance JAC_TOL: ten times the measured difference (see its comment)."""
    c, pr = _problem("mono_two_fixed" if kind == "mono" else "w8_fixed1")
    est, X = list(pr.est0), pr.assoc["X0"].copy()
    h, worst, seen = 1e-6, 0.0, 0
    for f in range(pr.nfix, pr.W):
        sel = pr.mask[:, f] & (pr.stereo[:, f] if kind == "stereo" else ~pr.stereo[:, f])
        if not sel.any():
            continue
        pc, _ = pr.errors(est, X, f, exact_invz=True)
        Jl, Jp = ba_ref.jacobians(est[f], pc, pr.cam, pr.stereo[:, f])
        for a in range(3):
            Xp, Xm = X.copy(), X.copy()
            Xp[:, a] += h
            Xm[:, a] -= h
            ep, em = pr.errors(est, Xp, f, exact_invz=True)[1], pr.errors(est, Xm, f, exact_invz=True)[1]
            for i in range(3):
                num = (ep[i] - em[i]) / (2 * h)
                worst = max(worst, float(np.max(np.abs(num - Jl[i][a])[sel] / np.maximum(1.0, np.abs(Jl[i][a])[sel]))))
        for r in range(6):
            u = [0.0] * 6
            u[r] = h
            ep_ = list(est)
            ep_[f] = ba_ref.se3_oplus(u, est[f])
            u[r] = -h
            em_ = list(est)
            em_[f] = ba_ref.se3_oplus(u, est[f])
            ep, em = pr.errors(ep_, X, f, exact_invz=True)[1], pr.errors(em_, X, f, exact_invz=True)[1]
            for i in range(3):
                num = (ep[i] - em[i]) / (2 * h)
                worst = max(worst, float(np.max(np.abs(num - Jp[i][r])[sel] / np.maximum(1.0, np.abs(Jp[i][r])[sel]))))
        seen += int(sel.sum())
    print("jacobians %s: %d edges, worst %.3e" % (kind, seen, worst))
    assert seen > 50
    assert worst < JAC_TOL


# measured: largest |Schur - dense| / max(1, largest |dense|) over the pose and the point unknowns 2.67e-12 at lambda 1e-3 (less at
# lambda 10; both float64, the dense solve is LAPACK's); a margin of 10
SCHUR_TOL = 2.7e-11


def test_schur_solve_against_a_dense_solve():
    """BlockSolver's route (Dinv, Hschur, LDL^T, back-substitution) against one dense solve of the full damped system with
    6 free + 3 points unknowns, on a case of 20 points.  Tolerance SCHUR_TOL: ten times the measured difference."""
    c = ba_cases.make(seed=61, window=4, n_points=20)
    pr = ba_ref.Problem(c["obs"], c["counts"], c["Tcw"], c["cam"], c["params"])
    so, po = ba_ref._orders(pr.P, pr.W, "canonical")
    S = pr.build(list(pr.est0), pr.assoc["X0"].copy(), so, po)
    assert pr.P == 20
    n, P = 6 * pr.nfree, pr.P
    for lam in (1e-3, 10.0):
        ok, x, dx = pr.solve(S, lam, so, po)
        assert ok
        H = np.zeros((n + 3 * P, n + 3 * P))
        b = np.concatenate([S["bp"].ravel(), S["bl"].ravel()])
        for j in range(pr.nfree):
            H[6 * j:6 * j + 6, 6 * j:6 * j + 6] = S["Hpp"][j]
            for p in range(P):
                H[6 * j:6 * j + 6, n + 3 * p:n + 3 * p + 3] = S["W"][p, j]
                H[n + 3 * p:n + 3 * p + 3, 6 * j:6 * j + 6] = S["W"][p, j].T
        for p in range(P):
            H[n + 3 * p:n + 3 * p + 3, n + 3 * p:n + 3 * p + 3] = S["Hll"][p]
        H += lam * np.eye(n + 3 * P)
        ref = np.linalg.solve(H, b)
        got = np.concatenate([x, dx.ravel()])
        worst = float(np.abs(got - ref).max() / max(1.0, float(np.abs(ref).max())))
        print("schur lambda %g: worst %.3e" % (lam, worst))
        assert worst < SCHUR_TOL


def _records(rows, window, stride=8):
    """rows: (frame, gid, kp, u, v, depth, X, Y, Z) in storage order."""
    obs = np.zeros((window, stride), ba_ref.MAP_OBS_DTYPE)
    counts = np.zeros(window, np.int32)
    for f, g, kp, u, v, d, X, Y, Z in rows:
        obs[f, counts[f]] = (g, kp, 0, u, v, d, X, Y, Z)
        counts[f] += 1
    return obs, counts


def test_edge_list_rules():
    W = 3
    T = np.tile(np.eye(4, dtype=np.float32), (W, 1, 1))
    T[2, 2, 3] = -5.0          # frame 2 stands 5 m ahead: a point at Z = 4 is behind it
    big = 2 ** 31 - 1
    rows = [
        # gid 10: frames 0 and 1, in frame 1 twice - the lower kp (stored later) counts
        (0, 10, 3, 1.0, 2.0, 9.0, 0.1, 0.2, 8.0), (1, 10, 5, 50.0, 2.0, 9.0, 7.0, 7.0, 7.0), (1, 10, 2, 60.0, 2.0, -1.0, 7.0, 7.0, 7.0),
        # gid 11: one record only - dropped
        (1, 11, 0, 1.0, 1.0, 5.0, 0.0, 0.0, 6.0),
        # gid 12: ahead of frames 0, 1, behind frame 2 (z = 4 - 5): two edges left
        (0, 12, 1, 1.0, 1.0, 4.0, 0.0, 0.0, 4.0), (1, 12, 1, 1.0, 1.0, 4.0, 0.0, 0.0, 4.0), (2, 12, 1, 1.0, 1.0, 4.0, 0.0, 0.0, 4.0),
        # gid 13: frames 1 and 2, behind frame 2: one edge left - dropped
        (1, 13, 4, 1.0, 1.0, 4.0, 0.0, 0.0, 4.5), (2, 13, 4, 1.0, 1.0, 4.0, 0.0, 0.0, 4.5),
        # gid 14: z = 0 in frames 0 and 1 (dropped), ... so no point
        (0, 14, 6, 1.0, 1.0, 4.0, 1.0, 1.0, 0.0), (1, 14, 6, 1.0, 1.0, 4.0, 1.0, 1.0, 0.0),
        # gids near 2^31 - 1, stored in descending order; the start position is the EARLIEST frame's record
        (1, big, 7, 1.0, 1.0, 4.0, 9.0, 9.0, 9.0), (0, big, 7, 1.0, 1.0, 4.0, 1.0, 1.0, 20.0), (2, big, 0, 1.0, 1.0, 4.0, 8.0, 8.0, 8.0),
        (0, big - 1, 0, 1.0, 1.0, 4.0, 2.0, 2.0, 30.0), (2, big - 1, 2, 1.0, 1.0, 4.0, 2.0, 2.0, 30.0),
    ]
    obs, counts = _records(rows, W)
    a = ba_ref.associate(obs, counts, T, W)
    assert list(a["gid"]) == [10, 12, big - 1, big]
    assert list(a["n_obs"]) == [2, 2, 2, 3]
    assert a["mask"].tolist() == [[True, True, False], [True, True, False], [True, False, True], [True, True, True]]
    assert a["X0"].tolist() == [[float(np.float32(0.1)), float(np.float32(0.2)), 8.0], [0.0, 0.0, 4.0], [2.0, 2.0, 30.0], [1.0, 1.0, 20.0]]
    k = int(a["rec"][0, 1])
    assert obs["kp"][1, k] == 2 and obs["u"][1, k] == 60.0
    # a count above the stride is clamped, a negative one is 0
    counts2 = counts.copy()
    counts2[0] = 100
    counts2[2] = -3
    a2 = ba_ref.associate(obs, counts2, T, W)
    assert list(a2["gid"]) == [10, 12, big]
    # edge types: depth > 0 and stereo = 1
    p = ba_ref.default_params()
    p.update(window=W, n_fixed=1)
    pr = ba_ref.Problem(obs, counts, T, ba_cases.KITTI, p)
    assert pr.stereo[0].tolist() == [True, False, False]
    bf = float(np.float32(ba_cases.KITTI[4]))
    assert pr.obs[2][0, 0] == 1.0 - bf / 9.0 and pr.obs[2][0, 1] == 0.0
    p["stereo"] = 0
    assert not ba_ref.Problem(obs, counts, T, ba_cases.KITTI, p).stereo.any()


# ---- the pins and the order scatter ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def all_orders():
    return {name: ba_cases.run_orders(name) for name in ba_cases.CASES}


def test_restatement_matches_its_pins(all_orders):
    """The twin's discrete results per case, and the scatter between its summation orders (the device tests' yardstick): the
    recorded scatter is not exceeded by more than a factor of 2 (it is a deterministic float64 computation; equal on this
    numpy)."""
    want = json.load(open(os.path.join(ba_ref.GOLDEN, "ba_restatement_pins.json")))
    assert sorted(want) == sorted(ba_cases.CASES)
    for name, rs in all_orders.items():
        assert ba_ref.discrete(rs[0]) == want[name]["discrete"], name
        sc = ba_cases.scatter(rs)
        for k, v in sc.items():
            assert v <= 2 * want[name]["scatter"][k] + 1e-16, (name, k, v, want[name]["scatter"][k])


def test_discrete_results_do_not_depend_on_the_summation_order(all_orders):
    """A condition on the case list: no case is excused, a seed that fails it is replaced."""
    for name, rs in all_orders.items():
        d = [ba_ref.discrete(r) for r in rs]
        assert d[0] == d[1] == d[2], name
        for r in rs[1:]:
            assert np.array_equal(r["gid"], rs[0]["gid"]) and np.array_equal(r["n_obs"], rs[0]["n_obs"]), name


def test_chi2_of_the_accepted_estimates_never_increases(all_orders):
    for name, rs in all_orders.items():
        r = rs[0]
        if r["stats"]["status"] != ba_ref.STATUS_OK:
            continue
        cur = r["stats"]["chi2_initial"]
        for trials in r["log"]:
            for lam, chi, rho, accepted, solved in trials:
                if accepted:
                    assert chi <= cur, name
                    cur = chi
        assert cur == r["stats"]["chi2_final"] <= r["stats"]["chi2_initial"], name


def test_cases_reach_what_they_are_for(all_orders):
    """The twin's log proves the paths the GPU cases are there for."""
    def log(name):
        return all_orders[name][0]["log"]
    assert any(not acc for t in log("rejected_trial") for _, _, _, acc, _ in t)
    assert len(log("rejected_first")[0]) > 1
    assert len(log("ten_rejections")[-1]) == 10 and not any(acc for _, _, _, acc, _ in log("ten_rejections")[-1])
    assert all_orders["empty"][0]["stats"]["status"] == ba_ref.STATUS_EMPTY
    for n, want in (("n1", 1), ("n2", 2), ("n63", 63), ("n64", 64), ("n65", 65), ("n255", 255), ("n256", 256), ("n257", 257),
                    ("big_500x8", 500), ("big_2000x2", 2000)):
        assert all_orders[n][0]["stats"]["n_points"] == want, n
    assert all_orders["big_500x8"][0]["stats"]["n_edges"] == 4000 == all_orders["big_2000x2"][0]["stats"]["n_edges"]
    s = all_orders["mono_two_fixed"][0]["stats"]
    assert s["n_edges_stereo"] == 0 and s["n_edges"] > 0
    s = all_orders["mixed_depth"][0]["stats"]
    assert 0 < s["n_edges_stereo"] < s["n_edges"]
    # Huber's linear branch is reached with outliers; a frame without edges keeps its pose
    c, pr = _problem("outliers")
    e = pr.errors(list(pr.est0), pr.assoc["X0"], 3)[1]
    chi = e[0] * e[0] + e[1] * e[1] + e[2] * e[2]
    assert (chi[pr.mask[:, 3]] > ba_ref.HUBER_STEREO ** 2).any()
    for name, f in (("free_no_edges", 4), ("counts0", 3)):
        c = ba_cases.case(name)
        assert np.array_equal(all_orders[name][0]["Tcw"][f], c["Tcw"][f].astype(np.float64).ravel()), name
    # the point behind frames 5 .. 7 keeps its edges in frames 3 and 4
    r = all_orders["behind"][0]
    assert r["n_obs"][list(r["gid"]).index(77)] == 2
