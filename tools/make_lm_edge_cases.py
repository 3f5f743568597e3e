"""Writes tests/golden/lm_edge_cases.npz, the fixture of tests/test_lm_edges_cpu.py and tests/test_lm_edges_gpu.py: pose-only LM
problems (Optimizer::PoseOptimization) that walk the paths the seeded, well-posed problems of the suite never take - the retry
loop (2, 3..5, 6..9 trials in one iteration, the stop on ten rejections), ten iterations without termination, the stops on
nBad >= 3 and on rho == 0, a restart from the LM's own result (theta < 1e-5 in SE3Quat::exp), starts rotated by +-170 degrees about
each axis (the three "largest diagonal" branches of Eigen's Quaternion(Matrix3) and the q.w < 0 flip), every edge on Huber's linear
branch, points behind the camera, n = 2 and 3, the chunk boundaries of the device's build (n = 127 .. 321), starts 40 degrees off
(libm's sin / cos: not bit-comparable) and a depth of exactly zero.  Every case is searched or built here, walked by the CPU
restatement (oracle/orc_pose.c) and stored with its pose and statistics as the restatement left them, the trials each iteration
took, how the LM stopped and the restatement's branch counters (orc_pose_last_counts); coverage() - shared with the CPU test -
proves every tag from those records and fails if one is missing.  Needs no GPU:  python tools/make_lm_edge_cases.py"""
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
PATH = os.path.join(ROOT, "tests", "golden", "lm_edge_cases.npz")
MAX_BYTES = 167028                          # (the largest EPnP fixture, epnp_gn_cases.npy)
BITWISE, LARGE_ROTATION, DEPTH_ZERO = 0, 1, 2
STOPS = {"qmax": 0, "rho0": 1, "nbad": 2, "ten": 3}
K_DYADIC = np.array([512.0, 512.0, 320.0, 240.0])
SEARCH_N, SEARCH_SEEDS = 40, 3000           # the seeded search: problems of 40 edges, this many seeds at the most


def rodrigues(w):
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.eye(3)
    k = np.asarray(w, np.float64) / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def rigid(R, t=(0, 0, 0)):
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
    return T


def walk(orc, Xw, obs, K, T0):
    """The restatement on one problem: everything the fixture keeps of it."""
    T, st, tr = orc.pose_opt(Xw, obs, K, T0)
    counts = orc.pose_counts()
    trials = np.zeros(10, np.int32)
    for row in tr:
        trials[int(row[0])] += 1
    last = int(st.iterations) - 1
    if st.terminated and trials[last] == 10:
        stop = "qmax"
    elif st.terminated and tr[-1, 5] == 0:
        stop = "rho0"
    elif st.terminated:
        stop = "nbad"
    else:
        stop = "ten"
    return {"T": T, "stats_i": np.array([st.n_edges, st.iterations, st.trials_total, st.terminated], np.int32),
            "stats_f": np.array([st.chi2_initial, st.chi2_final, st.lambda_final], np.float64), "counts": counts, "trials": trials,
            "stop": STOPS[stop], "failed_solves": int((tr[:, 7] == 0).sum()), "trace": tr}


def twin_difference(Xw, obs, K, T0, w):
    """The numpy twin (tests/golden/make_golden.py, sin / cos from numpy everywhere) on the same case: does it agree with the
    restatement within the tolerances of test_oracle_golden.test_lm_trace - the same branch sequence, every trial's lambda, chi2
    and rho, the pose, chi2 at both ends -, and how far are its pose and final chi2 from the restatement's."""
    import make_golden as mg
    T, trace, chi0, chi1, lam, iters = mg.pose_opt(Xw, obs, K, T0)
    tr = w["trace"]
    same = trace.shape == tr.shape and np.array_equal(trace[:, [0, 1, 6, 7]], tr[:, [0, 1, 6, 7]])
    same = same and np.allclose(tr[:, 2:6], trace[:, 2:6], rtol=1e-7) and np.allclose(w["T"], T, rtol=0, atol=1e-8)
    same = same and iters == w["stats_i"][1] and np.isclose(w["stats_f"][0], chi0, rtol=1e-10) and np.isclose(w["stats_f"][1], chi1, rtol=1e-7)
    return bool(same), float(np.abs(T - w["T"]).max()), float(abs(chi1 - w["stats_f"][1]))


def case(orc, tag, kind, Xw, obs, K, T0, twin=False):
    Xw = np.ascontiguousarray(Xw, np.float64); obs = np.ascontiguousarray(obs, np.float64)
    w = walk(orc, Xw, obs, K, T0)
    c = {"tag": tag, "kind": kind, "Xw": Xw, "obs": obs, "K": np.array(K, np.float64), "T0": np.array(T0, np.float64),
         "twin_dT": np.nan, "twin_dchi": np.nan}
    c.update({k: w[k] for k in ("T", "stats_i", "stats_f", "counts", "trials", "stop", "failed_solves")})
    if twin:
        same, c["twin_dT"], c["twin_dchi"] = twin_difference(Xw, obs, K, T0, w)
        assert same, "the numpy twin and the restatement part ways on " + tag
    if kind == BITWISE:
        assert c["counts"][2] == 0, tag + ": a bitwise case on libm's sin / cos"
    return c


def offset_start(T_true, rng):
    """N(0, 0.08 rad) / N(0, 5 m) per axis, applied to the true pose"""
    return rigid(rodrigues(rng.normal(0, 0.08, 3)), rng.normal(0, 5.0, 3)) @ T_true


def searched(orc, util):
    """Seeded problems with an offset start, classified by what the restatement does on them: two of each kind the retry loop and the
    stopping rules offer, all of them on the fixed series (no libm)."""
    want = {"trials 2": 2, "trials 3..5": 2, "trials 6..9": 2, "stop qmax": 2, "ten iterations": 2, "stop nbad": 2}
    out, seen = [], {k: 0 for k in want}
    for seed in range(SEARCH_SEEDS):
        if all(seen[k] >= want[k] for k in want):
            break
        Xw, obs, K, T_true = util.pose_problem(seed, n=SEARCH_N)
        T0 = offset_start(T_true, np.random.default_rng(100000 + seed))
        w = walk(orc, Xw, obs, K, T0)
        if w["counts"][2] != 0 or not np.isfinite(w["stats_f"]).all():
            continue
        mx = int(w["trials"].max())
        tag = None
        if w["stop"] == STOPS["qmax"]:
            tag = "stop qmax"
        elif w["stop"] == STOPS["ten"]:
            tag = "ten iterations"
        elif mx == 2:
            tag = "trials 2"
        elif 3 <= mx <= 5:
            tag = "trials 3..5"
        elif 6 <= mx <= 9:
            tag = "trials 6..9"
        elif w["stop"] == STOPS["nbad"] and mx == 1:
            tag = "stop nbad"
        if tag is None or seen[tag] >= want[tag]:
            continue
        if not twin_difference(Xw, obs, K, T0, w)[0]:      # (kept only where the independent twin walks the same branches)
            continue
        seen[tag] += 1
        out.append(case(orc, tag, BITWISE, Xw, obs, K, T0, twin=True))
    missing = [k for k in want if seen[k] < want[k]]
    return out, missing, seed + 1


def built(orc, util):
    out = []
    # the stop on rho == 0 from exact data: dyadic camera, identity pose, points on a 1/16 grid at depths 2, 4, 8 - every operation exact
    for shift in (0, 1):
        pts = [((i - 2 + shift) / 16.0 * z, (j - 1) / 16.0 * z, z) for i in range(4) for j in range(4) for z in ((2.0, 4.0, 8.0)[(i + j) % 3],)]
        Xw = np.array(pts)
        obs = np.stack([K_DYADIC[0] * Xw[:, 0] / Xw[:, 2] + K_DYADIC[2], K_DYADIC[1] * Xw[:, 1] / Xw[:, 2] + K_DYADIC[3]], 1)
        out.append(case(orc, "stop rho0 exact", BITWISE, Xw, obs, K_DYADIC, np.eye(4), twin=True))
    # a restart from the LM's own result: the first step is below 1e-5 rad
    n_restart = 0
    for seed in range(200):
        Xw, obs, K, T_true = util.pose_problem(seed, n=SEARCH_N)
        T1 = walk(orc, Xw, obs, K, np.eye(4))["T"]
        w = walk(orc, Xw, obs, K, T1)
        if w["counts"][0] > 0 and w["counts"][2] == 0:
            out.append(case(orc, "restart", BITWISE, Xw, obs, K, T1, twin=True))
            n_restart += 1
            if n_restart == 2:
                break
    # starts rotated by +-170 degrees about x, y, z, the scene consistent with them (the start is the true pose, the observations noisy)
    for axis in range(3):
        for sign in (1, -1):
            Xw, obs, K, T_true = util.pose_problem(300 + axis, n=SEARCH_N)
            w3 = np.zeros(3); w3[axis] = sign * np.deg2rad(170.0)
            A = rigid(rodrigues(w3))
            T0 = A @ T_true                                  # camera pose: the scene is seen from a frame turned by 170 degrees
            Xc = (T_true[:3, :3] @ Xw.T).T + T_true[:3, 3]
            Xw2 = (T0[:3, :3].T @ (Xc - T0[:3, 3]).T).T        # the same camera-frame points under the turned pose
            out.append(case(orc, "rot170 %s%s" % ("xyz"[axis], "+" if sign > 0 else "-"), BITWISE, Xw2, obs, K, T0, twin=True))
    # every edge on Huber's linear branch: +-300 px on every observation
    # (independent signs pull the first step beyond 0.5 rad, onto libm, and the fit then brings some edges back under delta; so every
    # world point is there twice, observed 300 px off in opposite directions: the pulls cancel, the steps stay small, no edge ever
    # leaves the linear branch)
    n_huber = 0
    for seed in range(400, 1400):
        Xw, obs, K, T_true = util.pose_problem(seed, n=SEARCH_N // 2, outlier_frac=0.0)
        sg = np.random.default_rng(seed).choice([-1.0, 1.0], obs.shape)
        Xw = np.repeat(Xw, 2, axis=0)
        obs = np.repeat(obs, 2, axis=0) + 300.0 * np.repeat(sg, 2, axis=0) * np.tile([[1.0], [-1.0]], (SEARCH_N // 2, 1))
        w = walk(orc, Xw, obs, K, T_true)
        if w["counts"][2] == 0 and twin_difference(Xw, obs, K, T_true, w)[0]:      # (steps below 0.5 rad: the fixed series)
            out.append(case(orc, "huber linear", BITWISE, Xw, obs, K, T_true, twin=True))
            n_huber += 1
            if n_huber == 2:
                break
    # a fifth of the points 120 m behind the camera
    for seed in (410, 411):
        Xw, obs, K, T_true = util.pose_problem(seed, n=SEARCH_N)
        Xc = (T_true[:3, :3] @ Xw.T).T + T_true[:3, 3]
        Xc[::5, 2] = -120.0
        Xw2 = (T_true[:3, :3].T @ (Xc - T_true[:3, 3]).T).T
        out.append(case(orc, "behind", BITWISE, Xw2, obs, K, np.eye(4), twin=True))
    # n = 2 and n = 3 (rank-deficient / barely determined systems), and the chunk boundaries of the device's build
    for n in (2, 3, 127, 128, 129, 192, 193, 256, 320, 321):
        for seed in range(500, 700):
            Xw, obs, K, T_true = util.pose_problem(seed, n=n, outlier_frac=0.0 if n < 5 else 0.2)
            T0 = np.eye(4) if n < 5 else offset_start(T_true, np.random.default_rng(200000 + seed))
            w = walk(orc, Xw, obs, K, T0)
            if w["counts"][2] == 0 and np.isfinite(w["stats_f"]).all() and (n < 5 or (w["trials"].max() >= 2 and w["stats_i"][1] >= 3)):
                if twin_difference(Xw, obs, K, T0, w)[0]:
                    out.append(case(orc, "n %d" % n, BITWISE, Xw, obs, K, T0, twin=True))
                    break
        else:
            raise SystemExit("no case for n = %d" % n)
    # starts 40 degrees off: SE3Quat::exp on libm's sin / cos, not bit-comparable - recorded with the twin's distance
    # (kept where a step of the LM does reach 0.5 rad - most starts are walked back in smaller steps - and the twin takes the same branches)
    n_large = 0
    for seed in range(420, 1420):
        Xw, obs, K, T_true = util.pose_problem(seed, n=SEARCH_N)
        w3 = np.zeros(3); w3[seed % 3] = np.deg2rad(40.0)
        T0 = rigid(rodrigues(w3)) @ T_true
        w = walk(orc, Xw, obs, K, T0)
        if w["counts"][2] > 0 and np.isfinite(w["stats_f"]).all() and twin_difference(Xw, obs, K, T0, w)[0]:
            out.append(case(orc, "large rotation", LARGE_ROTATION, Xw, obs, K, T0, twin=True))
            n_large += 1
            if n_large == 3:
                break
    # a depth of exactly zero under the start pose: a point at the camera centre (0 / 0), a point at (1, 0.5, 0) (1 / 0)
    for tag, p in (("depth zero centre", (0.0, 0.0, 0.0)), ("depth zero plane", (1.0, 0.5, 0.0))):
        Xw, obs, K, T_true = util.pose_problem(430, n=16, outlier_frac=0.0)
        Xw[5] = p
        out.append(case(orc, tag, DEPTH_ZERO, Xw, obs, K, np.eye(4)))
    return out


def pack(cases):
    off = np.cumsum([0] + [len(c["Xw"]) for c in cases]).astype(np.int32)
    g = {"tag": np.array([c["tag"] for c in cases]), "kind": np.array([c["kind"] for c in cases], np.int32), "off": off,
         "Xw": np.concatenate([c["Xw"] for c in cases]), "obs": np.concatenate([c["obs"] for c in cases]),
         "K": np.stack([c["K"] for c in cases]), "T0": np.stack([c["T0"] for c in cases]), "T": np.stack([c["T"] for c in cases]),
         "stats_i": np.stack([c["stats_i"] for c in cases]), "stats_f": np.stack([c["stats_f"] for c in cases]),
         "counts": np.stack([c["counts"] for c in cases]).astype(np.int32), "trials": np.stack([c["trials"] for c in cases]),
         "stop": np.array([c["stop"] for c in cases], np.int32), "failed_solves": np.array([c["failed_solves"] for c in cases], np.int32),
         "twin_dT": np.array([c["twin_dT"] for c in cases]), "twin_dchi": np.array([c["twin_dchi"] for c in cases])}
    return g


def unpack(g):
    """The fixture as a list of cases (what the tests iterate over)."""
    out = []
    for i in range(len(g["tag"])):
        a, b = int(g["off"][i]), int(g["off"][i + 1])
        c = {k: g[k][i] for k in ("kind", "K", "T0", "T", "stats_i", "stats_f", "counts", "trials", "stop", "failed_solves", "twin_dT", "twin_dchi")}
        c["tag"] = str(g["tag"][i]); c["Xw"] = g["Xw"][a:b]; c["obs"] = g["obs"][a:b]
        out.append(c)
    return out


def coverage(cases):
    """What the fixture has to hold, proven from the restatement's own records; returns the figures, raises on a shortfall."""
    def count(pred, kinds=(BITWISE,)):
        return sum(1 for c in cases if c["kind"] in kinds and pred(c))
    out = {}
    out["2 trials in one iteration"] = count(lambda c: (c["trials"] == 2).any())
    out["3..5 trials in one iteration"] = count(lambda c: ((c["trials"] >= 3) & (c["trials"] <= 5)).any())
    out["6..9 trials in one iteration"] = count(lambda c: ((c["trials"] >= 6) & (c["trials"] <= 9)).any())
    out["stop on qmax == 10"] = count(lambda c: c["stop"] == STOPS["qmax"] and c["trials"][c["stats_i"][1] - 1] == 10 and c["stats_i"][3] == 1)
    out["ten iterations, not terminated"] = count(lambda c: c["stats_i"][1] == 10 and c["stats_i"][3] == 0 and c["stop"] == STOPS["ten"])
    out["stop on nBad >= 3"] = count(lambda c: c["stop"] == STOPS["nbad"] and c["stats_i"][3] == 1)
    out["stop on rho == 0, exact data"] = count(lambda c: c["tag"] == "stop rho0 exact" and c["stop"] == STOPS["rho0"] and tuple(c["stats_i"][1:]) == (1, 1, 1)
                                                and c["stats_f"][1] == 0.0)
    out["restart: theta < 1e-5"] = count(lambda c: c["tag"] == "restart" and c["counts"][0] > 0)
    for k in out:
        assert out[k] >= 2, (k, out)
    for axis in range(3):
        key = "largest diagonal %d (start turned by 170 degrees)" % axis
        out[key] = count(lambda c: c["tag"].startswith("rot170") and c["counts"][4 + axis] > 0 and np.trace(c["T0"][:3, :3]) < -0.9)
        assert out[key] >= 2, (key, out)
    out["q.w < 0 before the flip"] = count(lambda c: c["tag"].startswith("rot170") and c["counts"][7] > 0)
    assert out["q.w < 0 before the flip"] >= 1, out
    out["every edge on Huber's linear branch"] = count(lambda c: c["tag"] == "huber linear" and all_linear(c))
    out["a fifth of the points behind the camera"] = count(lambda c: c["tag"] == "behind" and (depths(c, c["T0"]) < -100).sum() == (len(c["Xw"]) + 4) // 5)
    assert out["every edge on Huber's linear branch"] >= 2 and out["a fifth of the points behind the camera"] >= 2, out
    for n in (2, 3, 127, 128, 129, 192, 193, 256, 320, 321):
        out["n = %d" % n] = count(lambda c: len(c["Xw"]) == n and c["stats_i"][0] == n)
        assert out["n = %d" % n] >= 1, (n, out)
    out["bitwise cases on libm"] = count(lambda c: c["counts"][2] != 0)
    assert out["bitwise cases on libm"] == 0, out
    out["bitwise cases beyond 64 edges without need"] = count(lambda c: len(c["Xw"]) > 64 and not c["tag"].startswith("n "))
    assert out["bitwise cases beyond 64 edges without need"] == 0, out
    out["large rotation (libm counter > 0)"] = count(lambda c: c["counts"][2] > 0 and np.isfinite(c["twin_dT"]) and np.isfinite(c["twin_dchi"]), (LARGE_ROTATION,))
    assert out["large rotation (libm counter > 0)"] >= 3, out
    out["depth zero"] = count(lambda c: (depths(c, c["T0"]) == 0).sum() == 1, (DEPTH_ZERO,))
    assert out["depth zero"] == 2 and {c["tag"] for c in cases if c["kind"] == DEPTH_ZERO} == {"depth zero centre", "depth zero plane"}, out
    return out


def depths(c, T):
    return (T[:3, :3] @ c["Xw"].T).T[:, 2] + T[2, 3]


def all_linear(c):
    """every edge beyond Huber's delta^2 = 5.991 at the start and at the result (plain numpy reprojection; the margin is hundreds of px)"""
    for T in (c["T0"], c["T"]):
        pc = (T[:3, :3] @ c["Xw"].T).T + T[:3, 3]
        e0 = c["obs"][:, 0] - (pc[:, 0] / pc[:, 2] * c["K"][0] + c["K"][2]); e1 = c["obs"][:, 1] - (pc[:, 1] / pc[:, 2] * c["K"][1] + c["K"][3])
        if not (e0 * e0 + e1 * e1 > 100.0).all():
            return False
    return True


def write_npz(path, g):
    """np.savez with fixed member order and dates: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for k in sorted(g):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(g[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def main():
    from oracle import binding as orc
    import util
    found, missing, seeds = searched(orc, util)
    print("seeded search: %d problems of %d edges walked, missing: %s" % (seeds, SEARCH_N, missing or "nothing"))
    cases = found + built(orc, util)
    for key, v in coverage(cases).items():
        print("%-52s %d" % (key, v))
    for c in cases:
        print("%-20s n %3d  iterations %2d  trials %-22s stop %d  failed solves %2d  counts %s  twin dT %.2e dchi %.2e" %
              (c["tag"], len(c["Xw"]), c["stats_i"][1], "".join("%d," % t for t in c["trials"][:c["stats_i"][1]]), c["stop"], c["failed_solves"],
               c["counts"].tolist(), c["twin_dT"], c["twin_dchi"]))
    write_npz(PATH, pack(cases))
    size = os.path.getsize(PATH)
    assert size <= MAX_BYTES, size
    back = unpack(np.load(PATH))
    assert len(back) == len(cases) and all(a["T"].tobytes() == b["T"].tobytes() for a, b in zip(back, cases))
    print("%d cases (%d bytes) -> %s" % (len(cases), size, PATH))


if __name__ == "__main__":
    main()
