"""Writes tests/golden/epnp5_small_cases.npy, the fixture of tests/test_epnp_small_gpu.py: five-point EPnP samples and what the CPU
restatement (oracle/orc_pnp_cv.c) makes of them, chosen so that each of the five 3 x 3 decompositions of a solve (control points,
cvInvert(CC), the three candidates' ABt - the step loop EO_JACOBI_ASM_3R of tools/gen_jacobi_asm.py) is left after several
different numbers of sweeps and the three ABt problems, which run side by side, stop in different sweeps (one leaves the loop while
another goes on; three pairwise different sweep counts are taken where the search meets them); plus an exactly coplanar
sample (a zero singular value) and one with two equal singular values of PW0^T PW0.  Needs no GPU:
python tools/make_epnp_small_cases.py"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import util                                   # noqa: E402
from oracle import binding as orc             # noqa: E402

K = np.array([718.856, 718.856, 607.1928, 185.2157])
CASE = np.dtype([("X", "<f8", (5, 3)), ("u", "<f8", (5, 2)), ("R", "<f8", (3, 3)), ("t", "<f8", 3), ("rep", "<f8", 3),
                 ("sweeps", "<i4", 5), ("kind", "<i4")])   # sweeps: control points, CC, ABt 1..3; kind 0 ordinary, 1 coplanar, 2 equal values
NAMES = ("control points", "cvInvert(CC)", "ABt 1", "ABt 2", "ABt 3")
SEARCH, PER_COUNT, SPLIT, MAX_CASES = 200000, 6, 40, 400


def shim():
    so = os.path.join(tempfile.mkdtemp(), "epnp_small_shim.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-D_GNU_SOURCE", "-w",
                           "-I", os.path.join(ROOT, "include"), "-o", so, os.path.join(ROOT, "tools", "epnp_small_shim.c"), "-lm"])
    lib = C.CDLL(so)
    p = C.POINTER(C.c_double)
    lib.shim_epnp5_small.argtypes = [p, p, p, C.POINTER(C.c_int), p]
    lib.shim_epnp5_small.restype = C.c_int

    def small(X5, u5):
        X5 = np.ascontiguousarray(X5, np.float64).reshape(15); u5 = np.ascontiguousarray(u5, np.float64).reshape(10)
        w, sw = np.zeros(15), np.zeros(5, np.int32)
        eq = lib.shim_epnp5_small(X5.ctypes.data_as(p), u5.ctypes.data_as(p), K.ctypes.data_as(p), sw.ctypes.data_as(C.POINTER(C.c_int)), w.ctypes.data_as(p))
        return sw, w.reshape(5, 3), bool(eq)
    return small


def ordinary(w):
    """No problem of the sample needs the sequential finish: singular values in [2^-100, 2^100], all different."""
    return bool(np.all((w >= 2.0 ** -100) & (w <= 2.0 ** 100))) and all(len(set(r.tolist())) == 3 for r in w)


def pools():
    """Seeded point sets to draw five-point samples from: ordinary, three kilometres from the origin, every correspondence twice."""
    out = []
    for seed in range(40):
        Xw, obs, _, _ = util.pose_problem(seed, n=60, outlier_frac=0.1, sigma=(0.0, 0.5, 1.5)[seed % 3])
        if seed % 4 == 1:
            Xw = (Xw + np.array([900.0, 2.0, 3000.0])).astype(np.float32).astype(np.float64)
        if seed % 4 == 3:
            Xw = np.repeat(Xw[:30], 2, axis=0); obs = np.repeat(obs[:30], 2, axis=0)
        out.append((Xw, obs))
    return out


def project(Xw, T, Kc):
    Xc = (T[:3, :3] @ Xw.T).T + T[:3, 3]
    return np.stack([Kc[0] * Xc[:, 0] / Xc[:, 2] + Kc[2], Kc[1] * Xc[:, 1] / Xc[:, 2] + Kc[3]], 1).astype(np.float32).astype(np.float64)


def main():
    small = shim()
    rng = np.random.default_rng(2025)
    P = pools()
    rep_o = (C.c_double * 3).in_dll(orc.lib(), "orc_epnp_last_rep")
    cases, split, apart = [], 0, 0
    have = [dict() for _ in range(5)]       # per problem: sweep count -> cases that show it
    hist = [dict() for _ in range(5)]
    for i in range(SEARCH):
        Xw, obs = P[i % len(P)]
        idx = rng.choice(len(Xw), 5, replace=False)
        sw, w, _ = small(Xw[idx], obs[idx])
        if not ordinary(w) or sw.max() >= 25:
            continue
        for p in range(5):
            hist[p][int(sw[p])] = hist[p].get(int(sw[p]), 0) + 1
        nabt = len(set(sw[2:].tolist()))                   # 2: one ABt problem leaves the loop while another goes on; 3: all three apart
        rare = any(have[p].get(int(sw[p]), 0) < PER_COUNT for p in range(5))
        if len(cases) < MAX_CASES - 8 and (rare or (nabt == 2 and split < SPLIT) or (nabt == 3 and apart < SPLIT)):
            cases.append((Xw[idx], obs[idx], sw, 0))
            split += nabt >= 2
            apart += nabt == 3
            for p in range(5):
                have[p][int(sw[p])] = have[p].get(int(sw[p]), 0) + 1
    # exactly coplanar: every world point on the plane Z = 20 (a zero singular value of PW0^T PW0)
    Xw, obs, Kc, T = util.pose_problem(3, n=60, outlier_frac=0.1)
    Xw = Xw.copy(); Xw[:, 2] = 20.0
    obs = project(Xw, T, Kc)
    idx = rng.choice(60, 5, replace=False)
    sw, w, _ = small(Xw[idx], obs[idx])
    assert w[0].min() == 0.0
    cases.append((Xw[idx], obs[idx], sw, 1))
    # two equal singular values of PW0^T PW0: a point set symmetric in x and y about its centroid (every difference exact)
    Xs = np.array([[3.0, 2.0, 20.0], [-1.0, 2.0, 20.0], [1.0, 4.0, 20.0], [1.0, 0.0, 20.0], [1.0, 2.0, 25.0]])
    us = project(Xs, T, Kc)
    sw, w, eq = small(Xs, us)
    assert eq and sorted(w[0].tolist()) == [8.0, 8.0, 20.0], (eq, w[0])
    cases.append((Xs, us, sw, 2))
    arr = np.zeros(len(cases), CASE)
    for a, (X5, u5, sw, kind) in zip(arr, cases):
        R, t = orc.epnp5(X5, u5, K)
        a["X"], a["u"], a["R"], a["t"], a["rep"], a["sweeps"], a["kind"] = X5, u5, R, t, np.array(list(rep_o)), sw, kind
    path = os.path.join(ROOT, "tests", "golden", "epnp5_small_cases.npy")
    np.save(path, arr)
    for p in range(5):
        print("%-14s sweeps over the ordinary tries: %s; in the fixture: %s" % (NAMES[p], sorted(hist[p].items()), sorted(have[p].items())))
    print("%d cases (%d bytes) -> %s; the three ABt problems do not stop in the same sweep in %d of them (three different sweeps: %d)" %
          (len(arr), os.path.getsize(path), path, split, apart))


if __name__ == "__main__":
    main()
