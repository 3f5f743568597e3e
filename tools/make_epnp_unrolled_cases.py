"""Writes tests/golden/epnp5_unrolled_cases.npy, the fixture of tests/test_epnp_unrolled_gpu.py: five-point EPnP samples and what the
CPU restatement (oracle/orc_pnp_cv.c) makes of them, chosen so that the 12 x 12 decomposition's unrolled step loop
(tools/gen_jacobi_asm.py) is left after several different numbers of sweeps, plus an exactly coplanar sample and - if the search
finds one - a sample whose decomposition leaves the range of the loop's unscaled divisions (a singular value outside
[2^-100, 2^100], or 25 sweeps without convergence).  Needs no GPU:  python tools/make_epnp_unrolled_cases.py"""
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
                 ("sweeps", "<i4"), ("kind", "<i4")])      # kind 0 ordinary, 1 exactly coplanar, 2 out of range
ORDINARY, SEARCH = 240, 100000


def shim():
    so = os.path.join(tempfile.mkdtemp(), "epnp_sweeps_shim.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-D_GNU_SOURCE", "-w",
                           "-I", os.path.join(ROOT, "include"), "-o", so, os.path.join(ROOT, "tools", "epnp_sweeps_shim.c"), "-lm"])
    lib = C.CDLL(so)
    p = C.POINTER(C.c_double)
    lib.shim_epnp5_sweeps12.argtypes = [p, p, p, p, p]
    lib.shim_epnp5_sweeps12.restype = C.c_int

    def sweeps12(X5, u5):
        X5 = np.ascontiguousarray(X5, np.float64).reshape(15); u5 = np.ascontiguousarray(u5, np.float64).reshape(10)
        w, cc = np.zeros(12), np.zeros(3)
        n = lib.shim_epnp5_sweeps12(*(a.ctypes.data_as(p) for a in (X5, u5, K, w, cc)))
        return n, w, cc
    return sweeps12


def in_range(w):
    return bool(np.all((w >= 2.0 ** -100) & (w <= 2.0 ** 100)))


def degenerate(cc):
    """The control points' 3 x 3 problem needs the sequential finish: a singular value out of range (zero) or two equal ones."""
    return not in_range(cc) or len(set(cc.tolist())) < 3


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


def main():
    sweeps12 = shim()
    rng = np.random.default_rng(2024)
    P = pools()
    rep_o = (C.c_double * 3).in_dll(orc.lib(), "orc_epnp_last_rep")
    cases, found_out = [], None
    hist = {}
    for i in range(SEARCH):
        Xw, obs = P[i % len(P)]
        idx = rng.choice(len(Xw), 5, replace=False)
        n, w, cc = sweeps12(Xw[idx], obs[idx])
        if degenerate(cc):
            continue
        out = n >= 25 or not in_range(w)
        hist[n] = hist.get(n, 0) + 1
        if out and found_out is None:
            found_out = (Xw[idx], obs[idx], n, 2)
        elif not out and len(cases) < ORDINARY:
            cases.append((Xw[idx], obs[idx], n, 0))
        elif not out and sum(1 for c in cases if c[2] == n) < 3:      # rare sweep counts met later in the search
            cases.append((Xw[idx], obs[idx], n, 0))
    # exactly coplanar: every world point on the plane Z = 20
    Xw, obs, Kc, T = util.pose_problem(3, n=60, outlier_frac=0.1)
    Xw = Xw.copy(); Xw[:, 2] = 20.0
    Xc = (T[:3, :3] @ Xw.T).T + T[:3, 3]
    obs = np.stack([Kc[0] * Xc[:, 0] / Xc[:, 2] + Kc[2], Kc[1] * Xc[:, 1] / Xc[:, 2] + Kc[3]], 1).astype(np.float32).astype(np.float64)
    for _ in range(2):
        idx = rng.choice(60, 5, replace=False)
        n, w, cc = sweeps12(Xw[idx], obs[idx])
        assert degenerate(cc)
        cases.append((Xw[idx], obs[idx], n, 1))
    if found_out is not None:
        cases.append(found_out)
    arr = np.zeros(len(cases), CASE)
    for a, (X5, u5, n, kind) in zip(arr, cases):
        R, t = orc.epnp5(X5, u5, K)
        a["X"], a["u"], a["R"], a["t"], a["rep"], a["sweeps"], a["kind"] = X5, u5, R, t, np.array(list(rep_o)), n, kind
    path = os.path.join(ROOT, "tests", "golden", "epnp5_unrolled_cases.npy")
    np.save(path, arr)
    print("sweeps of the 12 x 12 decomposition over %d non-degenerate tries: %s" % (sum(hist.values()), sorted(hist.items())))
    print("out-of-range sample: %s" % ("none found" if found_out is None else "sweeps %d" % found_out[2]))
    print("%d cases (%d bytes) -> %s; sweep counts in the fixture: %s" % (len(arr), os.path.getsize(path), path,
                                                                        sorted(set(arr["sweeps"][arr["kind"] == 0].tolist()))))


if __name__ == "__main__":
    main()
