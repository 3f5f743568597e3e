"""Writes tests/golden/jacobi12_cases.npy, the fixture of tests/test_jacobi12_resched_cpu.py and tests/test_jacobi12_resched_gpu.py: 12 x 12
matrices for the wave engine's M = 12 step loop (jacobi_rows<12>, block EO_JACOBI_ASM_12 of tools/gen_jacobi_asm.py) with what
JacobiSVDImpl_'s sequential sweeps (tools/jacobi12_shim.c) make of them: the rows (scaled by 1 / W), W and the number of sweeps.
Groups (field `group`):
  a  M^T M of seeded five-point samples, several different sweep counts
  b  a diagonal matrix: no pair ever rotates, the speculative first division of a step sees p = 0
  c  a multiple of the identity: beta = 0 and p = 0 - the discarded speculation computes 0 / 0
  d  2 x 2 blocks with beta < 0, beta > 0, beta == 0 and |2p| == |beta|, each also mirrored, on the pairs (2k, 2k + 1) and (k, 11 - k)
  e  exactly one pair rotates per sweep: (0, 1), (5, 6), (10, 11)
  f  a pair inside the 2^-40 margin of the rotation threshold (found by bisection with the shim), resolved to "rotate" and to
     "leave", on a pair of sum 11, on one of sum 13 (steps 10 and 12 of the schedule: copies of the period) and on the pair (3, 4)
     (step 6: a copy of the prologue)
  g  a matrix with a NaN, and one with a singular value below 2^-100 (excused from the bitwise comparison: the caller acts on the
     flag / the out-of-range value)
Needs no GPU:  python tools/make_jacobi12_cases.py"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K = np.array([718.856, 718.856, 607.1928, 185.2157])
CASE = np.dtype([("At", "<f8", (12, 12)), ("rows", "<f8", (12, 12)), ("W", "<f8", 12), ("sweeps", "<i4"), ("rotations", "<i4"),
                 ("und_rotate", "<i4"), ("und_leave", "<i4"), ("und_first", "<i4", 3), ("group", "S1")])
EPS = 2.220446049250313e-16 * 10
SAMPLES, PER_COUNT = 30, 10


def shim():
    so = os.path.join(tempfile.mkdtemp(), "jacobi12_shim.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-D_GNU_SOURCE", "-w",
                           "-I", os.path.join(ROOT, "include"), "-o", so, os.path.join(ROOT, "tools", "jacobi12_shim.c"), "-lm"])
    lib = C.CDLL(so)
    p, pi = C.POINTER(C.c_double), C.POINTER(C.c_int)
    lib.shim_jacobi12_mtm.argtypes = [p, p, p, p]
    lib.shim_jacobi12_mtm.restype = None
    lib.shim_jacobi12_sweeps.argtypes = [p, p, p, pi]
    lib.shim_jacobi12_sweeps.restype = C.c_int

    def mtm(X5, u5):
        X5 = np.ascontiguousarray(X5, np.float64).reshape(15); u5 = np.ascontiguousarray(u5, np.float64).reshape(10)
        At = np.zeros(144)
        lib.shim_jacobi12_mtm(*(a.ctypes.data_as(p) for a in (X5, u5, K, At)))
        return At.reshape(12, 12)

    def sweeps(At):
        work = np.ascontiguousarray(At, np.float64).reshape(144).copy()
        rows, w, und = np.zeros(144), np.zeros(12), np.zeros(6, np.int32)
        with np.errstate(all="ignore"):
            n = lib.shim_jacobi12_sweeps(work.ctypes.data_as(p), rows.ctypes.data_as(p), w.ctypes.data_as(p), und.ctypes.data_as(pi))
        return n, rows.reshape(12, 12), w, und
    return mtm, sweeps


def diag():
    return np.diag(1.0 + np.arange(12) / 16.0)


def with_block(A, i, j, a, b, c):
    A = A.copy()
    A[i, i], A[j, j], A[i, j], A[j, i] = a, b, c, c
    return A


def blocks(pairs):
    """Six 2 x 2 blocks [[a, c], [c, b]]: with rows (a, c) and (c, b), p = c (a + b) and beta = a^2 - b^2."""
    kinds = [(1.0, 2.0, 0.25),      # beta < 0
             (2.0, 1.0, 0.25),      # beta > 0
             (1.5, 1.5, 0.125),     # beta == 0
             (3.0, 1.0, 1.0),       # 2p = 8 = beta
             (1.0, 3.0, 1.0),       # 2p = 8 = -beta
             (1.5, 1.5, -0.125)]    # beta == 0, p < 0
    A = np.zeros((12, 12))
    for (i, j), (a, b, c) in zip(pairs, kinds):
        A = with_block(A, i, j, a, b, c)
    return A


def margin_pair(sweeps, i, j):
    """Two matrices - diagonal but for the pair (i, j) - whose off-diagonal element lies one ulp to either side of the rotation
    threshold: the pair test is inside the 2^-40 margin in both, one rotates, one does not."""
    D = diag()
    a, b = D[i, i], D[j, j]
    c0 = EPS * a * b / (a + b)
    lo, hi = np.float64(c0 * (1 - 1e-6)).view(np.int64), np.float64(c0 * (1 + 1e-6)).view(np.int64)

    def rotates(bits):
        return sweeps(with_block(D, i, j, a, b, np.int64(bits).view(np.float64)))[3][5] > 0
    assert not rotates(lo) and rotates(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if rotates(mid):
            hi = mid
        else:
            lo = mid
    out = []
    for bits, want in ((hi, 0), (lo, 1)):
        A = with_block(D, i, j, a, b, np.int64(bits).view(np.float64))
        n, rows, w, und = sweeps(A)
        assert und[want] >= 1 and tuple(und[2:5]) == (0, i, j), (i, j, und)     # the generator asserts both resolutions
        out.append(A)
    return out


def main():
    import util                                   # noqa: E402  (tests/util.py: the seeded pose problems)
    mtm, sweeps = shim()
    cases = []
    # (a) seeded five-point samples
    rng = np.random.default_rng(2025)
    per, tried = {}, 0
    pools = [util.pose_problem(seed, n=60, outlier_frac=0.1, sigma=(0.0, 0.5, 1.5)[seed % 3])[:2] for seed in range(12)]
    while sum(len(v) for v in per.values()) < SAMPLES and tried < 20000:
        Xw, obs = pools[tried % len(pools)]
        tried += 1
        idx = rng.choice(len(Xw), 5, replace=False)
        At = mtm(Xw[idx], obs[idx])
        n, rows, w, und = sweeps(At)
        if n >= 25 or not np.all((w >= 2.0 ** -100) & (w <= 2.0 ** 100)) or len(set(w.tolist())) < 12:
            continue
        if len(per.setdefault(n, [])) < PER_COUNT:
            per[n].append(At)
    assert len(per) >= 3, sorted(per)
    cases += [(At, b"a") for n in sorted(per) for At in per[n]]
    # (b), (c)
    cases.append((diag(), b"b"))
    cases.append((3.0 * np.eye(12), b"c"))
    # (d)
    cases.append((blocks([(2 * k, 2 * k + 1) for k in range(6)]), b"d"))
    cases.append((blocks([(k, 11 - k) for k in range(6)]), b"d"))
    # (e)
    for i, j in ((0, 1), (5, 6), (10, 11)):
        A = with_block(diag(), i, j, 1.0 + i / 16.0, 1.0 + j / 16.0, 0.375)
        cases.append((A, b"e"))
    # (f)
    for i, j in ((5, 6), (6, 7), (3, 4)):
        cases += [(A, b"f") for A in margin_pair(sweeps, i, j)]
    # (g)
    A = diag(); A[3, 7] = A[7, 3] = np.nan
    cases.append((A, b"g"))
    A = diag(); A[4, 4] = 2.0 ** -120
    cases.append((A, b"g"))
    assert len(cases) <= 64
    arr = np.zeros(len(cases), CASE)
    for rec, (At, group) in zip(arr, cases):
        n, rows, w, und = sweeps(At)
        rec["At"], rec["rows"], rec["W"], rec["sweeps"], rec["rotations"] = At, rows, w, n, und[5]
        rec["und_rotate"], rec["und_leave"], rec["und_first"], rec["group"] = und[0], und[1], und[2:5], group
        if group == b"e":
            assert n >= 2 and und[5] == n - 1, (n, und)          # one rotation in every sweep but the last
        if group in (b"b", b"c"):
            assert n == 1 and und[5] == 0
    path = os.path.join(ROOT, "tests", "golden", "jacobi12_cases.npy")
    np.save(path, arr)
    print("%d cases (%d bytes) -> %s" % (len(arr), os.path.getsize(path), path))
    for g in b"abcdefg":
        sel = arr[arr["group"] == bytes([g])]
        print("  %s: %d matrices, sweeps %s, rotations %s, inside the margin (rotate / leave) %s" % (
            chr(g), len(sel), sorted(set(sel["sweeps"].tolist())), sel["rotations"].tolist() if len(sel) < 8 else "...",
            list(zip(sel["und_rotate"].tolist(), sel["und_leave"].tolist())) if len(sel) < 8 else "..."))


if __name__ == "__main__":
    main()
