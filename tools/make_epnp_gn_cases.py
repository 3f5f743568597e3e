"""Writes tests/golden/epnp_gn_cases.npy, the fixture of tests/test_epnp_gn_cpu.py and tests/test_epnp_gn_gpu.py: inputs of
epnp::gauss_newton - L (6 x 10), rho, the betas of three candidates (candidate 0 general, candidate 1 of shape 2: betas[2] =
betas[3] = 0, candidate 2 of shape 3: betas[3] = 0, as compute_pose hands them over) - with what the CPU restatement
(oracle/orc_pnp_cv.c through tools/epnp_gn_shim.c) makes of them and the branches its five iterations took.  Chosen so that
every branch of qr_solve is met in every Householder step, the candidates (which a wave runs side by side) part ways, and the
quirks of its `eta` scan show; the conditions are checked at the end (coverage(), shared with the CPU test) and the script fails if
one is not met.  Needs no GPU:  python tools/make_epnp_gn_cases.py"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = np.dtype([("L", "<f8", (6, 10)), ("rho", "<f8", 6), ("bin", "<f8", (3, 4)), ("bout", "<f8", (3, 4)),
                 ("cnt", "u1", (3, 5, 4, 4)),    # [candidate][iteration][k]: negative pivot, eta from below the diagonal, eta == 0, |A[5][k]| >= 1e6 eta
                 ("kind", "<i4")])
KINDS = {0: "seeded", 1: "L scaled by 1e-3", 2: "small-integer L", 3: "all betas zero", 4: "one candidate's betas zero",
         5: "betas reach zero after the first iteration", 6: "columns 6..9 of L zero", 7: "the fourth column zero in one candidate only",
         8: "row 5 of L dominates", 9: "infinity in L", 10: "NaN in L"}
PATH = os.path.join(ROOT, "tests", "golden", "epnp_gn_cases.npy")
MAX_CASES = 400


def shim():
    so = os.path.join(tempfile.mkdtemp(), "epnp_gn_shim.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-D_GNU_SOURCE", "-w",
                           "-I", os.path.join(ROOT, "include"), "-o", so, os.path.join(ROOT, "tools", "epnp_gn_shim.c"), "-lm"])
    lib = C.CDLL(so)
    p = C.POINTER(C.c_double)
    lib.shim_gn.argtypes = [p, p, p]
    lib.shim_gn_cols.argtypes = [p, p, p]
    lib.shim_gn_count.argtypes = [p, p, p, C.POINTER(C.c_ubyte)]
    lib.shim_gn_count.restype = C.c_int
    lib.shim_gn_many.argtypes = [C.c_int, C.c_int, p, p, p]
    lib.shim_gn.restype = lib.shim_gn_cols.restype = lib.shim_gn_many.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def walk(lib, L, rho, betas, fn="shim_gn"):
    """gauss_newton (or the column-ordered walk) on one system: the new betas."""
    L = np.ascontiguousarray(L, np.float64); rho = np.ascontiguousarray(rho, np.float64); b = np.array(betas, np.float64)
    getattr(lib, fn)(_p(L), _p(rho), _p(b))
    return b


def record(lib, L, rho, bin3, kind):
    a = np.zeros((), CASE)
    a["L"], a["rho"], a["bin"], a["kind"] = L, rho, bin3, kind
    for c in range(3):
        b = np.array(a["bin"][c]); cnt = np.zeros((5, 4, 4), np.uint8)
        differs = lib.shim_gn_count(_p(np.ascontiguousarray(a["L"])), _p(np.ascontiguousarray(a["rho"])), _p(b), cnt.ctypes.data_as(C.POINTER(C.c_ubyte)))
        ref = walk(lib, a["L"], a["rho"], a["bin"][c])
        assert not differs and ref.tobytes() == b.tobytes(), "the counting walk left gauss_newton's bits"
        a["bout"][c], a["cnt"][c] = ref, cnt
    return a


def shapes(rng, scale=1.0):
    """The three candidates' start values, in the shapes find_betas_approx_1 / _2 / _3 leave."""
    b = rng.normal(size=(3, 4)) * scale
    b[1, 2:] = 0.0
    b[2, 3] = 0.0
    return b


def sign_split(cnt):
    """A step all three candidates reach in which one takes the negative-pivot branch and another does not."""
    reached = np.cumsum(cnt[..., 2], axis=2) - cnt[..., 2] == 0            # [c][it][k]: no eta == 0 earlier in this iteration
    reached &= cnt[..., 2] == 0
    allr = reached.all(axis=0)
    neg = cnt[..., 0]
    return bool((allr & (neg.max(axis=0) != neg.min(axis=0))).any())


def alive_split(cnt):
    """An iteration in which one candidate meets eta == 0 and another does not."""
    dead = cnt[..., 2].any(axis=2)                                         # [c][it]
    return bool((dead.max(axis=0) != dead.min(axis=0)).any())


def coverage(arr):
    """What the fixture has to hold; returns the figures, raises on a shortfall."""
    cnt = arr["cnt"].astype(np.int64)                                       # [n][c][it][k][4]
    per_sys = cnt.any(axis=(1, 2))                                          # [n][k][4]: the system meets the branch at k
    out = {}
    for k in range(4):
        out["negative pivot at k=%d" % k] = int(per_sys[:, k, 0].sum())
        out["eta from below the diagonal at k=%d" % k] = int(per_sys[:, k, 1].sum())
        assert out["negative pivot at k=%d" % k] >= 10 and out["eta from below the diagonal at k=%d" % k] >= 10, out
    first = cnt[:, :, 0]                                                    # first iteration [n][c][k][4]
    out["eta == 0 at k=0, all candidates, first iteration"] = int((first[:, :, 0, 2] == 1).all(axis=1).sum())
    out["eta == 0 at k=0 in one candidate only"] = int(((cnt[:, :, :, 0, 2].any(axis=2)).sum(axis=1) == 1).sum())
    out["eta == 0 at k=0 in a later iteration only"] = int(((first[:, :, 0, 2] == 0) & cnt[:, :, 1:, 0, 2].any(axis=2)).any(axis=1).sum())
    out["eta == 0 at k=3, all candidates, first iteration"] = int((first[:, :, 3, 2] == 1).all(axis=1).sum())
    out["eta == 0 at k=3 in one candidate only"] = int(((cnt[:, :, :, 3, 2].any(axis=2)).sum(axis=1) == 1).sum())
    for key in list(out)[8:]:
        assert out[key] >= 1, (key, out)
    assert (arr["bin"][:, 1, 2:] == 0).all() and (arr["bin"][:, 2, 3] == 0).all()
    out["candidates of shape 2 and 3 with non-zero betas"] = int(((arr["bin"][:, 1, :2] != 0).all(axis=1) & (arr["bin"][:, 2, :3] != 0).all(axis=1)).sum())
    assert out["candidates of shape 2 and 3 with non-zero betas"] >= 20
    s = np.array([sign_split(c) for c in arr["cnt"]]); a = np.array([alive_split(c) for c in arr["cnt"]])
    out["candidates part ways on the pivot's sign"], out["candidates part ways on eta == 0"] = int(s.sum()), int(a.sum())
    assert (s | a).sum() >= 20 and s.sum() >= 10 and a.sum() >= 3, out
    out["row 5 holds the pivot column's largest entry by 1e6"] = int(per_sys[:, :, 3].any(axis=1).sum())
    assert out["row 5 holds the pivot column's largest entry by 1e6"] >= 5, out
    nonfin = ~np.isfinite(arr["L"]).all(axis=(1, 2))
    out["infinity or NaN in L"] = int(nonfin.sum())
    assert nonfin.sum() >= 2 and np.isinf(arr["L"]).any() and np.isnan(arr["L"]).any()
    assert not np.isfinite(arr["bout"][nonfin]).all(axis=(1, 2)).any(), "a non-finite L left finite betas"
    assert len(arr) <= MAX_CASES
    return out


def main():
    lib = shim()
    rng = np.random.default_rng(2026)
    cases = []
    # seeded systems: rho consistent with betas near the start values (the iterations converge) or not at all
    for i in range(150):
        kind = (0, 0, 1, 2)[i % 4]
        L = rng.normal(size=(6, 10))
        if kind == 1:
            L *= 1e-3
        if kind == 2:
            L = rng.integers(-4, 5, size=(6, 10)).astype(np.float64)
        b3 = shapes(rng)
        if i % 3 == 0:
            rho = rng.normal(size=6)
        else:
            bt = b3[0] + 0.1 * rng.normal(size=4)
            q = np.array([bt[0] * bt[0], bt[0] * bt[1], bt[1] * bt[1], bt[0] * bt[2], bt[1] * bt[2], bt[2] * bt[2], bt[0] * bt[3], bt[1] * bt[3], bt[2] * bt[3], bt[3] * bt[3]])
            rho = L @ q
        cases.append(record(lib, L, rho, b3, kind))
    # A = 0 at once: all betas zero, in every candidate / in one candidate only
    for i in range(2):
        cases.append(record(lib, rng.normal(size=(6, 10)), rng.normal(size=6), np.zeros((3, 4)), 3))
    for c in range(3):
        for _ in range(2):
            b3 = shapes(rng); b3[c] = 0.0
            cases.append(record(lib, rng.normal(size=(6, 10)), rng.normal(size=6), b3, 4))
    # betas reach zero exactly after the first iteration: A diagonal (row i of L holds the coefficient of betas[i]^2 only), every
    # operation of the first solve exact, x = -betas with rho[i] = -l[i] betas[i]^2; the second iteration then meets A = 0.
    # (candidates 1 and 2 have zero columns at once: eta == 0 at k = 2 and at k = 3)
    for l, b in (((1.0, 2.0, 0.5, 4.0), (2.0, -1.0, 4.0, 0.5)), ((-2.0, 1.0, 1.0, 0.25), (-1.0, 8.0, 2.0, -4.0))):
        L = np.zeros((6, 10)); rho = np.array([0, 0, 0, 0, 3.0, -1.0])
        for i, c in enumerate((0, 2, 5, 9)):
            L[i, c] = l[i]; rho[i] = -l[i] * b[i] * b[i]
        b3 = np.array([b, (b[0], b[1], 0, 0), (b[0], b[1], b[2], 0)], np.float64)
        cases.append(record(lib, L, rho, b3, 5))
    # the fourth column of A zero: columns 6..9 of L zero (every candidate); or columns 7..9 zero and betas[0] = 0 in candidate 0 only
    for i in range(2):
        L = rng.normal(size=(6, 10)); L[:, 6:] = 0.0
        cases.append(record(lib, L, rng.normal(size=6), shapes(rng), 6))
    for i in range(3):
        L = rng.normal(size=(6, 10)); L[:, 7:] = 0.0
        b3 = shapes(rng); b3[0, 0] = 0.0
        cases.append(record(lib, L, rng.normal(size=6), b3, 7))
    # the largest entry of the pivot columns in row 5, the row the `eta` scan never looks at
    for i in range(6):
        L = rng.normal(size=(6, 10)); L[5] *= 10.0 ** (7 + i)
        cases.append(record(lib, L, rng.normal(size=6), shapes(rng), 8))
    L = rng.normal(size=(6, 10)); L[2, 4] = np.inf
    cases.append(record(lib, L, rng.normal(size=6), shapes(rng), 9))
    L = rng.normal(size=(6, 10)); L[0, 0] = np.nan
    cases.append(record(lib, L, rng.normal(size=6), shapes(rng), 10))
    arr = np.array(cases, CASE)
    for key, v in coverage(arr).items():
        print("%-62s %d" % (key, v))
    np.save(PATH, arr)
    print("%d cases (%d bytes) -> %s" % (len(arr), os.path.getsize(PATH), PATH))


if __name__ == "__main__":
    main()
