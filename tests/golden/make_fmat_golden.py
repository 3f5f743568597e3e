#!/usr/bin/env python3
"""Generate tests/golden/fmat_cases.npz: the normalised 8-point fundamental matrix in 50-digit arithmetic (mpmath).

The 8-point estimate (cv::findFundamentalMat(..., CV_FM_8POINT), reference src/pnpmatch.cc:336) is restated twice in this
project, in float64: oracle/orc_fmat.c (cyclic Jacobi) and csrc/svo_fmat_dev.h (one wavefront).  Neither can referee the
other, so this file states the same algorithm - isotropic normalisation, 9 x 9 normal matrix, eigenvector of its smallest
eigenvalue (mpmath.eigsy), rank-2 projection, de-normalisation - with 50 digits, where its own rounding is nil.

Per case `c` the file holds
  c/p1, c/p2      the inputs (current / last frame's points, float64)
  c/F             the reference F rounded to float64: Frobenius norm 1, sign fixed by its largest entry (zeros: F = 0)
  c/f8            F[8] of the de-normalised UNIT eigenvector solution - what the |F[8]| > 1.19e-7 switch of both restatements sees
  c/lam           the two smallest and the largest eigenvalue of the normal matrix
  c/last, c/cur   probe point pairs (float32) at which the gate's point-to-line distance is compared
  c/dev, c/bound  (entry deviation, probe deviation) of the CPU oracle from the reference as tests/gate_ref.py measures
                  them, and the bounds the device gets: max(16 x that, 64 eps lam9 / (lam2 - lam1))
`names` lists the cases.  Run from the repository root:  python tests/golden/make_fmat_golden.py
(the oracle is built on the way; mpmath is needed here only - the tests read the .npz)."""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import gate_ref  # noqa: E402

mp.mp.dps = 50
EPS = 2.0 ** -52
K = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1.0]])
NS = [8, 9, 63, 64, 65, 127, 128, 129, 448, 511, 512]
GAP_MIN = 1e-8          # relative eigen-gap below which the eigenvector is not compared entry by entry


def rot_y(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def project(X):
    p = (K @ X.T).T
    return p[:, :2] / p[:, 2:]


def scene(rng, n, kind):
    if kind == "planar":            # points on the plane z = 20 + 0.3 x
        x = rng.uniform(-10, 10, n); y = rng.uniform(-2, 2, n)
        return np.stack([x, y, 20 + 0.3 * x], 1)
    return np.stack([rng.uniform(-10, 10, n), rng.uniform(-2, 2, n), rng.uniform(6, 50, n)], 1)


def two_view(seed, n, noise, R, t, kind="general"):
    """p1 = "current" view, p2 = "last" view of the same points (p2^T F p1 = 0)."""
    rng = np.random.default_rng(seed)
    X = scene(rng, n, kind)
    p1 = project(X)
    p2 = project((R @ X.T).T + t)
    if noise > 0:
        p1 = p1 + rng.normal(0, noise, p1.shape); p2 = p2 + rng.normal(0, noise, p2.shape)
    return p1, p2


# ---- the algorithm in 50 digits ---------------------------------------------------------------------------------------
def fmat_mp(p1, p2):
    """(F 3x3 mp matrix of the unit-eigenvector solution, or None where the point set is degenerate; [lam1, lam2, lam9])"""
    n = len(p1)
    P1 = [(mp.mpf(float(a)), mp.mpf(float(b))) for a, b in p1]
    P2 = [(mp.mpf(float(a)), mp.mpf(float(b))) for a, b in p2]
    if n < 8:
        return None, None

    def normalise(P):
        cx = mp.fsum(p[0] for p in P) / n; cy = mp.fsum(p[1] for p in P) / n
        d = mp.fsum(mp.sqrt((p[0] - cx) ** 2 + (p[1] - cy) ** 2) for p in P) / n
        if d == 0:
            return None, None
        s = mp.sqrt(2) / d
        return [((p[0] - cx) * s, (p[1] - cy) * s) for p in P], mp.matrix([[s, 0, -s * cx], [0, s, -s * cy], [0, 0, 1]])
    Q1, T1 = normalise(P1)
    Q2, T2 = normalise(P2)
    if Q1 is None or Q2 is None:
        return None, None
    A = mp.zeros(9, 9)
    for (a1, b1), (a2, b2) in zip(Q1, Q2):
        r = [a2 * a1, a2 * b1, a2, b2 * a1, b2 * b1, b2, a1, b1, mp.mpf(1)]
        for a in range(9):
            for b in range(a, 9):
                A[a, b] += r[a] * r[b]
    for a in range(9):
        for b in range(a):
            A[a, b] = A[b, a]
    w, V = mp.eigsy(A)                    # ascending eigenvalues
    order = sorted(range(9), key=lambda k: w[k])
    f = [V[k, order[0]] for k in range(9)]
    F0 = mp.matrix(3, 3)
    for k in range(9):
        F0[k // 3, k % 3] = f[k]
    # rank 2: F0 (I - v3 v3^T), v3 the eigenvector of the smallest eigenvalue of F0^T F0
    gw, GV = mp.eigsy(F0.T * F0)
    g = min(range(3), key=lambda k: gw[k])
    v3 = mp.matrix([GV[0, g], GV[1, g], GV[2, g]])
    F1 = F0 - (F0 * v3) * v3.T
    return T2.T * F1 * T1, [w[order[0]], w[order[1]], w[order[8]]]


def to_np(Fm):
    return np.array([[float(Fm[r, c]) for c in range(3)] for r in range(3)])


# ---- the case list -----------------------------------------------------------------------------------------------------
def gap_of(p1, p2):
    Fm, lam = fmat_mp(p1, p2)
    return float((lam[1] - lam[0]) / lam[2]), to_np(Fm)


def draw(seed, n, noise, R, t, min_gap, f8_rel_min=0.0):
    """two_view with the first seed (seed, seed + 7919, ...) whose reference eigen-gap is at least min_gap - ten times the
    1e-8 below which entries are not compared, a hundred times for the un-normalised branch, whose F[8] must stay far below
    the 1.19e-7 switch on the device as well - and, for the noisy translations, whose |F[8]| / ||F|| is above f8_rel_min."""
    while True:
        p1, p2 = two_view(seed, n, noise, R, t)
        gap, F = gap_of(p1, p2)
        if gap >= min_gap and abs(F[2, 2]) / np.linalg.norm(F) >= f8_rel_min:
            return p1, p2
        seed += 7919


def case_list():
    """(name, p1, p2, tag): tag 'norm' = the F[8] = 1 branch, 'raw' = |F[8]| tiny (un-normalised branch), 'zero' = F = 0,
    'ungapped' = the eigenvector is not unique (residual and rank only)."""
    Rg, tg = rot_y(0.03), np.array([0.1, -0.05, -1.0])
    I = np.eye(3)
    out = []
    for n in NS:
        for noise in (0.0, 0.3):
            out.append(("general_n%d_s%g" % (n, noise), *draw(1000 + n, n, noise, Rg, tg, 1e-7), "norm"))
    trans = {"forward": np.array([0.0, 0.0, -1.0]), "sideways": np.array([0.8, 0.0, 0.0]), "anytrans": np.array([0.3, -0.1, -0.9])}
    for name, t in trans.items():
        for n in (8, 64, 129):
            out.append(("%s_n%d_s0" % (name, n), *draw(2000 + n, n, 0.0, I, t, 1e-6), "raw"))
        for n in (9, 65, 511):
            # noisy: the normalised branch, and not near the switch
            out.append(("%s_n%d_s0.3" % (name, n), *draw(3000 + n, n, 0.3, I, t, 1e-7, 1e-3), "norm"))
    for off in (1e4, 1e6):
        for n in (9, 128):
            p1, p2 = draw(4000 + n, n, 0.3, Rg, tg, 1e-7)
            out.append(("offset%g_n%d" % (off, n), p1 + off, p2 + off, "norm"))
    for n in (8, 127):                      # every point inside a 2 x 2 px patch
        rng = np.random.default_rng(5000 + n)
        p1 = 300.0 + rng.uniform(0, 2, (n, 2))
        p2 = p1 + np.array([0.5, 0.25]) + 0.02 * (p1 - 301.0) ** 2 + rng.normal(0, 0.01, (n, 2))
        out.append(("patch_n%d" % n, p1, p2, "norm"))
    # all points scaled so that every diagonal entry of the normal matrix is nearly equal: the padding eigenvalue (the
    # largest diagonal entry) then ties with real diagonal entries.  Points on the unit square's corners, four of each, give
    # normalised coordinates of +-1 in both images: every product in a constraint row is +-1, every diagonal entry n.
    rng = np.random.default_rng(6000)
    corners = np.array([[0, 0], [0, 2], [2, 0], [2, 2]], np.float64)
    i1 = np.repeat(np.arange(4), 4); i2 = np.tile(np.arange(4), 4)
    p1 = 100.0 + corners[i1] + rng.normal(0, 1e-3, (16, 2)); p2 = 100.0 + corners[i2] + rng.normal(0, 1e-3, (16, 2))
    out.append(("equal_diagonal_n16", p1, p2, "norm"))
    # degenerate inputs: F = 0.  Coordinates are dyadic, so that n x sums and divides exactly in any order and the centroid
    # IS the point (with other coordinates the rounding residue of the centroid decides: see docs/NEXT_ROUNDS.md)
    rng = np.random.default_rng(7000)
    spread = np.round(rng.uniform(0, 1000, (20, 2)) * 8) / 8
    same = np.tile(np.array([[321.5, 100.25]]), (20, 1))
    out.append(("pts2_identical_n20", spread, same, "zero"))
    out.append(("pts1_identical_n20", same, spread, "zero"))
    out.append(("one_pair_x8", np.tile(np.array([[640.5, 180.25]]), (8, 1)), np.tile(np.array([[600.75, 181.0]]), (8, 1)), "zero"))
    # not unique: a planar scene (every F = [e]x H of the plane's homography family fits) and a collinear set
    for n in (9, 64, 129):
        out.append(("planar_n%d" % n, *two_view(8000 + n, n, 0.0, Rg, tg, "planar"), "ungapped"))
    for n in (8, 65, 448):
        rng = np.random.default_rng(9000 + n)
        u = rng.uniform(0, 1200, n)
        p1 = np.stack([u, 50 + 0.2 * u], 1)
        # the points correspond by no projective map of the two lines l1, l2, so the null space is exactly the family
        # l2 a^T + b l1^T: five-dimensional, and rank 2 throughout (the rank-2 step then leaves the residual alone)
        v = u + 5 + 30 * np.sin(u / 100)
        p2 = np.stack([v, 48 + 0.21 * v], 1)
        out.append(("collinear_n%d" % n, p1, p2, "ungapped"))
    return out


def probes(seed, p1):
    """32 probe pairs: last-frame and current-frame points spread over the inputs' own range, as float32."""
    rng = np.random.default_rng(seed)
    lo, hi = p1.min(0), p1.max(0)
    span = np.maximum(hi - lo, 1.0)
    last = (lo + rng.uniform(0, 1, (32, 2)) * span).astype(np.float32)
    cur = (lo + rng.uniform(0, 1, (32, 2)) * span).astype(np.float32)
    return last, cur


def write_npz(path, arrays):
    """np.savez stamps every member with the current time; this writes the same container (np.load reads it) with a fixed
    stamp, so that a second run reproduces the committed file byte for byte."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    from oracle import binding as orc
    orc.build()
    g = {}
    names, tags = [], []
    for k, (name, p1, p2, tag) in enumerate(case_list()):
        p1 = np.ascontiguousarray(p1, np.float64); p2 = np.ascontiguousarray(p2, np.float64)
        Fm, lam = fmat_mp(p1, p2)
        last, cur = probes(100 + k, p1)
        g[name + "/p1"], g[name + "/p2"], g[name + "/last"], g[name + "/cur"] = p1, p2, last, cur
        Fo = orc.fundamental_8point(p1, p2)
        if Fm is None:
            assert tag == "zero", name
            g[name + "/F"] = np.zeros((3, 3)); g[name + "/f8"] = np.zeros(1); g[name + "/lam"] = np.zeros(3)
            g[name + "/dev"] = np.zeros(2); g[name + "/bound"] = np.zeros(2)
            print("%-24s n=%3d  F = 0   (oracle F = 0: %s)" % (name, len(p1), not Fo.any()))
            names.append(name); tags.append(tag)
            continue
        F = to_np(Fm)
        Fn = gate_ref.normalise_F(F)
        lam = np.array([float(v) for v in lam])
        gap = (lam[1] - lam[0]) / lam[2]
        gapped = gap >= GAP_MIN
        assert gapped == (tag != "ungapped"), (name, gap)
        spread = float(np.linalg.norm(p1 - p1.mean(0), axis=1).mean())
        dev = np.array([gate_ref.entry_deviation(Fo, Fn), gate_ref.probe_deviation(Fo, Fn, last, cur, spread)]) if gapped \
            else np.zeros(2)
        floor = 64 * EPS / gap if gapped else 0.0
        bound = np.maximum(16 * dev, floor) if gapped else np.zeros(2)
        g[name + "/F"], g[name + "/f8"], g[name + "/lam"] = Fn, np.array([F[2, 2]]), lam
        g[name + "/dev"], g[name + "/bound"] = dev, bound
        print("%-24s n=%3d %-8s f8 %+.3e gap %.3e oracle dev entry %.2e probe %.2e bound entry %.2e probe %.2e"
              % (name, len(p1), tag, F[2, 2], gap, dev[0], dev[1], bound[0], bound[1]))
        names.append(name); tags.append(tag)
    g["names"] = np.array(names)
    g["tags"] = np.array(tags)
    path = os.path.join(HERE, "fmat_cases.npz")
    write_npz(path, g)
    print("wrote", path, os.path.getsize(path), "bytes,", len(names), "cases")


if __name__ == "__main__":
    main()
