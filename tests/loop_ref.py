"""The numpy twin of loop verification (svo_loop_* in include/svo.h): SearchByBoW over two FeatureVectors and the fixed-scale
Sim3Solver, operation by operation as DESIGN.md section 8 "Loop verification" states them.  Every rule the contract fixes is a
switch in RULES, so that tests/test_loop_cpu.py can show for each one a case that tells it from its neighbour.

A *scene* is a dict of arrays in the device layout: desc (F, S, 32) uint8, kp (F, S) KP, n (F,), fv (F, S) FEATURE, fv_n (F,),
obs (F, So) MAP_OBS, obs_n (F,), Tcw (F, 16) float32.  Floating point: Python floats and numpy float64 / float32 scalars only,
one rounding per operation, sums in the stated order."""
import math

import numpy as np

KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
               ("class_id", "<i4")])
FEATURE = np.dtype([("node", "<u4"), ("feature", "<u4")])
MAP_OBS = np.dtype([("gid", "<i4"), ("kp", "<i2"), ("flags", "<u2"), ("u", "<f4"), ("v", "<f4"), ("depth", "<f4"),
                    ("X", "<f4"), ("Y", "<f4"), ("Z", "<f4")])
CAND = np.dtype([("frame", "<i4"), ("reserved", "<i4"), ("score", "<f8")])
RESULT = np.dtype([("status", "<i4"), ("n_matches", "<i4"), ("bound", "<i4"), ("visited", "<i4"), ("winner", "<i4"),
                   ("n_inliers", "<i4"), ("sample", "<i4", (3,)), ("reserved", "<i4"), ("T12", "<f8", (16,))])
OK, FEW, REJECTED, SKIPPED = 0, 1, 2, 3
MASK = (1 << 64) - 1
SWEEPS = 12

PARAMS = dict(th_low=50, nn_ratio=0.75, check_orientation=1, prob=0.99, min_inliers=20, max_iterations=300,
              seed=0x5eed5eed5eed5eed, chi2=9.210, scale_factor=1.2, refine=0)

# the contract's rules; each mutant of tests/test_loop_cpu.py flips one
RULES = dict(best_le=False,          # `<=` on the best distance (a tie takes the later i2)
             tie_second=True,        # a tie with the best becomes the second best
             th_le=False,            # best1 <= th_low
             ratio_f64=False,        # the ratio product in float64
             use_matched2=True,      # an i2 taken by an earlier i1 is skipped
             nomp_in_best2=False,    # an i2 without a map point still counts into best2
             round_even=False,       # round half to even
             wrap30=True,            # bin 30 -> 0
             maxima_later=False,     # ties among the maxima go to the later bin
             tenth_le=False,         # `<=` in the 0.1 rule
             best_gt=False,          # `>` instead of `>=` for the best hypothesis
             stop_ge=False,          # `>=` instead of `>` for the stop
             replace=False,          # draws with replacement
             use_keypoint=False,     # p1, p2 from the keypoints instead of the projected map points
             one_sided=False,        # only the error in a's image is tested
             wrong_octave=False)     # maxerr1 from b's octave and maxerr2 from a's


def params(**kw):
    p = dict(PARAMS)
    for k, v in kw.items():
        if k not in p:
            raise TypeError(k)
        p[k] = v
    return p


def rules(**kw):
    r = dict(RULES)
    for k, v in kw.items():
        if k not in r:
            raise TypeError(k)
        r[k] = v
    return r


_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(d, D):
    """d (32,) against D (m, 32) -> (m,) int"""
    return _POP[np.bitwise_xor(D, d[None, :])].sum(axis=1)


def clamp(v, hi):
    return min(max(int(v), 0), int(hi))


def has_map_point(scene, f):
    S = scene["desc"].shape[1]
    n = clamp(scene["n"][f], S)
    has = np.zeros(S, bool)
    for o in scene["obs"][f][:clamp(scene["obs_n"][f], scene["obs"].shape[1])]:
        if 0 <= o["kp"] < n:
            has[o["kp"]] = True
    return has


def node_runs(fv):
    runs, order = {}, []
    for e in fv:
        nd = int(e["node"])
        if nd not in runs:
            runs[nd] = []
            order.append(nd)
        runs[nd].append(int(e["feature"]))
    return runs, order


def c_round(x, even=False):
    x = float(x)
    if even:
        return int(np.rint(x))
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


def rot_bin(a1, a2, R=RULES):
    rot = np.float32(a1) - np.float32(a2)
    if rot < 0:
        rot = np.float32(rot + np.float32(360.0))
    x = np.float32(rot * np.float32(np.float32(1.0) / np.float32(30)))
    if not (-1000.0 < x < 1000.0):
        return -1
    b = c_round(x, R["round_even"])
    if b == 30 and R["wrap30"]:
        b = 0
    return b if 0 <= b < 30 else -1


def three_maxima(hist, R=RULES):
    max1 = max2 = max3 = 0
    i1 = i2 = i3 = -1
    gt = (lambda s, m: s >= m and s > 0) if R["maxima_later"] else (lambda s, m: s > m)
    for i in range(30):
        s = int(hist[i])
        if gt(s, max1):
            max3, max2, max1 = max2, max1, s
            i3, i2, i1 = i2, i1, i
        elif gt(s, max2):
            max3, max2 = max2, s
            i3, i2 = i2, i
        elif gt(s, max3):
            max3, i3 = s, i
    lt = (lambda a, b: a <= b) if R["tenth_le"] else (lambda a, b: a < b)
    if lt(np.float32(max2), np.float32(0.1) * np.float32(max1)):
        i2 = i3 = -1
    elif lt(np.float32(max3), np.float32(0.1) * np.float32(max1)):
        i3 = -1
    return i1, i2, i3


def _scan(dist, cand, counted, P, R):
    """the contract's scan over one node's i2 (dist, cand, counted per position) -> accepted position or -1, best1, best2"""
    best1 = best2 = 256
    idx = -1
    for pos in range(len(dist)):
        if not counted[pos]:
            continue
        d = int(dist[pos])
        if not cand[pos]:              # (only with nomp_in_best2: it may become the second best, never the match)
            best2 = min(best2, d)
            continue
        if d < best1 or (R["best_le"] and d == best1):
            best2, best1, idx = best1, d, pos
        elif d < best2 and (R["tie_second"] or d != best1):
            best2 = d
    ok1 = best1 <= P["th_low"] if R["th_le"] else best1 < P["th_low"]
    if R["ratio_f64"]:
        ok2 = float(best1) < float(np.float32(P["nn_ratio"])) * float(best2)
    else:
        ok2 = np.float32(best1) < np.float32(np.float32(P["nn_ratio"]) * np.float32(best2))
    return (idx if ok1 and ok2 and idx >= 0 else -1), best1, best2


def _scan_fast(dist, cand, P):
    """_scan under the default rules, vectorised (tests/test_loop_cpu.py holds the two against each other)"""
    pos = np.flatnonzero(cand)
    if pos.size == 0:
        return -1, 256, 256
    keys = dist[pos].astype(np.int64) * 4096 + pos
    k = int(np.argmin(keys))
    best = int(keys[k])
    keys[k] = 1 << 40
    second = int(keys.min())
    best1, idx = best >> 12, best & 4095
    best2 = 256 if second >= (1 << 40) else second >> 12
    ok = best1 < P["th_low"] and np.float32(best1) < np.float32(np.float32(P["nn_ratio"]) * np.float32(best2))
    return (idx if ok else -1), best1, best2


def match_pair(scene, a, b, P=PARAMS, R=RULES, fast=None):
    """SearchByBoW(KF1 = a, KF2 = b) -> (match (S,) int32, n_matches, info)"""
    S = scene["desc"].shape[1]
    match = np.full(S, -1, np.int32)
    info = dict(nodes=[], log=[], hist=np.zeros(30, np.int64), keep=(-1, -1, -1), before=None)
    if a < 0 or b < 0:
        return match, 0, info
    nA, nB = clamp(scene["n"][a], S), clamp(scene["n"][b], S)
    hasA, hasB = has_map_point(scene, a), has_map_point(scene, b)
    runsA, orderA = node_runs(scene["fv"][a][:clamp(scene["fv_n"][a], S)])
    runsB, _ = node_runs(scene["fv"][b][:clamp(scene["fv_n"][b], S)])
    default = R == RULES
    for node in orderA:
        if node not in runsB:
            continue
        f1s, f2s = runsA[node], np.array(runsB[node], np.int64)
        info["nodes"].append((node, len(f1s), len(f2s)))
        inb = f2s < nB
        mp2 = inb & hasB[np.minimum(f2s, S - 1)]
        matched = np.zeros(len(f2s), bool)
        use_fast = default and (fast if fast is not None else len(f2s) > 128)
        D2 = scene["desc"][b][np.minimum(f2s, S - 1)]
        for i1 in f1s:
            if i1 >= nA or not hasA[i1]:
                continue
            dist = hamming(scene["desc"][a][i1], D2)
            free = ~matched if R["use_matched2"] else np.ones(len(f2s), bool)
            cand = mp2 & free
            if use_fast:
                pos, b1, b2 = _scan_fast(dist, cand, P)
            else:
                counted = (inb & free) if R["nomp_in_best2"] else cand
                pos, b1, b2 = _scan(dist, cand, counted, P, R)
            info["log"].append((int(i1), b1, b2, int(f2s[pos]) if pos >= 0 else -1))
            if pos >= 0:
                match[i1] = f2s[pos]
                matched[pos] = True
    info["before"] = match.copy()
    if P["check_orientation"]:
        bins = np.full(S, -1, np.int64)
        for i1 in np.flatnonzero(match >= 0):
            bins[i1] = rot_bin(scene["kp"][a][i1]["angle"], scene["kp"][b][match[i1]]["angle"], R)
            if bins[i1] >= 0:
                info["hist"][bins[i1]] += 1
        keep = three_maxima(info["hist"], R)
        info["keep"] = keep
        for i1 in np.flatnonzero(match >= 0):
            if bins[i1] < 0 or bins[i1] not in keep:
                match[i1] = -1
    return match, int((match >= 0).sum()), info


# ---- the solver -----------------------------------------------------------------------------------------------------------------
def sigma2_table(scale_factor):
    sc = np.float32(1.0)
    out = []
    for l in range(8):
        if l > 0:
            sc = np.float32(sc * np.float32(scale_factor))
        out.append(float(np.float32(sc * sc)))
    return out


def bounds(P, n_max):
    out = np.zeros(n_max + 1, np.int32)
    for N in range(n_max + 1):
        b = 0
        if N == P["min_inliers"]:
            b = 1
        elif N > P["min_inliers"]:
            eps = float(P["min_inliers"]) / float(N)
            den = math.log(1.0 - math.pow(eps, 3.0))
            num = math.log(1.0 - P["prob"])
            v = math.ceil(num / den) if den != 0.0 else -math.inf
            if not (v < P["max_iterations"]) or v < 0:
                b = P["max_iterations"]
            else:
                b = 1 if v < 1 else int(v)
        out[N] = b
    return out


def splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def sample(seed, it, N, replace=False):
    avail = list(range(N))
    out = []
    for d in range(3):
        size = N if replace else N - d
        x = splitmix64((seed + 3 * it + d) & MASK)
        r = (x * size) >> 64
        out.append(avail[r])
        if not replace:
            avail[r] = avail[size - 1]
    return out


def quat_rot(M):
    """M 3 x 3 (lists) -> R12 3 x 3 (lists): Horn's N, the cyclic Jacobi, the quaternion's rotation"""
    a = [[0.0] * 4 for _ in range(4)]
    a[0][0] = M[0][0] + M[1][1] + M[2][2]
    a[0][1] = M[1][2] - M[2][1]
    a[0][2] = M[2][0] - M[0][2]
    a[0][3] = M[0][1] - M[1][0]
    a[1][1] = M[0][0] - M[1][1] - M[2][2]
    a[1][2] = M[0][1] + M[1][0]
    a[1][3] = M[2][0] + M[0][2]
    a[2][2] = -M[0][0] + M[1][1] - M[2][2]
    a[2][3] = M[1][2] + M[2][1]
    a[3][3] = -M[0][0] - M[1][1] + M[2][2]
    for i in range(4):
        for j in range(i):
            a[i][j] = a[j][i]
    v = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    sweeps = 0
    for _ in range(SWEEPS):
        rotated = False
        for p in range(3):
            for q in range(p + 1, 4):
                apq = a[p][q]
                if apq == 0.0:
                    continue
                app, aqq = a[p][p], a[q][q]
                g = 100.0 * abs(apq)
                if abs(app) + g == abs(app) and abs(aqq) + g == abs(aqq):
                    a[p][q] = a[q][p] = 0.0
                    continue
                rotated = True
                theta = (aqq - app) / (2.0 * apq)
                den = abs(theta) + math.sqrt(theta * theta + 1.0)
                t = -1.0 / den if theta < 0.0 else 1.0 / den
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(4):
                    if k != p and k != q:
                        akp, akq = a[k][p], a[k][q]
                        a[k][p] = a[p][k] = c * akp - s * akq
                        a[k][q] = a[q][k] = s * akp + c * akq
                a[p][p] = app - t * apq
                a[q][q] = aqq + t * apq
                a[p][q] = a[q][p] = 0.0
                for k in range(4):
                    vkp, vkq = v[k][p], v[k][q]
                    v[k][p] = c * vkp - s * vkq
                    v[k][q] = s * vkp + c * vkq
        sweeps += 1
        if not rotated:
            break
    best, col = a[0][0], 0
    for j in range(1, 4):
        if a[j][j] > best:
            best, col = a[j][j], j
    w, x, y, z = v[0][col], v[1][col], v[2][col], v[3][col]
    nrm = math.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / nrm, x / nrm, y / nrm, z / nrm
    R = [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
         [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
         [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]]
    return R, dict(sweeps=sweeps, eig=[a[i][i] for i in range(4)], col=col, quat=(w, x, y, z))


def _sum3(a, b, c, order):
    if order == 0:
        return (a + b) + c
    if order == 1:
        return (c + b) + a
    return a + (b + c)


def _seq(vals, order):
    if order == 1:
        vals = vals[::-1]
    if order == 2 and len(vals) > 1:
        h = len(vals) // 2
        return _seq(vals[:h], 0) + _seq(vals[h:], 0)
    s = 0.0
    for x in vals:
        s += x
    return s


def horn(P1, P2, three, order=0):
    """P1, P2: lists of [x, y, z] (camera a / camera b) -> (R12, t12).  three: the sample's form ((a + b) + c, / 3.0); else the
    refit's (a running sum from 0.0, / n)."""
    n = len(P1)
    if three:
        O1 = [_sum3(P1[0][c], P1[1][c], P1[2][c], order) / 3.0 for c in range(3)]
        O2 = [_sum3(P2[0][c], P2[1][c], P2[2][c], order) / 3.0 for c in range(3)]
    else:
        O1 = [_seq([p[c] for p in P1], order) / float(n) for c in range(3)]
        O2 = [_seq([p[c] for p in P2], order) / float(n) for c in range(3)]
    r1 = [[p[c] - O1[c] for c in range(3)] for p in P1]
    r2 = [[p[c] - O2[c] for c in range(3)] for p in P2]
    if three:
        M = [[_sum3(r2[0][i] * r1[0][j], r2[1][i] * r1[1][j], r2[2][i] * r1[2][j], order) for j in range(3)] for i in range(3)]
    else:
        M = [[_seq([r2[k][i] * r1[k][j] for k in range(n)], order) for j in range(3)] for i in range(3)]
    R, info = quat_rot(M)
    t = [O1[i] - ((R[i][0] * O2[0] + R[i][1] * O2[1]) + R[i][2] * O2[2]) for i in range(3)]
    return R, t, info


def correspondences(scene, a, b, match, cam, P, R=RULES):
    """the accepted matches by ascending i1 whose keypoints both have a record -> dict of float64 arrays"""
    S, So = scene["desc"].shape[1], scene["obs"].shape[1]
    ix = []
    for f in (a, b):
        t = np.full(S, -1, np.int64)
        for i, o in enumerate(scene["obs"][f][:clamp(scene["obs_n"][f], So)]):
            if 0 <= o["kp"] < S:
                t[o["kp"]] = i
        ix.append(t)
    i1s = [i for i in range(S) if 0 <= match[i] < S and ix[0][i] >= 0 and ix[1][match[i]] >= 0]
    N = len(i1s)
    i1s = np.array(i1s, np.int64)
    i2s = match[i1s].astype(np.int64) if N else np.zeros(0, np.int64)
    fx, fy, cx, cy = (float(np.float32(cam[k])) for k in ("fx", "fy", "cx", "cy"))
    sig = sigma2_table(P["scale_factor"])
    out = dict(N=N, i1=i1s, i2=i2s)
    X = []
    for f, ks, t in ((a, i1s, ix[0]), (b, i2s, ix[1])):
        T = scene["Tcw"][f].astype(np.float64).reshape(4, 4)
        o = scene["obs"][f][t[ks]]
        Xw = [o[c].astype(np.float64) for c in ("X", "Y", "Z")]
        X.append([((T[r, 0] * Xw[0] + T[r, 1] * Xw[1]) + T[r, 2] * Xw[2]) + T[r, 3] for r in range(3)])
    out["X1"], out["X2"] = X
    with np.errstate(all="ignore"):
        out["p1"] = [fx * X[0][0] / X[0][2] + cx, fy * X[0][1] / X[0][2] + cy]
        out["p2"] = [fx * X[1][0] / X[1][2] + cx, fy * X[1][1] / X[1][2] + cy]
    kA, kB = scene["kp"][a][i1s], scene["kp"][b][i2s]
    if R["use_keypoint"]:
        out["p1"] = [kA["x"].astype(np.float64), kA["y"].astype(np.float64)]
        out["p2"] = [kB["x"].astype(np.float64), kB["y"].astype(np.float64)]
    oa = np.clip(kA["octave"], 0, 7)
    ob = np.clip(kB["octave"], 0, 7)
    if R["wrong_octave"]:
        oa, ob = ob, oa
    out["maxerr1"] = np.array([P["chi2"] * sig[l] for l in oa], np.float64)
    out["maxerr2"] = np.array([P["chi2"] * sig[l] for l in ob], np.float64)
    out["cam"] = (fx, fy, cx, cy)
    return out


def errors(Cn, R, t):
    """(e1, e2) of every correspondence under (R12, t12)"""
    fx, fy, cx, cy = Cn["cam"]
    x1, y1, z1 = Cn["X1"]
    x2, y2, z2 = Cn["X2"]
    t21 = [-((R[0][i] * t[0] + R[1][i] * t[1]) + R[2][i] * t[2]) for i in range(3)]
    with np.errstate(all="ignore"):
        X = ((R[0][0] * x2 + R[0][1] * y2) + R[0][2] * z2) + t[0]
        Y = ((R[1][0] * x2 + R[1][1] * y2) + R[1][2] * z2) + t[1]
        Z = ((R[2][0] * x2 + R[2][1] * y2) + R[2][2] * z2) + t[2]
        du1 = Cn["p1"][0] - (fx * X / Z + cx)
        dv1 = Cn["p1"][1] - (fy * Y / Z + cy)
        e1 = du1 * du1 + dv1 * dv1
        U = ((R[0][0] * x1 + R[1][0] * y1) + R[2][0] * z1) + t21[0]
        V = ((R[0][1] * x1 + R[1][1] * y1) + R[2][1] * z1) + t21[1]
        W = ((R[0][2] * x1 + R[1][2] * y1) + R[2][2] * z1) + t21[2]
        du2 = (fx * U / W + cx) - Cn["p2"][0]
        dv2 = (fy * V / W + cy) - Cn["p2"][1]
        e2 = du2 * du2 + dv2 * dv2
    return e1, e2


def inlier_flags(Cn, R, t, Ru=RULES):
    e1, e2 = errors(Cn, R, t)
    with np.errstate(all="ignore"):
        f = e1 < Cn["maxerr1"]
        if not Ru["one_sided"]:
            f = f & (e2 < Cn["maxerr2"])
    return f


def hypothesis(Cn, idx, order=0):
    P1 = [[float(Cn["X1"][c][j]) for c in range(3)] for j in idx]
    P2 = [[float(Cn["X2"][c][j]) for c in range(3)] for j in idx]
    return horn(P1, P2, True, order)


def solve_pair(scene, a, b, match, cam, P=PARAMS, R=RULES, order=0, all_counts=False):
    """Sim3Solver with the scale fixed -> (result RESULT scalar, inliers (S,) uint8, info)"""
    S = scene["desc"].shape[1]
    res = np.zeros(1, RESULT)[0]
    res["winner"] = -1
    res["sample"] = -1
    res["T12"] = np.eye(4).ravel()
    inl = np.zeros(S, np.uint8)
    info = dict(counts=[], corr=None)
    if a < 0 or b < 0:
        res["status"] = SKIPPED
        return res, inl, info
    Cn = correspondences(scene, a, b, match, cam, P, R)
    info["corr"] = Cn
    N = Cn["N"]
    res["n_matches"] = N
    if N < P["min_inliers"]:
        res["status"] = FEW
        return res, inl, info
    bound = int(bounds(P, N)[N])
    best, winner, status, visited = 0, -1, REJECTED, 0
    for i in range(bound):
        idx = sample(P["seed"], i, N, R["replace"])
        Rm, t, _ = hypothesis(Cn, idx, order)
        c = int(inlier_flags(Cn, Rm, t, R).sum())
        info["counts"].append(c)
        if status == OK:
            continue
        visited = i + 1
        if (c > best) if R["best_gt"] else (c >= best):
            best, winner = c, i
            if (c >= P["min_inliers"]) if R["stop_ge"] else (c > P["min_inliers"]):
                status = OK
                if not all_counts:
                    break
    if winner < 0:      # (only with best_gt: nothing ever beat 0)
        winner = 0
    idx = sample(P["seed"], winner, N, R["replace"])
    Rm, t, _ = hypothesis(Cn, idx, order)
    flags = inlier_flags(Cn, Rm, t, R)
    n_inl = int(flags.sum())
    info["e_winner"] = errors(Cn, Rm, t)
    if P["refine"] and n_inl > 0:
        js = np.flatnonzero(flags)
        P1 = [[float(Cn["X1"][c][j]) for c in range(3)] for j in js]
        P2 = [[float(Cn["X2"][c][j]) for c in range(3)] for j in js]
        Rm, t, _ = horn(P1, P2, False, order)
        flags = inlier_flags(Cn, Rm, t, R)
        n_inl = int(flags.sum())
    inl[Cn["i1"][flags]] = 1
    res["status"], res["bound"], res["visited"], res["winner"], res["n_inliers"] = status, bound, visited, winner, n_inl
    res["sample"] = idx
    T = np.eye(4)
    T[:3, :3] = np.array(Rm)
    T[:3, 3] = np.array(t)
    res["T12"] = T.ravel()
    info["flags"] = flags
    return res, inl, info


def pairs_of(cand, cand_n, q0, top_k):
    Q = cand.shape[0]
    out = np.full((Q * top_k, 2), -1, np.int32)
    for i in range(Q):
        for t in range(clamp(cand_n[i], top_k)):
            if cand[i, t]["frame"] >= 0:
                out[i * top_k + t] = (q0 + i, cand[i, t]["frame"])
    return out


def verify(scene, pairs, cam, P=PARAMS, R=RULES):
    """every pair through both stages -> (match (n, S), match_n (n,), result (n,) RESULT, inliers (n, S))"""
    n, S = len(pairs), scene["desc"].shape[1]
    match = np.zeros((n, S), np.int32)
    mn = np.zeros(n, np.int32)
    res = np.zeros(n, RESULT)
    inl = np.zeros((n, S), np.uint8)
    for p, (a, b) in enumerate(pairs):
        match[p], mn[p], _ = match_pair(scene, int(a), int(b), P, R)
        res[p], inl[p], _ = solve_pair(scene, int(a), int(b), match[p], cam, P, R)
    return match, mn, res, inl
