"""Numpy twin of the windowed bundle adjustment (DESIGN.md section 8 "Windowed bundle adjustment"; the device unit is
csrc/svo_ba.hip).  float64 throughout, every sum written out in its order: no BLAS call, no np.sum / np.dot / einsum, so the
results do not depend on the numpy build.  A sum over points is np.cumsum(...)[-1] (a strictly sequential accumulation), a sum
over a point's edges a Python loop over the frames of the window.

run(...) takes the records as the tracker leaves them (MAP_OBS_DTYPE, window x obs_stride), the per-frame counts and the float32
start poses, and returns the refined poses, the points, the statistics and a per-iteration trial log.  `order` changes the order
in which edges are summed - "canonical" (points by ascending gid, a point's edges by ascending frame), "reversed", or
("perm", seed) - and nothing else: numbering and outputs stay canonical.  The scatter between the three is the yardstick of the
device tests (tests/golden/ba_restatement_pins.json)."""
import math
import os
from fractions import Fraction

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

MAP_OBS_DTYPE = np.dtype([("gid", "<i4"), ("kp", "<i2"), ("flags", "<u2"), ("u", "<f4"), ("v", "<f4"), ("depth", "<f4"),
                          ("X", "<f4"), ("Y", "<f4"), ("Z", "<f4")])
HUBER_MONO = float(np.float32(math.sqrt(5.991)))     # (double)(float)sqrt(5.991)
HUBER_STEREO = float(np.float32(math.sqrt(7.815)))
STATUS_OK, STATUS_EMPTY = 0, 1
DBL_MAX = float(np.finfo(np.float64).max)


def default_params():
    return dict(window=8, n_fixed=1, iterations=10, stereo=1, huber_mono=HUBER_MONO, huber_stereo=HUBER_STEREO, lambda_init=0.0)


# ---- SE3 as g2o's SE3Quat, operation by operation as oracle/orc_pose.c states it (scalar Python floats) ----------------------
def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))   # exact product and sum, one rounding


def quat_from_R(m):
    q = [0.0] * 4
    t = m[0] + m[4] + m[8]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[7] - m[5]) * t
        q[1] = (m[2] - m[6]) * t
        q[2] = (m[3] - m[1]) * t
    else:
        i = 0
        if m[4] > m[0]:
            i = 1
        if m[8] > m[4 * i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[3 * k + j] - m[3 * j + k]) * t
        q[j] = (m[3 * j + i] + m[3 * i + j]) * t
        q[k] = (m[3 * k + i] + m[3 * i + k]) * t
    return q


def normalize_rotation(q):
    if q[3] < 0:
        q = [-v for v in q]
    n = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return [v / n for v in q]


def quat_mul(a, b):
    w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]
    x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1]
    y = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2]
    z = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0]
    return [x, y, z, w]


def quat_rot(q, v0, v1, v2):
    """q * v; v0, v1, v2 floats or arrays (the same expression element by element)."""
    uv0 = q[1] * v2 - q[2] * v1
    uv1 = q[2] * v0 - q[0] * v2
    uv2 = q[0] * v1 - q[1] * v0
    uv0 = uv0 + uv0
    uv1 = uv1 + uv1
    uv2 = uv2 + uv2
    return (v0 + q[3] * uv0 + (q[1] * uv2 - q[2] * uv1),
            v1 + q[3] * uv1 + (q[2] * uv0 - q[0] * uv2),
            v2 + q[3] * uv2 + (q[0] * uv1 - q[1] * uv0))


def quat_to_R(q):
    tx, ty, tz = 2 * q[0], 2 * q[1], 2 * q[2]
    twx, twy, twz = tx * q[3], ty * q[3], tz * q[3]
    txx, txy, txz = tx * q[0], ty * q[0], tz * q[0]
    tyy, tyz, tzz = ty * q[1], tz * q[1], tz * q[2]
    return [1 - (tyy + tzz), txy - twz, txz + twy,
            txy + twz, 1 - (txx + tzz), tyz - twx,
            txz - twy, tyz + twx, 1 - (txx + tyy)]


def se3_from_T(T):
    T = [float(v) for v in np.asarray(T, np.float64).ravel()]
    q = normalize_rotation(quat_from_R([T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]]))
    return (q, [T[3], T[7], T[11]])


def se3_to_T(s):
    R = quat_to_R(s[0])
    t = s[1]
    return np.array([R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2], 0.0, 0.0, 0.0, 1.0])


_SER_A = [-1.0 / 121645100408832000.0, 1.0 / 355687428096000.0, -1.0 / 1307674368000.0, 1.0 / 6227020800.0, -1.0 / 39916800.0,
          1.0 / 362880.0, -1.0 / 5040.0, 1.0 / 120.0, -1.0 / 6.0, 1.0]
_SER_B = [1.0 / 6402373705728000.0, -1.0 / 20922789888000.0, 1.0 / 87178291200.0, -1.0 / 479001600.0, 1.0 / 3628800.0,
          -1.0 / 40320.0, 1.0 / 720.0, -1.0 / 24.0, 0.5]
_SER_C = [1.0 / 121645100408832000.0, -1.0 / 355687428096000.0, 1.0 / 1307674368000.0, -1.0 / 6227020800.0, 1.0 / 39916800.0,
          -1.0 / 362880.0, 1.0 / 5040.0, -1.0 / 120.0, 1.0 / 6.0]


def exp_coeffs(t):
    """sin t / t, (1 - cos t) / t^2, (t - sin t) / t^3 for |t| < 0.5: the project's fixed series, a Horner chain of fma()."""
    x = t * t
    out = []
    for ser in (_SER_A, _SER_B, _SER_C):
        p = ser[0]
        for c in ser[1:]:
            p = _fma(p, x, c)
        out.append(p)
    return out


def se3_exp(u):
    om, up = u[:3], u[3:]
    theta = math.sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2])
    Om = [0.0, -om[2], om[1], om[2], 0.0, -om[0], -om[1], om[0], 0.0]
    Om2 = [Om[3 * r] * Om[c] + Om[3 * r + 1] * Om[3 + c] + Om[3 * r + 2] * Om[6 + c] for r in range(3) for c in range(3)]
    eye = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    if theta < 0.00001:
        R = [eye[i] + Om[i] + Om2[i] for i in range(9)]
        V = list(R)
    else:
        if theta < 0.5:
            a, b, c = exp_coeffs(theta)
        else:
            a = math.sin(theta) / theta
            b = (1 - math.cos(theta)) / (theta * theta)
            c = (theta - math.sin(theta)) / (theta * theta * theta)
        R = [eye[i] + a * Om[i] + b * Om2[i] for i in range(9)]
        V = [eye[i] + b * Om[i] + c * Om2[i] for i in range(9)]
    q = quat_from_R(R)
    t = [V[3 * r] * up[0] + V[3 * r + 1] * up[1] + V[3 * r + 2] * up[2] for r in range(3)]
    return (normalize_rotation(q), t)


def se3_oplus(u, est):
    """est <- exp(u) * est"""
    e = se3_exp([float(v) for v in u])
    rt = quat_rot(e[0], est[1][0], est[1][1], est[1][2])
    t = [e[1][0] + rt[0], e[1][1] + rt[1], e[1][2] + rt[2]]
    return (normalize_rotation(quat_mul(e[0], est[0])), t)


# ---- the edge list -------------------------------------------------------------------------------------------------------------
def associate(obs, counts, Tcw, window):
    """The edge-list rules.  Returns dict(gid (P,), n_obs (P,), X0 (P, 3) float64, mask (P, W) bool, rec (P, W) int: index into
    obs[f] of the edge's record, -1 where there is none)."""
    obs = np.asarray(obs)
    stride = obs.shape[1]
    est = [se3_from_T(np.asarray(Tcw[f], np.float32).astype(np.float64)) for f in range(window)]
    gid, frm, kp, idx = [], [], [], []
    for f in range(window):
        n = min(max(int(counts[f]), 0), stride)
        gid.append(obs["gid"][f, :n].astype(np.int64))
        kp.append(obs["kp"][f, :n].astype(np.int64))
        frm.append(np.full(n, f, np.int64))
        idx.append(np.arange(n, dtype=np.int64))
    gid, frm, kp, idx = (np.concatenate(a) for a in (gid, frm, kp, idx))
    order = np.lexsort((idx, kp, frm, gid))      # (gid, frame, kp); two records with one kp: the one stored first
    out_gid, out_X, out_mask, out_rec = [], [], [], []
    i, n = 0, len(order)
    while i < n:
        j = i
        g = gid[order[i]]
        slots = {}
        while j < n and gid[order[j]] == g:
            f = int(frm[order[j]])
            if f not in slots:
                slots[f] = int(idx[order[j]])
            j += 1
        i = j
        f0 = min(slots)
        r0 = obs[f0, slots[f0]]
        X = (float(r0["X"]), float(r0["Y"]), float(r0["Z"]))
        keep = {}
        for f, k in slots.items():
            z = quat_rot(est[f][0], X[0], X[1], X[2])[2] + est[f][1][2]
            if z > 0:           # z <= 0 (or not a number) at the start estimate: no edge
                keep[f] = k
        if len(keep) < 2:
            continue
        out_gid.append(int(g))
        out_X.append(X)
        m = np.zeros(window, bool)
        r = np.full(window, -1, np.int64)
        for f, k in keep.items():
            m[f] = True
            r[f] = k
        out_mask.append(m)
        out_rec.append(r)
    P = len(out_gid)
    return dict(gid=np.array(out_gid, np.int64), X0=np.array(out_X, np.float64).reshape(P, 3),
                mask=np.array(out_mask, bool).reshape(P, window), rec=np.array(out_rec, np.int64).reshape(P, window),
                n_obs=np.array([int(m.sum()) for m in out_mask], np.int64), est=est)


# ---- residuals and Jacobians ---------------------------------------------------------------------------------------------------
def project(est, X, cam, stereo_edge, exact_invz=False):
    """Camera coordinates and the projection of points X (P, 3) in the frame `est`.  stereo_edge (P,) bool: the stereo edge's
    cam_project (const float invz = 1.0f / z: a double division rounded to float, bf * invz a float product); otherwise the mono
    edge's (x / z fx + cx, y / z fy + cy) and a third component 0.  exact_invz: the stereo formulas with a double 1 / z (the
    differentiable variant the Jacobian test compares with)."""
    fx, fy, cx, cy, bf = cam
    x, y, z = quat_rot(est[0], X[:, 0], X[:, 1], X[:, 2])
    x = x + est[1][0]
    y = y + est[1][1]
    z = z + est[1][2]
    with np.errstate(all="ignore"):
        m0 = x / z * fx + cx
        m1 = y / z * fy + cy
        if exact_invz:
            invz = 1.0 / z
            bfi = bf * invz
        else:
            invz32 = (1.0 / z).astype(np.float32)
            invz = invz32.astype(np.float64)
            bfi = (np.float32(bf) * invz32).astype(np.float64)
        s0 = x * invz * fx + cx
        s1 = y * invz * fy + cy
        s2 = s0 - bfi
    p0 = np.where(stereo_edge, s0, m0)
    p1 = np.where(stereo_edge, s1, m1)
    p2 = np.where(stereo_edge, s2, 0.0)
    return (x, y, z), (p0, p1, p2)


def jacobians(est, pc, cam, stereo_edge):
    """Jl[i][a] (3 x 3: d error / d point, _jacobianOplusXi) and Jp[i][r] (3 x 6: d error / d pose, _jacobianOplusXj), each entry an
    array over the points; row 2 is 0 for a mono edge."""
    fx, fy, cx, cy, bf = cam
    x, y, z = pc
    R = quat_to_R(est[0])
    with np.errstate(all="ignore"):
        z_2 = z * z
        # mono: -1. / z * tmp * R, tmp = [fx 0 -x/z fx; 0 fy -y/z fy]  (the products with tmp's zeros left out)
        s = -1.0 / z
        a0, a2 = s * fx, s * (-x / z * fx)
        b1, b2 = s * fy, s * (-y / z * fy)
        Jl = [[None] * 3 for _ in range(3)]
        for j in range(3):
            mono0 = a0 * R[j] + a2 * R[6 + j]
            mono1 = b1 * R[3 + j] + b2 * R[6 + j]
            st0 = -fx * R[j] / z + fx * x * R[6 + j] / z_2
            st1 = -fy * R[3 + j] / z + fy * y * R[6 + j] / z_2
            st2 = st0 - bf * R[6 + j] / z_2
            Jl[0][j] = np.where(stereo_edge, st0, mono0)
            Jl[1][j] = np.where(stereo_edge, st1, mono1)
            Jl[2][j] = np.where(stereo_edge, st2, 0.0)
        zero = np.zeros_like(z)
        Jp = [[None] * 6 for _ in range(3)]
        Jp[0][0] = x * y / z_2 * fx
        Jp[0][1] = -(1 + (x * x / z_2)) * fx
        Jp[0][2] = y / z * fx
        Jp[0][3] = -1. / z * fx
        Jp[0][4] = zero
        Jp[0][5] = x / z_2 * fx
        Jp[1][0] = (1 + y * y / z_2) * fy
        Jp[1][1] = -x * y / z_2 * fy
        Jp[1][2] = -x / z * fy
        Jp[1][3] = zero
        Jp[1][4] = -1. / z * fy
        Jp[1][5] = y / z_2 * fy
        Jp[2][0] = np.where(stereo_edge, Jp[0][0] - bf * y / z_2, 0.0)
        Jp[2][1] = np.where(stereo_edge, Jp[0][1] + bf * x / z_2, 0.0)
        Jp[2][2] = np.where(stereo_edge, Jp[0][2], 0.0)
        Jp[2][3] = np.where(stereo_edge, Jp[0][3], 0.0)
        Jp[2][4] = zero
        Jp[2][5] = np.where(stereo_edge, Jp[0][5] - bf / z_2, 0.0)
    return Jl, Jp


def huber(chi, delta):
    """rho[0], rho[1] of RobustKernelHuber (delta an array over the edges; <= 0: no kernel)."""
    with np.errstate(all="ignore"):
        sq = np.sqrt(chi)
        lin = (delta > 0) & ~(chi <= delta * delta)
        rho0 = np.where(lin, 2 * sq * delta - delta * delta, chi)
        rho1 = np.where(lin, delta / sq, 1.0)
    return rho0, rho1


def _dot3(a0, b0, a1, b1, a2, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


class Problem:
    """One window's edges as arrays over (point, frame)."""

    def __init__(self, obs, counts, Tcw, cam, params):
        self.W = W = int(params["window"])
        self.nfix = int(params["n_fixed"])
        self.nfree = W - self.nfix
        self.cam = tuple(float(np.float32(v)) for v in cam)    # fx fy cx cy bf: the float32 camera, widened
        self.params = params
        a = associate(obs, counts, Tcw, W)
        self.assoc = a
        self.P = P = len(a["gid"])
        self.mask = a["mask"]
        self.est0 = a["est"]
        self.Tin = np.asarray(Tcw, np.float32).astype(np.float64).reshape(W, 16)
        u = np.zeros((P, W))
        v = np.zeros((P, W))
        d = np.zeros((P, W))
        obs = np.asarray(obs)
        for f in range(W):
            k = np.where(self.mask[:, f], a["rec"][:, f], 0)
            if obs.shape[1] == 0:
                continue
            u[:, f] = obs["u"][f, k].astype(np.float64)
            v[:, f] = obs["v"][f, k].astype(np.float64)
            d[:, f] = obs["depth"][f, k].astype(np.float64)
        self.stereo = self.mask & (d > 0) & bool(params["stereo"])
        with np.errstate(all="ignore"):
            self.obs = (u, v, np.where(self.stereo, u - self.cam[4] / np.where(self.stereo, d, 1.0), 0.0))
        self.delta = np.where(self.stereo, float(params["huber_stereo"]), float(params["huber_mono"]))
        self.has_edges = [bool(self.mask[:, f].any()) for f in range(W)]

    def errors(self, est, X, f, exact_invz=False):
        pc, p = project(est[f], X, self.cam, self.stereo[:, f], exact_invz)
        return pc, (self.obs[0][:, f] - p[0], self.obs[1][:, f] - p[1], self.obs[2][:, f] - p[2])

    def chi2(self, est, X, slot_order, point_order):
        """The robust chi2: per point the sum over its edges, then the sum over the points."""
        c = np.zeros(self.P)
        for f in slot_order:
            _, e = self.errors(est, X, f)
            with np.errstate(all="ignore"):
                r0, _ = huber(_dot3(e[0], e[0], e[1], e[1], e[2], e[2]), self.delta[:, f])
            c = c + np.where(self.mask[:, f], r0, 0.0)
        return float(np.cumsum(c[point_order])[-1])

    def build(self, est, X, slot_order, point_order):
        """Everything of buildSystem that does not depend on lambda."""
        P, W, nfix, nfree = self.P, self.W, self.nfix, self.nfree
        Hll = np.zeros((P, 3, 3))
        bl = np.zeros((P, 3))
        Wm = np.zeros((P, max(nfree, 1), 6, 3))
        Hpp = np.zeros((max(nfree, 1), 6, 6))
        bp = np.zeros((max(nfree, 1), 6))
        c = np.zeros(P)
        for f in slot_order:
            m = self.mask[:, f]
            pc, e = self.errors(est, X, f)
            Jl, Jp = jacobians(est[f], pc, self.cam, self.stereo[:, f])
            with np.errstate(all="ignore"):
                r0, w = huber(_dot3(e[0], e[0], e[1], e[1], e[2], e[2]), self.delta[:, f])
                c = c + np.where(m, r0, 0.0)
                for a in range(3):
                    for b in range(3):
                        Hll[:, a, b] = Hll[:, a, b] + np.where(m, w * _dot3(Jl[0][a], Jl[0][b], Jl[1][a], Jl[1][b], Jl[2][a], Jl[2][b]), 0.0)
                    bl[:, a] = bl[:, a] - np.where(m, w * _dot3(Jl[0][a], e[0], Jl[1][a], e[1], Jl[2][a], e[2]), 0.0)
                if f < nfix:
                    continue
                j = f - nfix
                for r in range(6):
                    for a in range(3):
                        Wm[:, j, r, a] = np.where(m, w * _dot3(Jp[0][r], Jl[0][a], Jp[1][r], Jl[1][a], Jp[2][r], Jl[2][a]), 0.0)
                    for cc in range(r, 6):
                        t = np.where(m, w * _dot3(Jp[0][r], Jp[0][cc], Jp[1][r], Jp[1][cc], Jp[2][r], Jp[2][cc]), 0.0)
                        Hpp[j, r, cc] = Hpp[j, cc, r] = np.cumsum(t[point_order])[-1]
                    t = np.where(m, w * _dot3(Jp[0][r], e[0], Jp[1][r], e[1], Jp[2][r], e[2]), 0.0)
                    bp[j, r] = np.cumsum(-t[point_order])[-1]
        chi = float(np.cumsum(c[point_order])[-1])
        return dict(Hll=Hll, bl=bl, W=Wm, Hpp=Hpp, bp=bp, chi=chi)

    def solve(self, S, lam, slot_order, point_order, full=False):
        """BlockSolver::solve with lambda on every diagonal.  Returns (ok, x (6 nfree,), dx (P, 3))."""
        P, nfree = self.P, self.nfree
        n = 6 * nfree
        H = S["Hll"]
        with np.errstate(all="ignore"):
            d00, d11, d22 = H[:, 0, 0] + lam, H[:, 1, 1] + lam, H[:, 2, 2] + lam
            d01, d02, d12 = H[:, 0, 1], H[:, 0, 2], H[:, 1, 2]
            c00 = d11 * d22 - d12 * d12
            c01 = d02 * d12 - d01 * d22
            c02 = d01 * d12 - d02 * d11
            det = (d00 * c00 + d01 * c01) + d02 * c02
            if not bool(np.all(np.isfinite(det) & (det > 0))):
                return False, None, None
            inv = 1.0 / det
            Di = np.empty((P, 3, 3))
            Di[:, 0, 0] = c00 * inv
            Di[:, 0, 1] = Di[:, 1, 0] = c01 * inv
            Di[:, 0, 2] = Di[:, 2, 0] = c02 * inv
            Di[:, 1, 1] = (d00 * d22 - d02 * d02) * inv
            Di[:, 1, 2] = Di[:, 2, 1] = (d01 * d02 - d00 * d12) * inv
            Di[:, 2, 2] = (d00 * d11 - d01 * d01) * inv
            Wm = S["W"]
            Y = np.empty_like(Wm)
            for k in range(3):
                Y[..., k] = (Wm[..., 0] * Di[:, None, None, 0, k] + Wm[..., 1] * Di[:, None, None, 1, k]) + Wm[..., 2] * Di[:, None, None, 2, k]
            Hs = np.zeros((n, n))
            bs = np.zeros(n)
            bl = S["bl"]
            for fi in range(nfree):
                for fj in range(fi, nfree):
                    t = (Y[:, fi, :, None, 0] * Wm[:, fj, None, :, 0] + Y[:, fi, :, None, 1] * Wm[:, fj, None, :, 1]) + Y[:, fi, :, None, 2] * Wm[:, fj, None, :, 2]
                    s = np.cumsum(t[point_order], axis=0)[-1] if P else np.zeros((6, 6))
                    for r in range(6):
                        for c in range(6):
                            a, b = 6 * fi + r, 6 * fj + c
                            if a > b:
                                continue
                            h = (S["Hpp"][fi, r, c] if fi == fj else 0.0)
                            if a == b:
                                h = h + lam
                            Hs[a, b] = Hs[b, a] = h - s[r, c]
                t = (Y[:, fi, :, 0] * bl[:, None, 0] + Y[:, fi, :, 1] * bl[:, None, 1]) + Y[:, fi, :, 2] * bl[:, None, 2]
                s = np.cumsum(t[point_order], axis=0)[-1]
                for r in range(6):
                    bs[6 * fi + r] = S["bp"][fi, r] - s[r]
        x = _ldlt_solve(Hs.tolist(), bs.tolist())
        if x is None:
            return False, None, None
        x = np.array(x)
        with np.errstate(all="ignore"):
            t = bl.copy()
            for f in slot_order:
                j = f - self.nfix
                if j < 0:
                    continue
                xj = x[6 * j:6 * j + 6]
                for k in range(3):
                    acc = Wm[:, j, 0, k] * xj[0]
                    for r in range(1, 6):
                        acc = acc + Wm[:, j, r, k] * xj[r]
                    t[:, k] = t[:, k] - acc
            dx = np.empty((P, 3))
            for k in range(3):
                dx[:, k] = (Di[:, k, 0] * t[:, 0] + Di[:, k, 1] * t[:, 1]) + Di[:, k, 2] * t[:, 2]
        if full:
            return True, x, dx, Hs, bs
        return True, x, dx


def _ldlt_solve(H, b):
    """LDL^T without pivoting, as oracle/orc_pose.c's ldlt6_solve for n unknowns; None when a pivot is not positive."""
    n = len(b)
    L = [[0.0] * n for _ in range(n)]
    D = [0.0] * n
    for j in range(n):
        d = H[j][j]
        Lj = L[j]
        for k in range(j):
            d -= Lj[k] * Lj[k] * D[k]
        if not d > 0.0:
            return None
        D[j] = d
        Lj[j] = 1.0
        for i in range(j + 1, n):
            s = H[i][j]
            Li = L[i]
            for k in range(j):
                s -= Li[k] * Lj[k] * D[k]
            Li[j] = s / d
    y = [0.0] * n
    for i in range(n):
        s = b[i]
        for k in range(i):
            s -= L[i][k] * y[k]
        y[i] = s
    for i in range(n):
        y[i] /= D[i]
    x = [0.0] * n
    for i in range(n - 1, -1, -1):
        s = y[i]
        for k in range(i + 1, n):
            s -= L[k][i] * x[k]
        x[i] = s
    return x


def _orders(P, W, order):
    if order == "canonical":
        return list(range(W)), np.arange(P)
    if order == "reversed":
        return list(range(W - 1, -1, -1)), np.arange(P)[::-1]
    kind, seed = order
    assert kind == "perm"
    rng = np.random.RandomState(seed)
    return [int(v) for v in rng.permutation(W)], rng.permutation(P)


def run(obs, counts, Tcw, cam, params, order="canonical"):
    """-> dict(Tcw (W, 16) float64, gid, n_obs, X (P, 3), stats dict, log: per iteration a list of trials
    (lambda, chi2 of the trial, rho, accepted, solved))."""
    pr = Problem(obs, counts, Tcw, cam, params)
    W, P, nfix, nfree = pr.W, pr.P, pr.nfix, pr.nfree
    stats = dict(status=STATUS_EMPTY, n_points=0, n_edges=0, n_edges_stereo=0, iterations=0, trials_total=0,
                 chi2_initial=0.0, chi2_final=0.0, lambda_final=0.0)
    if P == 0:
        return dict(Tcw=pr.Tin.copy(), gid=pr.assoc["gid"], n_obs=pr.assoc["n_obs"], X=pr.assoc["X0"], stats=stats, log=[], trials=[])
    slot_order, point_order = _orders(P, W, order)
    est = list(pr.est0)
    X = pr.assoc["X0"].copy()
    lam, ni, nbad = -1.0, 2.0, 0
    log, iters, trials_total = [], 0, 0
    chi_init = cur = 0.0
    for it in range(int(params["iterations"])):
        S = pr.build(est, X, slot_order, point_order)
        cur = S["chi"]
        ini = cur
        if it == 0:
            chi_init = cur
            if params["lambda_init"] > 0:
                lam = float(params["lambda_init"])
            else:
                md = 0.0
                for j in range(nfree):
                    for r in range(6):
                        md = max(abs(float(S["Hpp"][j, r, r])), md)
                md = max(md, float(np.max(np.abs(S["Hll"][:, [0, 1, 2], [0, 1, 2]]))))
                lam = 1e-5 * md
        trials, rho, qmax = [], 0.0, 0
        while True:
            ok, x, dx = pr.solve(S, lam, slot_order, point_order)
            if ok:
                est_t = [se3_oplus(x[6 * (f - nfix):6 * (f - nfix) + 6], est[f]) if f >= nfix and pr.has_edges[f] else est[f] for f in range(W)]
                X_t = X + dx
                tmp = pr.chi2(est_t, X_t, slot_order, point_order)
                with np.errstate(all="ignore"):
                    sp = 0.0
                    for a in range(6 * nfree):
                        sp = sp + float(x[a]) * (lam * float(x[a]) + float(S["bp"].ravel()[a]))
                    s = (dx[:, 0] * (lam * dx[:, 0] + S["bl"][:, 0]) + dx[:, 1] * (lam * dx[:, 1] + S["bl"][:, 1])) + dx[:, 2] * (lam * dx[:, 2] + S["bl"][:, 2])
                    scale = (sp + float(np.cumsum(s[point_order])[-1])) + 1e-3
            else:           # a failed solve: no update (x = 0), the trial's chi2 is DBL_MAX
                est_t, X_t, tmp, scale = est, X, DBL_MAX, 1e-3
            with np.errstate(all="ignore"):
                rho = float((np.float64(cur) - np.float64(tmp)) / np.float64(scale))
            lam_used = lam
            accepted = bool(rho > 0 and math.isfinite(tmp))
            if accepted:
                v = 2 * rho - 1
                alpha = min(1. - v * v * v, 2. / 3.)
                lam *= max(1. / 3., alpha)
                ni = 2.0
                cur = tmp
                est, X = est_t, X_t
            else:
                lam *= ni
                ni *= 2
            trials.append((lam_used, tmp, rho, accepted, bool(ok)))
            qmax += 1
            trials_total += 1
            if not (rho < 0 and qmax < 10):
                break
        log.append(trials)
        iters += 1
        if qmax == 10 or rho == 0:
            break
        nbad = nbad + 1 if (ini - cur) * 1e3 < ini else 0
        if nbad >= 3:
            break
    T = pr.Tin.copy()
    for f in range(nfix, W):
        if pr.has_edges[f]:
            T[f] = se3_to_T(est[f])
    stats.update(status=STATUS_OK, n_points=P, n_edges=int(pr.mask.sum()), n_edges_stereo=int(pr.stereo.sum()), iterations=iters,
                 trials_total=trials_total, chi2_initial=chi_init, chi2_final=cur, lambda_final=lam)
    return dict(Tcw=T, gid=pr.assoc["gid"], n_obs=pr.assoc["n_obs"], X=X, stats=stats, log=log,
                trials=[len(t) for t in log])


def discrete(res):
    s = res["stats"]
    return dict(status=s["status"], n_points=s["n_points"], n_edges=s["n_edges"], n_edges_stereo=s["n_edges_stereo"],
                iterations=s["iterations"], trials=[int(v) for v in res["trials"]])


ORDERS = ("canonical", "reversed", ("perm", 7))
