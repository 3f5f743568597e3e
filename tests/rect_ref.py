"""The numpy twin of DESIGN.md section 8 "Rectification" (rectification): cv::initUndistortRectifyMap's maps in scalar-order float64 - the running
sums along a row are kept as a serial chain, vectorised over the rows only -, cv::remap's fixed-point conversion (INTER_BITS 5)
and its 8-bit bilinear interpolation with a constant 0 border.  tests/golden/rect_restatement_pins.json pins what it gives on the
cases below (tools/make_rect_pins.py), so that it cannot drift together with the kernels it is compared with."""
import hashlib
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OUTSIDE = np.iinfo(np.int32).min    # sx = sy of a pixel that is outside by its map value


class Cam:
    def __init__(self, K, D, R=None, P=None):
        self.K = tuple(float(v) for v in K)
        self.D = tuple(float(v) for v in D) + (0.0,) * (5 - len(D))
        self.R = np.eye(3) if R is None else np.asarray(R, np.float64).reshape(3, 3).copy()
        self.P = self.K if P is None else tuple(float(v) for v in P)


def inverse(cam):
    """iR = (Ar R)^-1, cv::invert's 3 x 3 case: the cofactors times d = 1 / det."""
    Ar = np.array([[cam.P[0], 0.0, cam.P[2]], [0.0, cam.P[1], cam.P[3]], [0.0, 0.0, 1.0]])
    M = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            s = np.float64(0.0)
            for k in range(3):
                s = s + Ar[i, k] * cam.R[k, j]
            M[i, j] = s
    c00 = M[1, 1] * M[2, 2] - M[1, 2] * M[2, 1]
    c01 = M[1, 0] * M[2, 2] - M[1, 2] * M[2, 0]
    c02 = M[1, 0] * M[2, 1] - M[1, 1] * M[2, 0]
    det = M[0, 0] * c00 - M[0, 1] * c01 + M[0, 2] * c02
    d = 1.0 / det
    b = np.empty(9)
    b[0] = c00 * d
    b[1] = (M[0, 2] * M[2, 1] - M[0, 1] * M[2, 2]) * d
    b[2] = (M[0, 1] * M[1, 2] - M[0, 2] * M[1, 1]) * d
    b[3] = (M[1, 2] * M[2, 0] - M[1, 0] * M[2, 2]) * d
    b[4] = (M[0, 0] * M[2, 2] - M[0, 2] * M[2, 0]) * d
    b[5] = (M[0, 2] * M[1, 0] - M[0, 0] * M[1, 2]) * d
    b[6] = c02 * d
    b[7] = (M[0, 1] * M[2, 0] - M[0, 0] * M[2, 1]) * d
    b[8] = (M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]) * d
    return b


def build_maps(cam, W, H):
    """(iR, mapx, mapy) for a W x H destination."""
    fx, fy, u0, v0 = cam.K
    k1, k2, p1, p2, k3 = cam.D
    ir = inverse(cam)
    i = np.arange(H, dtype=np.float64)
    _x = i * ir[1] + ir[2]
    _y = i * ir[4] + ir[5]
    _w = i * ir[7] + ir[8]
    mx = np.empty((H, W), np.float32)
    my = np.empty((H, W), np.float32)
    with np.errstate(all="ignore"):
        for j in range(W):
            w = 1.0 / _w
            x = _x * w
            y = _y * w
            x2 = x * x
            y2 = y * y
            r2 = x2 + y2
            _2xy = 2.0 * x * y
            kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
            u = fx * (x * kr + p1 * _2xy + p2 * (r2 + 2.0 * x2)) + u0
            v = fy * (y * kr + p1 * (r2 + 2.0 * y2) + p2 * _2xy) + v0
            mx[:, j] = u.astype(np.float32)
            my[:, j] = v.astype(np.float32)
            _x = _x + ir[0]
            _y = _y + ir[3]
            _w = _w + ir[6]
    return ir, mx, my


def fixed(mx, my):
    """sxsy (H x W x 2 int32): rint(map * 32.0f) in float32, ties to even; OUTSIDE for both where a map value is not finite or
    |map * 32| >= 2^20."""
    with np.errstate(all="ignore"):
        fx32 = mx.astype(np.float32) * np.float32(32.0)
        fy32 = my.astype(np.float32) * np.float32(32.0)
        ok = np.isfinite(fx32) & np.isfinite(fy32) & (np.abs(fx32) < np.float32(2 ** 20)) & (np.abs(fy32) < np.float32(2 ** 20))
    sx = np.where(ok, np.rint(np.where(ok, fx32, np.float32(0))).astype(np.int64), OUTSIDE)
    sy = np.where(ok, np.rint(np.where(ok, fy32, np.float32(0))).astype(np.int64), OUTSIDE)
    return np.stack([sx, sy], axis=-1).astype(np.int32)


def remap(src, sxsy):
    """src: H x W or H x W x CN uint8 -> (out in the destination's size, taps inside per pixel 0..4)."""
    h, w = src.shape[:2]
    s3 = src.reshape(h, w, -1).astype(np.int64)
    out_of = sxsy[..., 0] == OUTSIDE
    sx = np.where(out_of, 0, sxsy[..., 0]).astype(np.int64)
    sy = np.where(out_of, 0, sxsy[..., 1]).astype(np.int64)
    ix, iy, a, b = sx >> 5, sy >> 5, sx & 31, sy & 31

    def tap(yy, xx):
        inside = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h) & ~out_of
        p = s3[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
        return np.where(inside[..., None], p, 0), inside

    p00, i00 = tap(iy, ix)
    p01, i01 = tap(iy, ix + 1)
    p10, i10 = tap(iy + 1, ix)
    p11, i11 = tap(iy + 1, ix + 1)
    w00, w01, w10, w11 = (32 - a) * (32 - b) * 32, a * (32 - b) * 32, (32 - a) * b * 32, a * b * 32
    acc = w00[..., None] * p00 + w01[..., None] * p01 + w10[..., None] * p10 + w11[..., None] * p11
    out = ((acc + 16384) >> 15).astype(np.uint8)
    n = i00.astype(np.int32) + i01 + i10 + i11
    return out.reshape(sxsy.shape[:2] + src.shape[2:]), n


def rand_u8(seed, shape):
    """Deterministic bytes (splitmix64 of the element index): the same on every numpy."""
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(56)).astype(np.uint8).reshape(shape)


def rot(rx=0.0, ry=0.0, rz=0.0):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], np.float64)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], np.float64)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], np.float64)
    return np.round(Rz @ Ry @ Rx, 12)   # (twelve decimals: the same matrix whatever the last bit of the machine's cos and sin)


def euroc_cams():
    """(left, right, W, H) of tests/golden/rect_euroc_like.yaml, read by a parser of this file's own (the package's loader is
    tested against it)."""
    import re
    txt = open(os.path.join(GOLDEN, "rect_euroc_like.yaml")).read()
    m = {}
    for key, data in re.findall(r"^((?:LEFT|RIGHT)\.[KDRP]):.*?data:\s*\[(.*?)\]", txt, re.S | re.M):
        m[key] = np.array([float(v) for v in data.split(",")])
    cams = []
    for s in ("LEFT", "RIGHT"):
        K, P = m[s + ".K"], m[s + ".P"]
        cams.append(Cam((K[0], K[4], K[2], K[5]), m[s + ".D"], m[s + ".R"], (P[0], P[5], P[2], P[6])))
    return cams[0], cams[1], 752, 480


_SMALL = dict(K=(60.0, 58.0, 33.3, 17.2), D=(-0.35, 0.12, 0.002, -0.001, 0.01), P=(40.0, 40.0, 30.0, 16.5))


def cases():
    """name -> (left Cam, right Cam, src_w, src_h, dst_w, dst_h)."""
    small = Cam(R=rot(rz=0.05), **_SMALL)
    el, er, ew, eh = euroc_cams()
    ident = Cam((100.0, 100.0, 30.0, 20.0), (0, 0, 0, 0, 0))
    wide = Cam((120.0, 118.0, 64.5, 4.2), (-0.08, 0.01, 0.001, 0.0005, 0.0), rot(rz=-0.01), (236.0, 120.0, 128.0, 2.4))
    tiny = Cam((10.0, 10.5, 3.5, 3.6), (-0.1, 0.02, 0.001, -0.002, 0.0), rot(rz=0.1), (9.0, 9.0, 3.7, 3.4))
    # a quarter turn about y: _w = (j - 4) / 16 in exact steps, 0 at j = 4 (w = inf, the map value not finite), and beside it map
    # values beyond 2^15 pixels; the right camera looks almost along the image plane instead
    far = Cam((20.0, 20.0, 8.0, 4.0), (0.1, 0.01, 0.0, 0.0, 0.001), [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], (16.0, 16.0, 4.0, 4.0))
    far_r = Cam((20.0, 20.0, 8.0, 4.0), (0.1, 0.01, 0.0, 0.0, 0.001), rot(ry=1.0), (16.0, 16.0, 4.0, 4.0))
    return {
        "far": (far, far_r, 16, 8, 12, 8),
        "small": (small, small, 67, 35, 61, 33),
        "small_lr": (small, Cam(R=rot(rx=0.02, ry=-0.015, rz=-0.03), **_SMALL), 67, 35, 61, 33),
        "identity": (ident, ident, 67, 35, 67, 35),
        "wide": (wide, Cam((121.0, 119.0, 65.0, 4.0), (-0.07, 0.0, 0.0, 0.001, 0.002), rot(ry=0.01), (236.0, 120.0, 128.0, 2.4)), 130, 9, 257, 5),
        "tiny": (tiny, tiny, 8, 8, 8, 8),
        "euroc": (el, er, ew, eh, ew, eh),
    }


_memo = {}


def case_maps(name):
    """[(iR, mapx, mapy, sxsy) of the left camera, the same of the right one], computed once."""
    if name not in _memo:
        cl, cr, _, _, dw, dh = cases()[name]
        out = []
        for c in (cl, cr):
            ir, mx, my = build_maps(c, dw, dh)
            out.append((ir, mx, my, fixed(mx, my)))
            for a in out[-1]:
                a.setflags(write=False)
        _memo[name] = out
    return _memo[name]


def case_sources(name, cn, B=1, seed=11):
    """B raw pairs of the case: (L, R), each B x src_h x src_w (x 3)."""
    _, _, sw, sh, _, _ = cases()[name]
    shape = (B, sh, sw) if cn == 1 else (B, sh, sw, 3)
    return rand_u8(seed, shape), rand_u8(seed + 1, shape)


def sha(a):
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":   # (a NaN's sign and payload are the machine's choice: one pattern for all of them)
        u = a.view(np.uint32 if a.dtype == np.float32 else np.uint64).copy()
        u[np.isnan(a)] = 0x7FC00000 if a.dtype == np.float32 else 0x7FF8000000000000
        a = u
    return hashlib.sha256(a.tobytes()).hexdigest()


def same_floats(a, b):
    """Bit for bit, except that any NaN equals any NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


def pins():
    """What tests/golden/rect_restatement_pins.json holds: per case and side the SHA-256 of iR, the float maps, sxsy and the gray
    and BGR outputs of the case's first raw pair."""
    out = {}
    for name in cases():
        maps = case_maps(name)
        gray = case_sources(name, 1)
        bgr = case_sources(name, 3)
        for side, tag in enumerate(("left", "right")):
            ir, mx, my, s = maps[side]
            out["%s.%s" % (name, tag)] = dict(iR=sha(ir), mapx=sha(mx), mapy=sha(my), sxsy=sha(s),
                                              gray=sha(remap(gray[side][0], s)[0]), bgr=sha(remap(bgr[side][0], s)[0]))
    return out
