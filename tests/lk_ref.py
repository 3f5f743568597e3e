"""Numpy restatement of the sparse pyramidal Lucas-Kanade contract of DESIGN.md section 8 ("LK"): OpenCV 3.2's
calcOpticalFlowPyrLK with its default arguments (21 x 21 window, maxLevel 3, COUNT+EPS 30 / 0.01, flags 0, minEigThreshold
1e-4) on 8-bit images of one channel, (H, W), or of three, (H, W, 3) - the "colour" part of the contract.  Written from the
contract, not from the kernels: one point at a time, the pyramid and the derivatives per channel, the window as one vector
of 21 x 21 x cn samples (pixel-major, channel-minor, as the interleaved bytes lie), every float32 operation spelled out as one
numpy float32 operation.  The channel count is in the sums (441 cn samples) and in the error divisor 32 * 441 * cn; the
minimum-eigenvalue divisor stays 2 * 441 = 882.

track() returns the next points, status and err, every level's image (h, w) or (h, w, 3) and derivative planes (h, w, 2 cn)
int16 with entry 2 c = dx and 2 c + 1 = dy of channel c - of both frames, for every point and level the way the level ended
(EXIT_*), so that a test can show which path a point took, and `sums`: per point the exact integers (sum ix^2, sum ix iy,
sum iy^2) of the first level the point runs (the highest level whose range test passes), with that level in `sums_level`
(-1: none ran).
"""
import numpy as np

F = np.float32
WIN = 21
NPIX = WIN * WIN
MAX_COUNT = 30
W_ONE = 16384                      # bilinear weights in 14 bits

(EXIT_NOT_RUN, EXIT_RANGE_PREV, EXIT_MIN_EIG, EXIT_RANGE_NEXT, EXIT_EPSILON, EXIT_OSCILLATION, EXIT_MAX_COUNT) = range(7)


def reflect101(i, n):
    """BORDER_REFLECT_101 of index array i into [0, n) (one fold: |i| and n + 20 at most, n >= 22)."""
    i = np.abs(np.asarray(i, np.int64))
    return np.where(i >= n, 2 * (n - 1) - i, i)


def pyr_down(img):
    """[1 4 6 4 1] x [1 4 6 4 1], reflect-101, ((w + 1) / 2, (h + 1) / 2), (sum + 128) >> 8; every channel on its own."""
    h, w = img.shape[:2]
    oh, ow = (h + 1) // 2, (w + 1) // 2
    k = (1, 4, 6, 4, 1)
    src = img.astype(np.int64)
    xs = reflect101(2 * np.arange(ow)[:, None] + np.arange(-2, 3)[None, :], w)
    ys = reflect101(2 * np.arange(oh)[:, None] + np.arange(-2, 3)[None, :], h)
    rows = sum(k[j] * src[:, xs[:, j]] for j in range(5))
    out = sum(k[i] * rows[ys[:, i], :] for i in range(5))
    return ((out + 128) >> 8).astype(np.uint8)


def scharr(img):
    """(h, w, 2 cn) int16: dx = [3 10 3]^T x [-1 0 1], dy = [-1 0 1]^T x [3 10 3] of every channel, neighbours reflect-101 inside
    the image."""
    h, w = img.shape[:2]
    s = img.astype(np.int64)
    xm, xp = reflect101(np.arange(w) - 1, w), reflect101(np.arange(w) + 1, w)
    ym, yp = reflect101(np.arange(h) - 1, h), reflect101(np.arange(h) + 1, h)
    dh = s[:, xp] - s[:, xm]
    dx = 3 * dh[ym, :] + 10 * dh + 3 * dh[yp, :]
    dv = s[yp, :] - s[ym, :]
    dy = 3 * dv[:, xm] + 10 * dv + 3 * dv[:, xp]
    return np.stack([dx, dy], axis=-1).reshape(h, w, -1).astype(np.int16)


def level_sizes(w, h, max_level=3):
    """[(w, h)] of the levels in use: a level of width <= 21 or height <= 21 is not built, the one before it is the top."""
    sizes = [(w, h)]
    while len(sizes) <= max_level:
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= WIN or h <= WIN:
            break
        sizes.append((w, h))
    return sizes


def build_pyramid(img, max_level=3):
    """([level images], [their derivatives]) of an (H, W) or (H, W, 3) image."""
    img = np.ascontiguousarray(img, np.uint8)
    assert img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 3)
    n = len(level_sizes(img.shape[1], img.shape[0], max_level))
    levels = [img]
    for _ in range(1, n):
        levels.append(pyr_down(levels[-1]))
    return levels, [scharr(l) for l in levels]


def _round_half_even(v):
    return int(np.rint(v))


def _weights(a, b):
    one, s = F(1), F(W_ONE)
    iw00 = _round_half_even(((one - a) * (one - b)) * s)
    iw01 = _round_half_even((a * (one - b)) * s)
    iw10 = _round_half_even(((one - a) * b) * s)
    return iw00, iw01, iw10, W_ONE - iw00 - iw01 - iw10


_WY, _WX = np.divmod(np.arange(NPIX), WIN)


def _sample_image(img, ix, iy, iw):
    """(441 cn,) sums of the four taps: sample (pixel, c) takes channel c of the pixel, of its right and of its lower neighbours,
    image read reflect-101 outside the level."""
    h, w = img.shape[:2]
    x0, x1 = reflect101(ix + _WX, w), reflect101(ix + _WX + 1, w)
    y0, y1 = reflect101(iy + _WY, h), reflect101(iy + _WY + 1, h)
    p = img.astype(np.int64)
    return (p[y0, x0] * iw[0] + p[y0, x1] * iw[1] + p[y1, x0] * iw[2] + p[y1, x1] * iw[3]).reshape(-1)


def _sample_deriv(der, ix, iy, iw):
    """(441 cn, 2) sums of the four taps of (dx, dy), samples outside the level are 0."""
    h, w = der.shape[:2]
    out = np.zeros((NPIX, der.shape[2]), np.int64)
    for (dy, dx), wgt in zip(((0, 0), (0, 1), (1, 0), (1, 1)), iw):
        x, y = ix + _WX + dx, iy + _WY + dy
        ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        v = der[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)].astype(np.int64)
        out += np.where(ok[:, None], v, 0) * wgt
    return out.reshape(-1, 2)


def _out_of_range(ix, iy, w, h):
    return ix < -WIN or ix >= w or iy < -WIN or iy >= h


def _to_f32(total):
    """An exact integer sum (below 2^53) to float32, rounded to nearest once."""
    return F(int(total))


def track_point(levels_prev, derivs_prev, levels_next, pt):
    """One point through the levels.  Returns (x, y, status, err, exits[4], iterations[4], sums (3 ints) or None, their level)."""
    top = len(levels_prev) - 1
    scale20 = F(1.0 / (1 << 20))
    half = F(10)
    exits = [EXIT_NOT_RUN] * 4
    iters = [0] * 4
    status, err = 1, F(0)
    sums, sums_level = None, -1
    ptx, pty = F(pt[0]), F(pt[1])
    ox = oy = F(0)
    for level in range(top, -1, -1):
        I, J, der = levels_prev[level], levels_next[level], derivs_prev[level]
        h, w = I.shape[:2]
        cn = 1 if I.ndim == 2 else I.shape[2]
        sc = F(1.0 / (1 << level))
        px, py = ptx * sc, pty * sc
        if level == top:
            ox, oy = px, py
        else:
            ox, oy = ox * F(2), oy * F(2)
        px, py = px - half, py - half
        ipx, ipy = int(np.floor(px)), int(np.floor(py))
        if _out_of_range(ipx, ipy, w, h):
            exits[level] = EXIT_RANGE_PREV
            if level == 0:
                status = 0
            continue
        iw = _weights(px - F(ipx), py - F(ipy))
        Ip = (_sample_image(I, ipx, ipy, iw) + (1 << 8)) >> 9
        d = (_sample_deriv(der, ipx, ipy, iw) + (1 << 13)) >> 14
        gx, gy = d[:, 0], d[:, 1]
        s11, s12, s22 = int((gx * gx).sum()), int((gx * gy).sum()), int((gy * gy).sum())
        if sums is None:
            sums, sums_level = (s11, s12, s22), level
        A11 = _to_f32(s11) * scale20
        A12 = _to_f32(s12) * scale20
        A22 = _to_f32(s22) * scale20
        D = A11 * A22 - A12 * A12
        t = A11 - A22
        root = np.sqrt(t * t + (F(4) * A12) * A12)
        min_eig = ((A22 + A11) - root) / F(2 * NPIX)                     # 882: the channel count is not in it
        if float(min_eig) < 1e-4 or D < np.finfo(np.float32).eps:    # the threshold is a double, FLT_EPSILON a float
            exits[level] = EXIT_MIN_EIG
            if level == 0:
                status = 0
            continue
        D = F(1) / D
        nx, ny = ox - half, oy - half
        pdx = pdy = F(0)
        exits[level] = EXIT_MAX_COUNT
        for j in range(MAX_COUNT):
            inx, iny = int(np.floor(nx)), int(np.floor(ny))
            if _out_of_range(inx, iny, w, h):
                exits[level] = EXIT_RANGE_NEXT
                if level == 0:
                    status = 0
                break
            iters[level] = j + 1
            jw = _weights(nx - F(inx), ny - F(iny))
            diff = ((_sample_image(J, inx, iny, jw) + (1 << 8)) >> 9) - Ip
            b1 = _to_f32((diff * gx).sum()) * scale20
            b2 = _to_f32((diff * gy).sum()) * scale20
            dx = (A12 * b2 - A22 * b1) * D
            dy = (A12 * b1 - A11 * b2) * D
            nx, ny = nx + dx, ny + dy
            ox, oy = nx + half, ny + half
            if float(dx) * float(dx) + float(dy) * float(dy) <= 1e-4:
                exits[level] = EXIT_EPSILON
                break
            if j > 0 and float(abs(dx + pdx)) < 0.01 and float(abs(dy + pdy)) < 0.01:
                ox, oy = ox - dx * F(0.5), oy - dy * F(0.5)
                exits[level] = EXIT_OSCILLATION
                break
            pdx, pdy = dx, dy
        if level == 0 and status:
            fx, fy = ox - half, oy - half
            ifx, ify = int(np.floor(fx)), int(np.floor(fy))
            if _out_of_range(ifx, ify, w, h):
                status = 0
            else:
                fw = _weights(fx - F(ifx), fy - F(ify))
                diff = ((_sample_image(J, ifx, ify, fw) + (1 << 8)) >> 9) - Ip
                err = _to_f32(np.abs(diff).sum()) / F(32 * NPIX * cn)      # 14112 gray, 42336 = 32 * 21 * 3 * 21 colour
    return ox, oy, status, err, exits, iters, sums, sums_level


def track(prev, nxt, pts, max_level=3):
    lp, dp = build_pyramid(prev, max_level)
    ln, dn = build_pyramid(nxt, max_level)
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    n = len(pts)
    out = dict(next_pts=np.zeros((n, 2), np.float32), status=np.zeros(n, np.uint8), err=np.zeros(n, np.float32),
               exits=np.zeros((n, 4), np.int32), iterations=np.zeros((n, 4), np.int32), top=len(lp) - 1,
               levels_prev=lp, derivs_prev=dp, levels_next=ln, derivs_next=dn,
               sums=np.zeros((n, 3), np.int64), sums_level=np.full(n, -1, np.int32))
    with np.errstate(all="ignore"):
        for i in range(n):
            x, y, st, e, ex, it, sums, sl = track_point(lp, dp, ln, pts[i])
            out["next_pts"][i] = (x, y)
            out["status"][i] = st
            out["err"][i] = e
            out["exits"][i] = ex
            out["iterations"][i] = it
            if sums is not None:
                out["sums"][i] = sums
                out["sums_level"][i] = sl
    return out
