"""Numpy restatement of the colour part of the Lucas-Kanade contract (DESIGN.md section 8 "LK", "colour"): OpenCV 3.2's
calcOpticalFlowPyrLK with its default arguments on 8UC3 images, cn = 3.  Written from the contract, not from the kernels: the
pyramid and the derivatives per channel with tests/lk_ref.py's own pyr_down and scharr, the window as one vector of
21 x 21 x 3 = 1323 samples (pixel-major, channel-minor, as the interleaved bytes lie), every float32 operation spelled out.

What differs from the gray restatement: the sums run over 1323 samples, the minimum-eigenvalue divisor stays 2 * 21 * 21 = 882,
the error divisor is 32 * 21 * 3 * 21 = 42336.

track() returns what lk_ref.track() returns - images (h, w, 3) uint8, derivatives (h, w, 6) int16 with entry 2 c = dx and
2 c + 1 = dy of channel c - and `sums`: per point the exact integers (sum ix^2, sum ix iy, sum iy^2) of the first level the
point runs (the highest level whose range test passes), with that level in `sums_level` (-1: none ran).
"""
import numpy as np

from lk_ref import (EXIT_EPSILON, EXIT_MAX_COUNT, EXIT_MIN_EIG, EXIT_NOT_RUN, EXIT_OSCILLATION, EXIT_RANGE_NEXT,
                    EXIT_RANGE_PREV, F, MAX_COUNT, NPIX, WIN, _out_of_range, _to_f32, _weights, level_sizes, pyr_down, reflect101,
                    scharr)

CN = 3
NSAMP = NPIX * CN                  # 1323
_WY, _WX = np.divmod(np.arange(NPIX), WIN)


def build_pyramid(img, max_level=3):
    """([level images (h, w, 3) uint8], [derivatives (h, w, 6) int16]): every channel on its own."""
    img = np.ascontiguousarray(img, np.uint8)
    assert img.ndim == 3 and img.shape[2] == CN
    n = len(level_sizes(img.shape[1], img.shape[0], max_level))
    levels = [img]
    for _ in range(1, n):
        levels.append(np.stack([pyr_down(levels[-1][:, :, c]) for c in range(CN)], axis=2))
    derivs = [np.concatenate([scharr(l[:, :, c]) for c in range(CN)], axis=2) for l in levels]
    return levels, derivs


def _sample_image(img, ix, iy, iw):
    """(1323,) sums of the four taps: sample (pixel, c) takes channel c of the pixel, of its right and of its lower neighbours."""
    h, w = img.shape[:2]
    x0, x1 = reflect101(ix + _WX, w), reflect101(ix + _WX + 1, w)
    y0, y1 = reflect101(iy + _WY, h), reflect101(iy + _WY + 1, h)
    p = img.astype(np.int64)
    return (p[y0, x0] * iw[0] + p[y0, x1] * iw[1] + p[y1, x0] * iw[2] + p[y1, x1] * iw[3]).reshape(-1)


def _sample_deriv(der, ix, iy, iw):
    """(1323, 2) sums of the four taps of (dx, dy), samples outside the level are 0."""
    h, w = der.shape[:2]
    out = np.zeros((NPIX, 2 * CN), np.int64)
    for (dy, dx), wgt in zip(((0, 0), (0, 1), (1, 0), (1, 1)), iw):
        x, y = ix + _WX + dx, iy + _WY + dy
        ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        v = der[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)].astype(np.int64)
        out += np.where(ok[:, None], v, 0) * wgt
    return out.reshape(NSAMP, 2)


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
        if float(min_eig) < 1e-4 or D < np.finfo(np.float32).eps:
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
                err = _to_f32(np.abs(diff).sum()) / F(32 * NSAMP)       # 42336 = 32 * 21 * 3 * 21
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
