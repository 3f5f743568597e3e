"""CPU suite of the rectification stage: the numpy restatement of DESIGN.md section 8 "Rectification" (tests/rect_ref.py) against its pins, its
properties, an independent check of its map builder, the settings loader, and the library's host-side argument checks."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import rect_ref as rr


def test_restatement_matches_its_pins():
    want = json.load(open(os.path.join(rr.GOLDEN, "rect_restatement_pins.json")))
    got = rr.pins()
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key


def test_case_conditions():
    """What the GPU tests rely on: the strong small case has pixels with 0, 1, 2 and 4 taps inside, the identity none with 0;
    the far case has map values that are not finite and finite ones beyond the fixed-point range."""
    L, _ = rr.case_sources("small", 1)
    n = rr.remap(L[0], rr.case_maps("small")[0][3])[1]
    hist = np.bincount(n.ravel(), minlength=5)
    assert hist[0] > 0 and hist[1] > 0 and hist[2] > 0 and hist[4] > 0
    Li, _ = rr.case_sources("identity", 1)
    assert (rr.remap(Li[0], rr.case_maps("identity")[0][3])[1] > 0).all()
    _, mx, _, s = rr.case_maps("far")[0]
    assert (~np.isfinite(mx)).any() and (np.isfinite(mx) & (np.abs(mx) >= 2.0 ** 15)).any()
    assert ((s[..., 0] == rr.OUTSIDE) == (s[..., 1] == rr.OUTSIDE)).all() and (s[..., 0] == rr.OUTSIDE).sum() >= 16


@pytest.mark.parametrize("cn", [1, 3])
def test_identity_returns_the_source(cn):
    L, _ = rr.case_sources("identity", cn)
    _, mx, my, s = rr.case_maps("identity")[0]
    assert np.array_equal(mx, np.broadcast_to(np.arange(67, dtype=np.float32), (35, 67)))
    assert np.array_equal(my, np.broadcast_to(np.arange(35, dtype=np.float32)[:, None], (35, 67)))
    assert np.array_equal(rr.remap(L[0], s)[0], L[0])


def test_principal_point_shift():
    """cx' = cx + 3: destination column j shows source column j - 3; the first three columns are the constant border."""
    cam = rr.Cam((100.0, 100.0, 30.0, 20.0), (0, 0, 0, 0, 0), None, (100.0, 100.0, 33.0, 20.0))
    _, mx, my = rr.build_maps(cam, 67, 35)
    out, n = rr.remap(rr.case_sources("identity", 1)[0][0], rr.fixed(mx, my))
    src = rr.case_sources("identity", 1)[0][0]
    assert np.array_equal(out[:, 3:], src[:, :-3])
    assert not out[:, :3].any() and not n[:, :2].any()


def test_rint_ties_go_to_even():
    k = np.array([[5.0, 6.0, -5.0, -6.0, 0.0, 1023.0]], np.float32)
    for frac, up in ((1.0 / 64, 0), (3.0 / 64, 2), (5.0 / 64, 2), (-1.0 / 64, 0), (-3.0 / 64, -2)):
        mx = k + np.float32(frac)
        assert np.array_equal((mx * np.float32(32)) % 1.0, np.full_like(k, 0.5)), "not an exact tie"
        s = rr.fixed(mx, np.zeros_like(mx))
        assert np.array_equal(s[..., 0], (32 * k).astype(np.int32) + up), frac
    # the range rule: |map * 32| >= 2^20 is outside, the largest value below it is not
    below = np.nextafter(np.float32(32768.0), np.float32(0))
    s = rr.fixed(np.array([[32768.0, below, -32768.0, np.inf, np.nan, 1.0]], np.float32), np.zeros((1, 6), np.float32))
    assert list(s[0, :, 0] == rr.OUTSIDE) == [True, False, True, True, True, False]
    assert s[0, 1, 0] == 2 ** 20 and (s[0, 1, 0] >> 5) == 32768


def _scalar_remap(src, sx, sy):
    """One pixel, one channel, written out tap by tap (independent of rect_ref.remap's array code)."""
    h, w = src.shape
    ix, iy, a, b = sx >> 5, sy >> 5, sx & 31, sy & 31
    acc, inside = 16384, 0
    for dy, dx, wt in ((0, 0, (32 - a) * (32 - b) * 32), (0, 1, a * (32 - b) * 32), (1, 0, (32 - a) * b * 32), (1, 1, a * b * 32)):
        y, x = iy + dy, ix + dx
        if 0 <= y < h and 0 <= x < w:
            acc += wt * int(src[y, x])
            inside += 1
    return acc >> 15, inside


def test_taps_at_borders_and_corners():
    src = rr.rand_u8(5, (5, 7)) | np.uint8(0x40)
    h, w = src.shape
    half = 16
    spots = {   # (ix, iy) of the upper-left tap, with a = b = 16 so that every tap has weight: taps inside
        "left": (-1, 2, 2), "right": (w - 1, 2, 2), "top": (3, -1, 2), "bottom": (3, h - 1, 2),
        "top-left": (-1, -1, 1), "top-right": (w - 1, -1, 1), "bottom-left": (-1, h - 1, 1), "bottom-right": (w - 1, h - 1, 1),
        "inside": (3, 2, 4), "beyond-left": (-2, 2, 0), "beyond-bottom": (3, h, 0),
    }
    sxsy = np.array([[[ix * 32 + half, iy * 32 + half] for ix, iy, _ in spots.values()]], np.int32)
    out, n = rr.remap(src, sxsy)
    for k, (name, (ix, iy, taps)) in enumerate(spots.items()):
        want, inside = _scalar_remap(src, ix * 32 + half, iy * 32 + half)
        assert inside == taps == n[0, k], name
        assert out[0, k] == want, name
        assert (want > 0) == (taps > 0), name
    # a = b = 0 on the last row / column: only the first tap has weight, and it is the source pixel
    s0 = np.array([[[(w - 1) * 32, (h - 1) * 32]]], np.int32)
    assert rr.remap(src, s0)[0][0, 0] == src[h - 1, w - 1]


def _undistort_project(cam, u, v):
    """(mapx, mapy) -> destination pixel: the distortion inverted by a fixed-point iteration in float64, then R and P."""
    fx, fy, cx, cy = cam.K
    k1, k2, p1, p2, k3 = cam.D
    xd, yd = (u - cx) / fx, (v - cy) / fy
    x, y = xd.copy(), yd.copy()
    for _ in range(60):
        r2 = x * x + y * y
        kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        x, y = (xd - dx) / kr, (yd - dy) / kr
    q = np.stack([x, y, np.ones_like(x)], axis=-1) @ cam.R.T
    return cam.P[0] * q[..., 0] / q[..., 2] + cam.P[2], cam.P[1] * q[..., 1] / q[..., 2] + cam.P[3]


@pytest.mark.parametrize("side", [0, 1])
def test_map_builder_inverts_to_the_pixel_grid(side):
    """Independent of the builder's own arithmetic: every destination pixel (j, i) of the EuRoC-like case, sent through its map
    value and back (distortion inverted iteratively, rotated by R, projected by P), returns to (j, i).  The only error of size is
    the float32 rounding of the map value: at most half an ulp of the largest map value per coordinate, carried back by the
    inverse mapping's Jacobian (finite differences, largest singular value over the image), times 1.5 for that estimate.
    Measured (Euclidean distance over both coordinates, pixels): left 5.98e-05 against a bound of 8.55e-05 (half ulp 3.05e-05,
    sigma_max 1.867, in the image corners), right 6.08e-05 against 8.63e-05 (sigma_max 1.884)."""
    cam = rr.cases()["euroc"][side]
    _, mx, my, _ = rr.case_maps("euroc")[side]
    u, v = mx.astype(np.float64), my.astype(np.float64)
    jj, ii = np.meshgrid(np.arange(752, dtype=np.float64), np.arange(480, dtype=np.float64))
    bj, bi = _undistort_project(cam, u, v)
    err = np.hypot(bj - jj, bi - ii).max()
    h = 1e-3
    ju1, iu1 = _undistort_project(cam, u + h, v)
    ju0, iu0 = _undistort_project(cam, u - h, v)
    jv1, iv1 = _undistort_project(cam, u, v + h)
    jv0, iv0 = _undistort_project(cam, u, v - h)
    J = np.stack([np.stack([ju1 - ju0, jv1 - jv0], -1), np.stack([iu1 - iu0, iv1 - iv0], -1)], -2) / (2 * h)
    smax = np.linalg.svd(J.reshape(-1, 2, 2), compute_uv=False)[:, 0].max()
    big = np.float32(max(np.abs(mx).max(), np.abs(my).max()))
    half_ulp = 0.5 * float(np.spacing(big))
    bound = half_ulp * smax * 1.5
    print("side %d: worst return error %.3e px, bound %.3e px (half ulp %.3e, sigma_max %.4f)" % (side, err, bound, half_ulp, smax))
    assert err <= bound


def test_settings_loader_euroc(pkg):
    s = pkg.load_rect_settings(os.path.join(rr.GOLDEN, "rect_euroc_like.yaml"))
    el, er, w, h = rr.euroc_cams()
    assert (s["src_w"], s["src_h"], s["dst_w"], s["dst_h"]) == (w, h, w, h)
    assert s["bf"] == 47.90639384423901
    for got, want in ((s["left"], el), (s["right"], er)):
        assert tuple(got.K) == want.K and tuple(got.D) == want.D and tuple(got.P) == want.P
        assert np.array_equal(np.array(got.R).reshape(3, 3), want.R)
    assert s["left"].R[1] == -0.001422739138722922 and s["right"].R[8] == 0.999945173484644   # (data: [...] over three lines)
    assert s["left"].K[:] == [458.654, 457.296, 367.215, 248.375] and s["right"].D[2] == -0.00010473


def test_settings_loader_flat_keys(pkg, tmp_path):
    s = pkg.load_rect_settings(os.path.join(rr.GOLDEN, "rect_flat_keys.yaml"))
    assert (s["src_w"], s["src_h"], s["bf"]) == (320, 240, 37.26)
    for cam in (s["left"], s["right"]):
        assert cam.K[:] == [310.5, 309.25, 160.75, 119.5] == cam.P[:]
        assert cam.D[:] == [-0.21, 0.045, 0.0007, -0.0004, -0.003]
        assert cam.R[:] == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    txt = open(os.path.join(rr.GOLDEN, "rect_flat_keys.yaml")).read()
    no_k3 = tmp_path / "no_k3.yaml"
    no_k3.write_text(txt.replace("Camera.k3: -0.003\n", ""))
    assert pkg.load_rect_settings(str(no_k3))["left"].D[4] == 0.0
    no_p1 = tmp_path / "no_p1.yaml"
    no_p1.write_text(txt.replace("Camera.p1: 0.0007\n", ""))
    with pytest.raises(pkg.SvoError, match="Camera.p1"):
        pkg.load_rect_settings(str(no_p1))
    half = tmp_path / "half.yaml"
    half.write_text(open(os.path.join(rr.GOLDEN, "rect_euroc_like.yaml")).read().replace("RIGHT.R:", "RIGHT.Q:"))
    with pytest.raises(pkg.SvoError, match="RIGHT.R"):
        pkg.load_rect_settings(str(half))


def test_argument_checks_touch_no_device(pkg):
    """svo_rect_create refuses on the host, before a device is looked for: SVO_E_INVALID (-1), never SVO_E_NODEVICE."""
    lib = pkg.load_library()
    lib.svo_rect_last_error.restype = C.c_char_p
    lib.svo_rect_last_error.argtypes = [C.c_void_p]
    lib.svo_rect_create.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    good = pkg.rect_cam((100.0, 100.0, 30.0, 20.0), (0.0, 0.0, 0.0, 0.0, 0.0))
    h = C.c_void_p()

    def create(sw=64, sh=48, dw=64, dh=48, left=good, right=good, out=C.byref(h)):
        return lib.svo_rect_create(0, sw, sh, dw, dh, None if left is None else C.addressof(left),
                                   None if right is None else C.addressof(right), out)

    assert create(out=None) == -1
    assert create(left=None) == -1 and create(right=None) == -1
    for bad in (dict(sw=7), dict(sh=8193), dict(dw=0), dict(dh=-5), dict(dw=8193), dict(dw=7), dict(sh=0), dict(dh=0), dict(sw=8193),
                dict(dh=8193)):
        assert create(**bad) == -1, bad
        assert b"8 .. 8192" in lib.svo_rect_last_error(None)
    nan = pkg.rect_cam((100.0, float("nan"), 30.0, 20.0), (0.0,) * 5)
    inf = pkg.rect_cam((100.0, 100.0, 30.0, 20.0), (0.0, float("inf"), 0.0, 0.0, 0.0))
    flat = pkg.rect_cam((100.0, 100.0, 30.0, 20.0), (0.0,) * 5, np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0.0]]))
    nof = pkg.rect_cam((100.0, 100.0, 30.0, 20.0), (0.0,) * 5, None, (0.0, 100.0, 30.0, 20.0))
    assert create(left=nan) == -1 and b"left" in lib.svo_rect_last_error(None)
    assert create(right=inf) == -1 and b"right" in lib.svo_rect_last_error(None)
    assert create(left=flat) == -1 and b"det" in lib.svo_rect_last_error(None)
    assert create(right=nof) == -1
    assert h.value is None
    # the other entries refuse a NULL object
    assert lib.svo_rect_destroy(None) == -1 and lib.svo_rect_sync(None) == -1
    lib.svo_rect_stream.restype = C.c_void_p
    assert lib.svo_rect_stream(None) is None
