"""GPU suite of the rectification stage (svo_rect_*): the device's maps and images against the numpy restatement of DESIGN.md
section 8 (tests/rect_ref.py, pinned by tests/golden/rect_restatement_pins.json), bit for bit."""
import numpy as np
import pytest

import rect_ref as rr

SENTINEL = 0xA5


def _rectifier(pkg, name):
    cl, cr, sw, sh, dw, dh = rr.cases()[name]
    cams = [pkg.rect_cam(c.K, c.D, c.R, c.P) for c in (cl, cr)]
    return pkg.Rectifier(sw, sh, cams[0], cams[1], dw, dh)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small", "small_lr", "identity", "euroc", "wide", "tiny", "far"])
def test_maps_bit_for_bit(pkg, name):
    """iR, both float maps and sx / sy of both sides.  (A NaN equals a NaN: its sign and payload are the machine's.)"""
    rect = _rectifier(pkg, name)
    for side in range(2):
        ir, mx, my, s = rr.case_maps(name)[side]
        g_ir, g_mx, g_my, g_s = rect.maps(side)
        assert g_ir.tobytes() == ir.tobytes(), (name, side)
        assert rr.same_floats(g_mx, mx), (name, side, "mapx", int((g_mx.view(np.uint32) != mx.view(np.uint32)).sum()))
        assert rr.same_floats(g_my, my), (name, side, "mapy", int((g_my.view(np.uint32) != my.view(np.uint32)).sum()))
        assert np.array_equal(g_s, s), (name, side, "sxsy", int((g_s != s).any(axis=-1).sum()))
    rect.close()


def _strides(name, cn):
    """(source stride, destination stride) in bytes: the strong small case has padded rows on both sides."""
    _, _, sw, _, dw, _ = rr.cases()[name]
    if name == "small":
        return (80, 64) if cn == 1 else (208, 192)
    if name == "wide":
        return cn * sw + 3, cn * dw + 1   # (a destination stride that is no multiple of 4: the byte-store path)
    return cn * sw, cn * dw


def _padded(imgs, stride):
    """B x H x W (x 3) -> B x H x stride bytes, padding = SENTINEL."""
    B, H = imgs.shape[:2]
    flat = imgs.reshape(B, H, -1)
    out = np.full((B, H, stride), SENTINEL, np.uint8)
    out[:, :, :flat.shape[2]] = flat
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("name,B", [("small", 1), ("small", 3), ("wide", 1), ("wide", 3), ("tiny", 1), ("tiny", 3), ("identity", 3),
                                    ("far", 1), ("small_lr", 5)])
def test_images_bit_for_bit(pkg, name, B, cn):
    """svo_rect_batch_dev on B resident pairs, padded rows on both sides: every pixel equals the restatement's, the destination
    rows' padding keeps its sentinel, and svo_rect_process gives the same bytes for every pair."""
    import torch
    _, _, sw, sh, dw, dh = rr.cases()[name]
    L, R = rr.case_sources(name, cn, B)
    ss, ds = _strides(name, cn)
    rect = _rectifier(pkg, name)
    dL, dR = torch.from_numpy(_padded(L, ss)).cuda(), torch.from_numpy(_padded(R, ss)).cuda()
    oL = torch.full((B, dh, ds), SENTINEL, dtype=torch.uint8, device="cuda")
    oR = torch.full((B, dh, ds), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rect.batch_dev(dL, dR, ss, cn, B, oL, oR, ds)
    rect.sync()
    got = [oL.cpu().numpy(), oR.cpu().numpy()]
    taps = np.zeros(5, np.int64)
    for side, src in enumerate((L, R)):
        s = rr.case_maps(name)[side][3]
        assert (got[side][:, :, cn * dw:] == SENTINEL).all(), "padding bytes of the destination rows were written"
        for b in range(B):
            want, n = rr.remap(src[b], s)
            taps += np.bincount(n.ravel(), minlength=5)
            g = got[side][b, :, :cn * dw].reshape(want.shape)
            assert np.array_equal(g, want), (name, side, b, int((g != want).sum()))
    if name == "small":
        assert taps[0] > 0 and taps[1] > 0 and taps[2] > 0 and taps[4] > 0
    if name == "identity":
        assert taps[0] == 0
        assert np.array_equal(got[0][:, :, :cn * dw].reshape(L.shape), L)
    # host to host: the same bytes, pair by pair, from views of the padded sources into padded outputs
    shape = (sh, sw) if cn == 1 else (sh, sw, 3)
    for b in range(B):
        vL = np.lib.stride_tricks.as_strided(_padded(L, ss)[b], shape, (ss, 1) if cn == 1 else (ss, 3, 1))
        vR = np.lib.stride_tricks.as_strided(_padded(R, ss)[b], shape, (ss, 1) if cn == 1 else (ss, 3, 1))
        pL, pR = rect.process(vL, vR, out_stride=ds)
        assert pL.tobytes() == got[0][b].tobytes() and pR.tobytes() == got[1][b].tobytes(), (name, b)
    rect.close()


@pytest.mark.gpu
def test_image_argument_checks(pkg):
    import torch
    rect = _rectifier(pkg, "tiny")
    d = torch.zeros(4 * 8 * 24, dtype=torch.uint8, device="cuda")
    p = d.data_ptr()
    ok = dict(d_L=p, d_R=p, src_stride=8, cn=1, B=1, d_outL=p, d_outR=p, dst_stride=8)
    for bad in (dict(d_L=0), dict(d_outR=0), dict(cn=2), dict(cn=4), dict(src_stride=7), dict(dst_stride=7), dict(B=0), dict(B=-1),
                dict(cn=3, src_stride=23, dst_stride=24), dict(cn=3, src_stride=24, dst_stride=23)):
        with pytest.raises(pkg.SvoError, match="invalid"):
            rect.batch_dev(**{**ok, **bad})
    with pytest.raises(pkg.SvoError, match="invalid"):
        rect.process(np.zeros((8, 8, 2), np.uint8), np.zeros((8, 8, 2), np.uint8))
    cam = rect.camera(bf=12.5)
    c = rr.cases()["tiny"][0]
    assert (cam.fx, cam.fy, cam.cx, cam.cy, cam.bf) == tuple(np.float32(v) for v in c.P) + (12.5,)
    assert rect.stream
    rect.close()


@pytest.mark.gpu
def test_batch_beyond_one_launch(pkg):
    """B = 131,071 tiny pairs: more than one launch's grid holds (2 x 32,767 slices of 4 images), so the call is chunked; the
    last launch has 3 images.  The restatement takes the batch as the channels of one image."""
    import torch
    B = 131068 + 3
    L, R = rr.case_sources("tiny", 1, B, seed=23)
    rect = _rectifier(pkg, "tiny")
    dL, dR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    oL = torch.full((B, 8, 8), SENTINEL, dtype=torch.uint8, device="cuda")
    oR = torch.full((B, 8, 8), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rect.batch_dev(dL, dR, 8, 1, B, oL, oR, 8)
    rect.sync()
    for side, (src, got) in enumerate(((L, oL), (R, oR))):
        want = rr.remap(np.ascontiguousarray(src.transpose(1, 2, 0)), rr.case_maps("tiny")[side][3])[0]
        g = got.cpu().numpy().transpose(1, 2, 0)
        assert np.array_equal(g, want), (side, np.flatnonzero((g != want).any(axis=(0, 1)))[:5])
    rect.close()
