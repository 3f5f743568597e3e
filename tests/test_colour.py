"""Colour (8UC3 BGR) input: the reference's driver reads KITTI image_2 / image_3 unchanged (main.cpp:160-161), cv::ORB reduces
them to gray with COLOR_BGR2GRAY's fixed point (src/frame.cc:75-79) and frame::MB hands the colour itself to MSA::solve
(src/frame.cc:82-91).  CPU: the C-ABI declares, binds and exports the colour entries; the host driver decodes colour files to
BGR and its gray decode is that fixed point.  GPU (-m gpu): k_bgr2gray is that fixed point on every BGR triple; colour of a gray
image tracks exactly like the gray; true colour tracks like its gray at depth sources 0 / 1 and like the oracle fed the colour
MSA maps at depth source 2; the batched and host-fed colour entries equal the frame-by-frame one; the host classes and the
driver take colour through."""
import ctypes as C
import importlib
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "stereo-semantic-vo_amd", "host")
NEW = ["svo_bgr_to_gray", "svo_track_frame_bgr", "svo_track_batch_bgr_dev", "svo_track_batch_bgr_host"]


def np_gray(bgr):
    """cv::cvtColor(COLOR_BGR2GRAY) for 8U: (1868 B + 9617 G + 4899 R + 8192) >> 14."""
    a = np.asarray(bgr).astype(np.int64)
    return ((a[..., 0] * 1868 + a[..., 1] * 9617 + a[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def as_bgr(g):
    return np.ascontiguousarray(np.repeat(np.asarray(g)[..., None], 3, -1))


def colourise(g):
    """Deterministic colour from a gray frame: per-channel look-up tables of the gray value plus a tint that depends on the
    row only - the channels differ, and the left / right images of a rectified pair stay consistent."""
    v = np.asarray(g).astype(np.int32)
    row = np.arange(v.shape[-2], dtype=np.int32)[:, None]
    b = np.clip((v * 7) // 8 + 16 + row % 9, 0, 255)
    gg = np.clip(v + row % 5 - 2, 0, 255)
    r = np.clip((v * v) // 255 + 12 + (row // 3) % 11, 0, 255)
    return np.ascontiguousarray(np.stack([b, gg, r], -1).astype(np.uint8))


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_colour_entries_declared_bound_and_exported(pkg):
    hdr = open(os.path.join(ROOT, "include", "svo.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in pkg.ABI_SYMBOLS, name
    assert re.search(r"#define SVO_ABI_VERSION 8\b", hdr)
    lib = os.path.join(ROOT, "stereo-semantic-vo_amd", "libsvo_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
    for name in NEW:
        assert name in exported, name
    for m in ("bgr_to_gray", "track_frame_bgr", "track_batch_bgr_dev", "track_batch_bgr_host"):
        assert callable(getattr(pkg.Svo, m, None)), m


def _png(img, colour_type):
    """A PNG file (8-bit, filter 0 on every row) of an H x W x C array, written with the standard library only."""
    H, W = img.shape[:2]
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(H))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, colour_type, 0, 0, 0)) +
            chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def _read_ppm(path):
    data = open(path, "rb").read()
    m = re.match(rb"P6\s+(\d+)\s+(\d+)\s+255\s", data)
    assert m, data[:20]
    W, H = int(m.group(1)), int(m.group(2))
    return np.frombuffer(data, np.uint8, W * H * 3, m.end()).reshape(H, W, 3)


def _read_pgm(path):
    data = open(path, "rb").read()
    m = re.match(rb"P5\s+(\d+)\s+(\d+)\s+255\s", data)
    assert m, data[:20]
    W, H = int(m.group(1)), int(m.group(2))
    return np.frombuffer(data, np.uint8, W * H, m.end()).reshape(H, W)


@pytest.fixture(scope="module")
def stereo_kitti():
    exe = os.path.join(HOST, "stereo_kitti")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", HOST, "-s"])
    return exe


def test_driver_decodes_colour_files_to_bgr(stereo_kitti, tmp_path):
    """--decode-bgr: an RGB PNG, an RGBA PNG (alpha dropped), a gray PNG (B = G = R) and a binary P6 PPM, written here, come
    out as the BGR bytes cv::imread gives."""
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (13, 29, 3), dtype=np.uint8)
    rgba = rng.integers(0, 256, (7, 11, 4), dtype=np.uint8)
    gray = rng.integers(0, 256, (9, 10), dtype=np.uint8)
    cases = [("rgb.png", _png(rgb, 2), rgb[..., ::-1]),
             ("rgba.png", _png(rgba, 6), rgba[..., 2::-1]),
             ("gray.png", _png(gray[..., None], 0), as_bgr(gray)),
             ("rgb.ppm", b"P6\n# comment\n29 13\n255\n" + rgb.tobytes(), rgb[..., ::-1])]
    for name, data, want in cases:
        src, dst = tmp_path / name, tmp_path / (name + ".out.ppm")
        src.write_bytes(data)
        subprocess.run([stereo_kitti, "--decode-bgr", str(src), str(dst)], check=True, capture_output=True)
        got = _read_ppm(str(dst))[..., ::-1]       # the PPM holds RGB; the BGR the driver decoded is its reverse
        assert np.array_equal(got, want), name


def test_driver_gray_decode_is_the_fixed_point_formula(stereo_kitti, tmp_path):
    """The existing gray --decode of a colour PNG equals cv::cvtColor(COLOR_BGR2GRAY)'s fixed point computed in numpy."""
    rng = np.random.default_rng(6)
    rgb = rng.integers(0, 256, (17, 23, 3), dtype=np.uint8)
    src, dst = tmp_path / "c.png", tmp_path / "c.pgm"
    src.write_bytes(_png(rgb, 2))
    subprocess.run([stereo_kitti, "--decode", str(src), str(dst)], check=True, capture_output=True)
    assert np.array_equal(_read_pgm(str(dst)), np_gray(rgb[..., ::-1]))


# ---- GPU ------------------------------------------------------------------------------------------------------------------

N_FRAMES = 8
BOXED = {2: [[300, 560, 120, 330]], 5: [[80, 340, 150, 330], [700, 900, 100, 250]], 6: [[500, 800, 140, 300]]}


@pytest.fixture(scope="module")
def frames(pkg):
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    L, R, _ = synth.render_sequence(N_FRAMES)
    L, R = L.numpy(), R.numpy()
    cL = np.stack([colourise(x) for x in L]); cR = np.stack([colourise(x) for x in R])
    return dict(L=L, R=R, cL=cL, cR=cR, W=L.shape[2], H=L.shape[1])


def _convert(ctx, buf, W, H, stride, gray_stride):
    buf = np.ascontiguousarray(buf)
    out = np.full((H, gray_stride), 0xA5, np.uint8)
    rc = ctx.lib.svo_bgr_to_gray(ctx.h, buf.ctypes.data_as(C.c_void_p), W, H, stride, out.ctypes.data_as(C.c_void_p), gray_stride)
    assert rc == 0, ctx.lib.svo_last_error(ctx.h)
    assert (out[:, W:] == 0xA5).all()                  # nothing written past the row
    return out[:, :W]


@pytest.mark.gpu
def test_bgr_to_gray_exhaustive(pkg):
    """Every one of the 2^24 BGR triples once (4096 x 4096, rows 3 * 4096 + 5 bytes apart: the rows start at every byte offset
    of a dword), a KITTI-sized image with stride 3 * 1241 + 1, and widths 1..9 with odd strides - against the numpy formula."""
    ctx = pkg.Svo(640, 240)
    W = H = 4096
    stride = 3 * W + 5
    i = np.arange(W * H, dtype=np.uint32).reshape(H, W)
    buf = np.zeros((H, stride), np.uint8)
    tri = np.stack([i & 255, (i >> 8) & 255, i >> 16], -1).astype(np.uint8)
    buf[:, :3 * W] = tri.reshape(H, 3 * W)
    got = _convert(ctx, buf, W, H, stride, W)
    assert np.array_equal(got, np_gray(tri))
    assert np.array_equal(np_gray(as_bgr(np.arange(256, dtype=np.uint8))), np.arange(256, dtype=np.uint8))
    rng = np.random.default_rng(11)
    W, H = 1241, 376
    stride = 3 * W + 1
    buf = rng.integers(0, 256, (H, stride), dtype=np.uint8)
    got = _convert(ctx, buf, W, H, stride, W + 3)
    assert np.array_equal(got, np_gray(buf[:, :3 * W].reshape(H, W, 3)))
    for W in range(1, 10):
        for pad in (0, 1, 2, 3, 7):
            stride = 3 * W + pad
            buf = rng.integers(0, 256, (5, stride), dtype=np.uint8)
            got = _convert(ctx, buf, W, 5, stride, W + pad % 3)
            assert np.array_equal(got, np_gray(buf[:, :3 * W].reshape(5, W, 3))), (W, pad)
    assert np.array_equal(ctx.bgr_to_gray(tri[:64, :64]), np_gray(tri[:64, :64]))
    ctx.close()


def _track(pkg, f, depth_source, colour, imgs=None, boxes=True, n=N_FRAMES):
    ctx = pkg.Svo(f["W"], f["H"])
    ctx.set_option("depth_source", depth_source)
    if depth_source == 2:
        ctx.set_option("epnp_exact", 1)
    ctx.track_reset(pkg.Camera(**pkg.KITTI_00_02))
    L, R = imgs if imgs is not None else ((f["cL"], f["cR"]) if colour else (f["L"], f["R"]))
    out = []
    for k in range(n):
        bx = BOXED.get(k) if boxes else None
        res = (ctx.track_frame_bgr if colour else ctx.track_frame)(L[k], R[k], boxes=bx)
        out.append((res.tobytes(), ctx.debug_track_matches().tobytes()))
    assert ctx.track_overflowed() == 0
    ctx.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("depth_source", [0, 1, 2])
def test_colour_of_gray_tracks_like_gray(pkg, frames, depth_source):
    """B = G = R copies of the gray frames through track_frame_bgr == track_frame on the gray, records and matches byte for
    byte (MSA gets the same B = G = R image either way)."""
    f = frames
    n = N_FRAMES if depth_source == 0 else 3
    gray = _track(pkg, f, depth_source, False, n=n)
    col = _track(pkg, f, depth_source, True, imgs=(as_bgr(f["L"]), as_bgr(f["R"])), n=n)
    assert col == gray


@pytest.mark.gpu
@pytest.mark.parametrize("depth_source", [0, 1])
def test_true_colour_sparse_and_elas_depth_track_like_their_gray(pkg, frames, depth_source):
    """ORB, the sparse matcher and ELAS run on the device gray: track_frame_bgr(colour) == track_frame(numpy gray)."""
    f = frames
    n = N_FRAMES if depth_source == 0 else 3
    want = _track(pkg, f, depth_source, False, imgs=(np_gray(f["cL"]), np_gray(f["cR"])), n=n)
    got = _track(pkg, f, depth_source, True, n=n)
    assert got == want


def _check_frame(k, res, cur, ref, ref_cur):
    """(tests/test_track.py's check, exact mode)"""
    for fld in ("frame_id", "n_kp", "n_stereo", "n_match_pass1", "n_match_pass2", "n_lm_edges", "n_new_mappoints", "n_local_map"):
        assert res[fld] == ref[fld], (k, fld, res[fld], ref[fld])
    assert np.array_equal(cur[:ref["n_kp"]], ref_cur[:ref["n_kp"]]), "frame %d match indices" % k
    assert res["n_pnp_inliers"] == ref["n_pnp_inliers"] and res["lm_iterations"] == ref["lm_iterations"], k
    assert res["Tcw"].tobytes() == ref["Tcw"].tobytes(), k


@pytest.mark.gpu
def test_true_colour_msa_depth_matches_oracle_on_colour(orc, pkg, frames):
    """depth_source 2 on colour: ORB on the gray, MSA::solve(l, r, 48, 1) on the COLOUR pair - the oracle tracker fed the
    numpy gray and the CPU restatement's maps of the colour pair.  The colour maps differ from the B = G = R maps, and the
    records differ from a gray-fed run somewhere: the colour reached MSA."""
    from oracle import binding as ob
    f = frames
    n = 3
    trk = orc.Tracker(f["W"], f["H"], pkg.KITTI_00_02)
    ctx = pkg.Svo(f["W"], f["H"])
    ctx.set_option("depth_source", 2)
    ctx.set_option("epnp_exact", 1)
    ctx.track_reset(pkg.Camera(**pkg.KITTI_00_02))
    recs = []
    for k in range(n):
        gL, gR = np_gray(f["cL"][k]), np_gray(f["cR"][k])
        dmap = ob.msa_solve(f["cL"][k], f["cR"][k], 48, 1)
        if k == 0:
            grey_map = ob.msa_solve(as_bgr(gL), as_bgr(gR), 48, 1)
            assert (dmap != grey_map).mean() > 0.02, (dmap != grey_map).mean()
        ref, ref_cur = trk.track(gL, gR, dense=dmap.astype(np.float32))
        res = ctx.track_frame_bgr(f["cL"][k], f["cR"][k])
        _check_frame(k, res, ctx.debug_track_matches(), ref, ref_cur)
        assert res["n_stereo"] > 100
        recs.append(res.tobytes())
    trk.close()
    ctx.close()
    grey = _track(pkg, f, 2, False, imgs=(np_gray(f["cL"]), np_gray(f["cR"])), boxes=False, n=n)
    assert any(r != g for r, (g, _) in zip(recs, grey))


def _resident(f, n, pitch):
    import torch
    dev = torch.device("cuda", 0)
    dL = torch.zeros((n, f["H"], pitch), dtype=torch.uint8, device=dev); dR = torch.zeros_like(dL)
    W3 = 3 * f["W"]
    dL[:, :, :W3] = torch.from_numpy(f["cL"][:n].reshape(n, f["H"], W3)).to(dev)
    dR[:, :, :W3] = torch.from_numpy(f["cR"][:n].reshape(n, f["H"], W3)).to(dev)
    return dL, dR


def _boxes_dev(pkg, n):
    import torch
    b = np.zeros((n, 2, 4), np.int32); c = np.zeros(n, np.int32)
    for k, bl in BOXED.items():
        if k < n:
            b[k, :len(bl)] = bl; c[k] = len(bl)
    tb, tn = torch.from_numpy(b).cuda(), torch.from_numpy(c).cuda()
    return (tb, tn), b, c


@pytest.fixture(scope="module")
def long_frames(pkg):
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    n = 40
    L, R, _ = synth.render_sequence(n)
    L, R = L.numpy(), R.numpy()
    return dict(cL=np.stack([colourise(x) for x in L]), cR=np.stack([colourise(x) for x in R]), W=L.shape[2], H=L.shape[1], n=n)


def _frame_by_frame(pkg, f, depth_source, n):
    ctx = pkg.Svo(f["W"], f["H"])
    ctx.set_option("depth_source", depth_source)
    ctx.track_reset(pkg.Camera(**pkg.KITTI_00_02))
    out = b"".join(ctx.track_frame_bgr(f["cL"][k], f["cR"][k], boxes=BOXED.get(k)).tobytes() for k in range(n))
    ctx.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("depth_source,n", [(0, 40), (1, 4), (2, 3)])
def test_batched_and_host_fed_colour_equal_frame_by_frame(pkg, long_frames, depth_source, n):
    """svo_track_batch_bgr_dev (40 pairs = two front-end sub-batches, rows 3 W + 37 bytes apart, boxes) == track_frame_bgr
    frame by frame; svo_track_batch_bgr_host from pinned and from pageable memory, cut into two calls without a sync in between,
    == the resident call."""
    import torch
    f = long_frames
    want = _frame_by_frame(pkg, f, depth_source, n)
    pitch = 3 * f["W"] + 37
    dL, dR = _resident(f, n, pitch)
    (tb, tn), hb, hn = _boxes_dev(pkg, n)
    rec = pkg.TRACK_DTYPE.itemsize
    ctx = pkg.Svo(f["W"], f["H"], max_batch=n)
    ctx.set_option("depth_source", depth_source)
    ctx.track_reset(pkg.Camera(**pkg.KITTI_00_02))
    out = torch.zeros(n * rec, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.track_batch_bgr_dev(dL.data_ptr(), dR.data_ptr(), pitch, n, out.data_ptr(), boxes=pkg.boxes_dev(tb.data_ptr(), tn.data_ptr(), 2))
    ctx.sync()
    assert out.cpu().numpy().tobytes() == want
    hL, hR = dL.cpu().numpy(), dR.cpu().numpy()
    fb = f["H"] * pitch
    cut = [n // 2, n - n // 2]
    for source in ("pinned", "pageable"):
        if source == "pinned":
            keep = (torch.from_numpy(hL).pin_memory(), torch.from_numpy(hR).pin_memory())
            pl, pr = keep[0].data_ptr(), keep[1].data_ptr()
        else:
            pl, pr = hL.ctypes.data, hR.ctypes.data
        ctx.track_reset(pkg.Camera(**pkg.KITTI_00_02))
        res = np.zeros(n, pkg.TRACK_DTYPE)
        k0 = 0
        for B in cut:
            bx = pkg.boxes_host(hb[k0:k0 + B], hn[k0:k0 + B])
            ctx.track_batch_bgr_host(pl + k0 * fb, pr + k0 * fb, pitch, B, res[k0:k0 + B], boxes=bx)
            k0 += B
        ctx.sync()
        assert res.tobytes() == want, source
    assert ctx.track_overflowed() == 0
    ctx.close()


@pytest.mark.gpu
def test_gray_and_colour_calls_mix_within_a_sequence(pkg, frames):
    """Gray and colour frames may follow each other: each record is what its own pixels imply."""
    f = frames
    gL, gR = np_gray(f["cL"]), np_gray(f["cR"])
    want = _track(pkg, f, 0, False, imgs=(gL, gR))
    ctx = pkg.Svo(f["W"], f["H"])
    ctx.track_reset(pkg.Camera(**pkg.KITTI_00_02))
    got = []
    for k in range(N_FRAMES):
        res = ctx.track_frame_bgr(f["cL"][k], f["cR"][k], boxes=BOXED.get(k)) if k % 2 else ctx.track_frame(gL[k], gR[k], boxes=BOXED.get(k))
        got.append((res.tobytes(), ctx.debug_track_matches().tobytes()))
    ctx.close()
    assert got == want


@pytest.mark.gpu
def test_colour_argument_checks(pkg, frames):
    import torch
    f = frames
    W, H = f["W"], f["H"]
    ctx = pkg.Svo(W, H, max_batch=2)
    ctx.track_reset(pkg.Camera(**pkg.KITTI_00_02))
    lib = ctx.lib
    a = np.zeros((H, 3 * W), np.uint8)
    res = np.zeros(4, pkg.TRACK_DTYPE)
    p, r = a.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p)
    assert lib.svo_track_frame_bgr(ctx.h, p, 3 * W - 1, p, 3 * W, C.c_double(0), None, 0, r) == -1
    assert lib.svo_track_batch_bgr_host(ctx.h, p, p, 3 * W - 1, 1, None, r) == -1
    assert lib.svo_track_batch_bgr_host(ctx.h, p, p, 3 * W, 3, None, r) == -5
    d = torch.zeros(3 * H * 3 * W, dtype=torch.uint8, device="cuda")
    dr = torch.zeros(4 * pkg.TRACK_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    dp, drp = C.c_void_p(d.data_ptr()), C.c_void_p(dr.data_ptr())
    assert lib.svo_track_batch_bgr_dev(ctx.h, dp, dp, 3 * W - 1, 1, None, drp) == -1
    assert lib.svo_track_batch_bgr_dev(ctx.h, dp, dp, 3 * W, 3, None, drp) == -5
    assert lib.svo_bgr_to_gray(ctx.h, p, 4, 4, 11, p, 4) == -1
    assert lib.svo_bgr_to_gray(ctx.h, p, 4, 4, 12, p, 3) == -1
    ctx.close()


def _colour_sequence(tmp_path, f, n, boxes=True):
    seq = tmp_path / "seq"
    (seq / "image_2").mkdir(parents=True); (seq / "image_3").mkdir(); (seq / "boxes").mkdir()
    for k in range(n):
        (seq / "image_2" / ("%06d.png" % k)).write_bytes(_png(f["cL"][k][..., ::-1], 2))
        (seq / "image_3" / ("%06d.png" % k)).write_bytes(_png(f["cR"][k][..., ::-1], 2))
        if boxes and k in BOXED:
            (seq / "boxes" / ("%d.txt" % (k + 1))).write_text("".join("%d %d %d %d\n" % tuple(b) for b in BOXED[k]))
    (seq / "times.txt").write_text("".join("%e\n" % (0.1 * k) for k in range(n)))
    return seq


@pytest.mark.gpu
def test_host_classes_with_colour_msa_equal_device_tracker(pkg, frames, tmp_path):
    """host_check msa-colour: featuredetect on the device gray, colour MBdense, computekeypoint_r, disp2Depth == svo_track_frame_bgr
    with depth_source 2."""
    seq = _colour_sequence(tmp_path, frames, 3, boxes=False)
    p = subprocess.run([os.path.join(HOST, "host_check"), str(seq), "3", "msa-colour"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    worst = [float(ln.split()[1]) for ln in p.stdout.splitlines() if ln.startswith("worst")]
    assert worst and worst[0] < 1e-3


@pytest.mark.gpu
def test_stereo_kitti_colour_writes_the_gray_trajectory(pkg, frames, tmp_path):
    """stereo_kitti --colour, frame by frame and --pipelined, on a colour image_2 / image_3 sequence with boxes: the trajectory
    files equal the default (gray-decoding) run's on the same files - at depth source 0 ORB sees the same gray by construction."""
    n = N_FRAMES
    seq = _colour_sequence(tmp_path, frames, n)
    y = tmp_path / "s.yaml"
    y.write_text("%YAML:1.0\nCamera.fx: 718.856\nCamera.fy: 718.856\nCamera.cx: 607.1928\nCamera.cy: 185.2157\n"
                 "Camera.width: 1241\nCamera.height: 376\nCamera.bf: 386.1448\n")
    out = {}
    for mode in ("frame", "pipelined"):
        for colour in (False, True):
            d = tmp_path / ("%s_%d" % (mode, colour))
            d.mkdir()
            cmd = ([os.path.join(HOST, "stereo_kitti")] + (["--colour"] if colour else []) +
                   (["--pipelined"] if mode == "pipelined" else []) + ["voc", str(y), str(seq)] + (["3"] if mode == "pipelined" else []))
            p = subprocess.run(cmd, capture_output=True, text=True, cwd=str(d))
            assert p.returncode == 0, p.stdout + p.stderr
            out[(mode, colour)] = ((d / "cameratrajectory_kitti.txt").read_text(), (d / "cameratrajectory_tum.txt").read_text())
        assert out[(mode, True)] == out[(mode, False)], mode
        assert np.loadtxt(str(tmp_path / ("%s_1" % mode) / "cameratrajectory_kitti.txt")).shape == (n, 12)
