"""Darknet detector behind the reference's own interfaces: the drop-in libYOLOv3SE.so (YoloLoad / YoloDetectFromImage /
YoloDetectFromFile, include/YOLOv3SE.h), stereo_kitti --detect / --write-boxes (the host YOLOv3 class), and a steady
detect -> track loop that reuses its box arrays with no host synchronisation."""
import ctypes as C
import importlib
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import darknet_ref as ref  # noqa: E402
import svo_loader  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "stereo-semantic-vo_amd")
HOST = os.path.join(PKG, "host")
YOLO3 = os.path.join(os.path.dirname(__file__), "golden", "tiny_yolo3_small.cfg")


@pytest.fixture(scope="module")
def pkg():
    return svo_loader.load()


def _png_rgb(rgb):
    H, W = rgb.shape[:2]
    raw = b"".join(b"\0" + rgb[y].tobytes() for y in range(H))
    chunk = lambda t, d: struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) +
            chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def _weights(tmp_path, seed, **kw):
    net = ref.parse_cfg(YOLO3)
    p = str(tmp_path / ("w%d.weights" % seed))
    ref.write_weights(p, ref.seeded_params(net, seed, **kw))
    return p


def _bgr(seed, W, H):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = (127 + 100 * np.sin(xx / 9.0 + seed) * np.cos(yy / 6.0)).astype(np.int64)
    return np.clip(base[:, :, None] + rng.integers(-40, 40, (H, W, 3)), 0, 255).astype(np.uint8)


def _planar(img_hwc):   # darknet's image from 8-bit bytes: (float)byte / 255. in planes
    return (img_hwc.astype(np.float32).astype(np.float64) / 255.).astype(np.float32).transpose(2, 0, 1).copy()


@pytest.mark.gpu
def test_shim_matches_device_entries(pkg, tmp_path):
    w = _weights(tmp_path, 4)
    lib = C.CDLL(os.path.join(PKG, "libYOLOv3SE.so"))
    lib.YoloLoad.restype = C.POINTER(C.c_int)
    lib.YoloLoad.argtypes = [C.c_char_p, C.c_char_p]
    lib.YoloDetectFromImage.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_float, C.c_void_p, C.c_int]
    lib.YoloDetectFromFile.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.c_float, C.c_void_p, C.c_int]
    net = lib.YoloLoad(YOLO3.encode(), w.encode())
    assert net
    det = pkg.Detector(YOLO3, w)
    W, H = 173, 101
    bgr = _bgr(2, W, H)
    want = det.detect(bgr, 0.5)                       # YOLOv3::Detect(cv::Mat): the BGR bytes unswapped
    assert len(want) >= 2
    pl = _planar(bgr)
    res = np.zeros(6000, np.float32)
    n = lib.YoloDetectFromImage(pl.ctypes.data, W, H, 3, net, 0.5, res.ctypes.data, 6000)
    assert res[:6 * n].reshape(-1, 6).tobytes() == want.tobytes()
    assert det.detect_planar(pl, 0.5).tobytes() == want.tobytes()
    # FromFile hands the net RGB (load_image_color): equal to FromImage on the RGB-swapped planes
    png = tmp_path / "img.png"
    png.write_bytes(_png_rgb(bgr[:, :, ::-1].copy()))
    res2 = np.zeros(6000, np.float32)
    n2 = lib.YoloDetectFromFile(str(png).encode(), net, 0.5, res2.ctypes.data, 6000)
    rgb_pl = _planar(bgr[:, :, ::-1].copy())
    res3 = np.zeros(6000, np.float32)
    n3 = lib.YoloDetectFromImage(rgb_pl.ctypes.data, W, H, 3, net, 0.5, res3.ctypes.data, 6000)
    assert n2 == n3 > 0
    assert res2[:6 * n2].tobytes() == res3[:6 * n3].tobytes()
    # truncation: result_sz = 11 holds one record
    res4 = np.zeros(11, np.float32)
    assert lib.YoloDetectFromImage(pl.ctypes.data, W, H, 3, net, 0.5, res4.ctypes.data, 11) == 1
    assert res4[:6].tobytes() == want[0].tobytes()
    det.close()


def _sequence(tmp_path, n):
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    L, R, _ = synth.render_sequence(n)
    L, R = L.numpy(), R.numpy()
    col = lambda x: np.stack([x, np.clip(x.astype(np.int32) + 9, 0, 255).astype(np.uint8), x], axis=2)
    seq = tmp_path / "seq"
    (seq / "image_2").mkdir(parents=True); (seq / "image_3").mkdir()
    for k in range(n):
        (seq / "image_2" / ("%06d.png" % k)).write_bytes(_png_rgb(col(L[k])[:, :, ::-1].copy()))
        (seq / "image_3" / ("%06d.png" % k)).write_bytes(_png_rgb(col(R[k])[:, :, ::-1].copy()))
    (seq / "times.txt").write_text("".join("%e\n" % (0.1 * k) for k in range(n)))
    y = tmp_path / "s.yaml"
    y.write_text("%YAML:1.0\nCamera.fx: 718.856\nCamera.fy: 718.856\nCamera.cx: 607.1928\nCamera.cy: 185.2157\n"
                 "Camera.width: 1241\nCamera.height: 376\nCamera.bf: 386.1448\n")
    return seq, y


def _run(tmp_path, name, args):
    d = tmp_path / name
    d.mkdir()
    p = subprocess.run([os.path.join(HOST, "stereo_kitti")] + args, capture_output=True, text=True, cwd=str(d))
    assert p.returncode == 0, p.stdout + p.stderr
    return (d / "cameratrajectory_kitti.txt").read_text()


@pytest.mark.gpu
def test_stereo_kitti_detect_end_to_end(pkg, tmp_path):
    """--detect tracks a synth sequence, serial and --pipelined, gray and --colour; --write-boxes writes the boxes each frame
    used, and feeding them back as offline boxes gives the same trajectory; without boxes the trajectory differs."""
    n = 6
    seq, y = _sequence(tmp_path, n)
    w = _weights(tmp_path, 5, obj_bias=2.5, cls_bias=2.5)
    base = ["voc", str(y), str(seq)]
    for colour in (False, True):
        c = ["--colour"] if colour else []
        wd = tmp_path / ("boxes_%d" % colour)
        wd.mkdir()
        online = _run(tmp_path, "det_%d" % colour, ["--detect", YOLO3, w, "0.8", "--write-boxes", str(wd)] + c + base)
        piped = _run(tmp_path, "det_pipe_%d" % colour, ["--detect", YOLO3, w, "0.8"] + c + ["--pipelined"] + base + ["3"])
        assert np.loadtxt(str(tmp_path / ("det_%d" % colour) / "cameratrajectory_kitti.txt")).shape == (n, 12)
        files = sorted(os.listdir(wd))
        assert len(files) == n and sum(len(open(wd / f).read().split()) for f in files) > 0
        # the written boxes as the offline input of the default mode
        os.symlink(str(wd), str(seq / "boxes"))
        offline = _run(tmp_path, "off_%d" % colour, c + base)
        offline_p = _run(tmp_path, "off_pipe_%d" % colour, c + ["--pipelined"] + base + ["3"])
        os.unlink(str(seq / "boxes"))
        none = _run(tmp_path, "none_%d" % colour, c + base)
        assert online == offline and piped == offline_p
        assert online != none, "the detector's boxes did not gate anything"


@pytest.mark.gpu
def test_steady_detect_track_loop_reuses_box_arrays(pkg, tmp_path):
    """Two rounds of svo_det_batch_dev(consumer) -> svo_track_batch_bgr_dev on the SAME box / record arrays, no host sync:
    the records equal the host-fed tracker given each round's boxes."""
    import torch
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    n, half = 8, 4
    L, R, _ = synth.render_sequence(n)
    L, R = L.numpy(), R.numpy()
    H, W = L.shape[1:]
    col = lambda a: np.stack([np.stack([x, np.clip(x.astype(np.int32) + 9, 0, 255).astype(np.uint8), x], axis=2) for x in a])
    cL, cR = col(L), col(R)
    det = pkg.Detector(YOLO3, _weights(tmp_path, 5, obj_bias=2.5, cls_bias=2.5), max_batch=half)
    ctx = pkg.Svo(W, H, max_batch=half)
    cam = pkg.Camera(**pkg.KITTI_00_02)
    ctx.track_reset(cam)
    dL, dR = torch.from_numpy(cL).cuda(), torch.from_numpy(cR).cuda()
    drec = torch.zeros(half * 64 * 6, dtype=torch.float32, device="cuda")
    dn = torch.zeros(half, dtype=torch.int32, device="cuda")
    bx = torch.zeros((half, 64, 4), dtype=torch.int32, device="cuda")
    bn = torch.zeros(half, dtype=torch.int32, device="cuda")
    rec = pkg.TRACK_DTYPE.itemsize
    out = torch.zeros(n * rec, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    bd = pkg.boxes_dev(bx.data_ptr(), bn.data_ptr(), 64)
    fb = H * W * 3
    for r in range(2):
        det.batch_dev(dL.data_ptr() + r * half * fb, W, H, 3, 3 * W, half, 0.8, drec.data_ptr(), 64, dn.data_ptr(), boxes=bd, consumer=ctx)
        ctx.track_batch_bgr_dev(dL.data_ptr() + r * half * fb, dR.data_ptr() + r * half * fb, 3 * W, half, out.data_ptr() + r * half * rec,
                                boxes=bd)
    ctx.sync()
    got = out.cpu().numpy().tobytes()
    # each round's boxes, from the detector alone
    hb, hn = [], []
    for r in range(2):
        for k in range(half):
            recs = det.detect(cL[r * half + k], 0.8, result_sz=6 * 64)
            b = np.zeros((64, 4), np.int32)
            tb = ref.tracker_boxes(recs)
            b[:len(tb)] = tb
            hb.append(b)
            hn.append(len(tb))
    hb, hn = np.stack(hb), np.array(hn, np.int32)
    assert hn.sum() > 0
    ctx.track_reset(cam)
    res = np.zeros(n, pkg.TRACK_DTYPE)
    cLc, cRc = np.ascontiguousarray(cL), np.ascontiguousarray(cR)
    for r in range(2):
        k0 = r * half
        ctx.track_batch_bgr_host(cLc.ctypes.data + k0 * fb, cRc.ctypes.data + k0 * fb, 3 * W, half, res[k0:k0 + half],
                                 boxes=pkg.boxes_host(hb[k0:k0 + half], hn[k0:k0 + half]))
    ctx.sync()
    assert res.tobytes() == got
    ctx.close()
    det.close()


@pytest.mark.gpu
def test_layer_times(pkg, tmp_path):
    det = pkg.Detector(YOLO3, _weights(tmp_path, 6))
    det.profile(True)
    det.detect(_bgr(1, 120, 80), 0.5)
    t = det.layer_times()
    assert len(t) == len(det.layers) + 2 and (t >= 0).all() and t.sum() > 0
    det.close()
