"""Darknet detector on the device (svo_det_*) against the independent restatement in darknet_ref.py: the input tensor bit
for bit, every layer within a bound calibrated from the oracle's float32 / float64 pair, decode + NMS + records byte for
byte from the device's own raw outputs, the batched entry against the latency entry, detector-fed tracking with no host
synchronisation in between, and argument checks."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import darknet_ref as ref  # noqa: E402
import svo_loader  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
YOLO3 = os.path.join(GOLD, "tiny_yolo3_small.cfg")
REGION = os.path.join(GOLD, "tiny_region_small.cfg")
D53 = os.path.join(GOLD, "darknet53_coco.cfg")
THRESH = 0.5
THRESH_OF = {YOLO3: 0.5, REGION: 0.25, D53: 0.5}   # (softmax spreads the region head's scores: a lower threshold lets some pass)


@pytest.fixture(scope="module")
def pkg():
    return svo_loader.load()


def _image(seed, W, H, C=3):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = (127 + 100 * np.sin(xx / 7.0 + seed) * np.cos(yy / 5.0)).astype(np.int64)
    img = np.clip(base[:, :, None] + rng.integers(-40, 40, (H, W, C)), 0, 255).astype(np.uint8)
    return img if C == 3 else img[:, :, 0]


def _weights(tmp_path, cfg, seed, **kw):
    net = ref.parse_cfg(cfg)
    params = ref.seeded_params(net, seed, **kw)
    p = str(tmp_path / ("%s_%d.weights" % (os.path.basename(cfg), seed)))
    ref.write_weights(p, params)
    return net, params, p


def _bound_ok(gpu, f32, f64):
    err = np.abs(gpu.astype(np.float64) - f64).max()
    bound = 4 * np.abs(f32.astype(np.float64) - f64).max() + 1e-6 * np.abs(f64).max()
    return err <= bound, err, bound


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["bgr_1241x376", "gray", "odd_size", "padded_stride"])
def test_input_tensor_bit_identical(pkg, tmp_path, case):
    cfg = YOLO3
    if case == "bgr_1241x376":     # (only the network's input size matters here: the small network at 416 x 416)
        cfg = str(tmp_path / "yolo3_416.cfg")
        open(cfg, "w").write(open(YOLO3).read().replace("width=96", "width=416").replace("height=64", "height=416"))
    net, params, w = _weights(tmp_path, cfg, 3)
    W, H, C_ = {"bgr_1241x376": (1241, 376, 3), "gray": (200, 90, 1), "odd_size": (77, 131, 3), "padded_stride": (101, 57, 3)}[case]
    img = _image(5, W, H, C_)
    det = pkg.Detector(cfg, w)
    if case == "padded_stride":
        padded = np.zeros((H, W * 3 + 13), np.uint8)
        padded[:, :W * 3] = img.reshape(H, -1)
        n = C.c_int(0)
        res = np.zeros(600, np.float32)
        rc = det.lib.svo_det_detect(det.h, padded.ctypes.data_as(C.c_void_p), W, H, 3, W * 3 + 13, THRESH,
                                    res.ctypes.data_as(C.c_void_p), 600, C.byref(n))
        assert rc == 0
    else:
        det.detect(img, THRESH)
    got = det.debug_tensor(-1)
    want = ref.letterbox(img, det.net_w, det.net_h)
    det.close()
    assert got.tobytes() == want.tobytes()


def _run_layers(pkg, tmp_path, cfg, B, seed, size=None):
    thresh = THRESH_OF[cfg]
    if size is not None:
        txt = open(cfg).read()
        net0 = ref.parse_cfg(cfg)
        txt = txt.replace("width=%d" % net0["w"], "width=%d" % size[0]).replace("height=%d" % net0["h"], "height=%d" % size[1])
        cfg = str(tmp_path / ("resized_" + os.path.basename(cfg)))
        open(cfg, "w").write(txt)
    net, params, w = _weights(tmp_path, cfg, seed)
    W, H = 160, 100   # (one image size per call)
    imgs = [_image(10 + b, W, H) for b in range(B)]
    import torch
    det = pkg.Detector(cfg, w, max_batch=B)
    d_img = torch.from_numpy(np.stack(imgs)).cuda()
    rec = torch.zeros(B * 100 * 6, dtype=torch.float32, device="cuda")
    nrec = torch.zeros(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    det.batch_dev(d_img.data_ptr(), W, H, 3, 3 * W, B, thresh, rec.data_ptr(), 100, nrec.data_ptr())
    det.sync()
    x = np.stack([ref.letterbox(im, net["w"], net["h"]) for im in imgs])
    return dict(det=det, net=net, params=params, x=x, W=W, H=H, B=B, thresh=thresh, rec=rec.cpu().numpy().reshape(B, 100, 6),
                nrec=nrec.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,size", [(YOLO3, None), (YOLO3, (64, 96)), (REGION, None), (REGION, (96, 96))])
def test_every_layer_within_calibrated_bound(pkg, tmp_path, cfg, size):
    r = _run_layers(pkg, tmp_path, cfg, 2, 7, size)
    f64 = ref.forward(r["net"], r["params"], r["x"], np.float64)
    f32 = ref.forward(r["net"], r["params"], r["x"], np.float32)
    for b in range(r["B"]):
        for li in range(len(r["net"]["layers"])):
            g = r["det"].debug_tensor(li, b)
            ok, err, bound = _bound_ok(g, f32[li][b], f64[li][b])
            assert ok, "layer %d image %d: |gpu - f64| %.3g > bound %.3g" % (li, b, err, bound)
    r["det"].close()


@pytest.mark.gpu
def test_darknet53_yolo_outputs_within_bound(pkg, tmp_path):
    r = _run_layers(pkg, tmp_path, D53, 2, 11)
    f64 = ref.forward(r["net"], r["params"], r["x"], np.float64)
    f32 = ref.forward(r["net"], r["params"], r["x"], np.float32)
    heads = [i for i, L in enumerate(r["net"]["layers"]) if L["type"] == ref.YOLO]
    assert len(heads) == 3
    for b in range(2):
        for li in heads:
            ok, err, bound = _bound_ok(r["det"].debug_tensor(li, b), f32[li][b], f64[li][b])
            assert ok, "layer %d image %d: %.3g > %.3g" % (li, b, err, bound)
    r["det"].close()


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [YOLO3, REGION])
def test_decode_nms_exact_from_device_tensors(pkg, tmp_path, cfg):
    r = _run_layers(pkg, tmp_path, cfg, 3, 21)
    total = 0
    for b in range(r["B"]):
        outs = [r["det"].debug_tensor(li, b) for li in range(len(r["net"]["layers"]))]
        want = ref.detect_from_outputs(r["net"], outs, r["W"], r["H"], r["thresh"], 100)
        n = int(r["nrec"][b])
        assert n == len(want)
        assert r["rec"][b, :n].tobytes() == want.tobytes()
        total += n
    assert total > 0, "no detection passed the threshold: the seeded case shows nothing"
    r["det"].close()


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [YOLO3, REGION])
def test_batch_dev_equals_detect(pkg, tmp_path, cfg):
    import torch
    net, params, w = _weights(tmp_path, cfg, 31)
    B, W, H = 4, 150, 90
    imgs = [_image(40 + b, W, H) for b in range(B)]
    det = pkg.Detector(cfg, w, max_batch=B)
    single = [det.detect(im, THRESH_OF[cfg], result_sz=6 * 50) for im in imgs]
    d_img = torch.from_numpy(np.stack(imgs)).cuda()
    rec = torch.zeros(B * 50 * 6, dtype=torch.float32, device="cuda")
    nrec = torch.zeros(B, dtype=torch.int32, device="cuda")
    bx = torch.full((B, 64, 4), -7, dtype=torch.int32, device="cuda")
    bn = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    det.batch_dev(d_img.data_ptr(), W, H, 3, 3 * W, B, THRESH_OF[cfg], rec.data_ptr(), 50, nrec.data_ptr(),
                  boxes=pkg.boxes_dev(bx.data_ptr(), bn.data_ptr(), 64))
    det.sync()
    rec, nrec, bx, bn = rec.cpu().numpy().reshape(B, 50, 6), nrec.cpu().numpy(), bx.cpu().numpy(), bn.cpu().numpy()
    assert sum(len(s) for s in single) > 0
    for b in range(B):
        assert nrec[b] == len(single[b])
        assert rec[b, :nrec[b]].tobytes() == single[b].tobytes()
        assert bn[b] == min(nrec[b], 64)
        assert bx[b, :bn[b]].tobytes() == ref.tracker_boxes(single[b]).tobytes()
    det.close()


@pytest.mark.gpu
def test_detector_fed_tracking_without_host_sync(pkg, tmp_path):
    import torch
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    n = 6
    L, R, _ = synth.render_sequence(n)
    L, R = L.numpy(), R.numpy()
    H, W = L.shape[1:]
    cL = np.stack([np.stack([x, np.clip(x.astype(np.int32) + 9, 0, 255).astype(np.uint8), x], axis=2) for x in L])
    cR = np.stack([np.stack([x, np.clip(x.astype(np.int32) + 9, 0, 255).astype(np.uint8), x], axis=2) for x in R])
    net, params, w = _weights(tmp_path, YOLO3, 5, obj_bias=2.5, cls_bias=2.5)
    det = pkg.Detector(YOLO3, w, max_batch=n)
    cam = pkg.Camera(**pkg.KITTI_00_02)
    rec_sz = pkg.TRACK_DTYPE.itemsize
    dL, dR = torch.from_numpy(cL).cuda(), torch.from_numpy(cR).cuda()
    drec = torch.zeros(n * 64 * 6, dtype=torch.float32, device="cuda")
    dn = torch.zeros(n, dtype=torch.int32, device="cuda")
    bx = torch.zeros((n, 64, 4), dtype=torch.int32, device="cuda")
    bn = torch.zeros(n, dtype=torch.int32, device="cuda")
    out = torch.zeros(n * rec_sz, dtype=torch.uint8, device="cuda")
    ctx = pkg.Svo(W, H, max_batch=n)
    ctx.track_reset(cam)
    torch.cuda.synchronize()
    # the detector on the left images, then the tracker with its boxes: no synchronisation in between
    det.batch_dev(dL.data_ptr(), W, H, 3, 3 * W, n, 0.8, drec.data_ptr(), 64, dn.data_ptr(),
                  boxes=pkg.boxes_dev(bx.data_ptr(), bn.data_ptr(), 64), consumer=ctx)
    ctx.track_batch_bgr_dev(dL.data_ptr(), dR.data_ptr(), 3 * W, n, out.data_ptr(), boxes=pkg.boxes_dev(bx.data_ptr(), bn.data_ptr(), 64))
    ctx.sync()
    got = out.cpu().numpy().tobytes()
    hb, hn = bx.cpu().numpy(), bn.cpu().numpy()
    assert hn.sum() > 0, "the detector found nothing: the case shows nothing"
    # the same boxes as host arrays through the host-fed entry
    ctx.track_reset(cam)
    res = np.zeros(n, pkg.TRACK_DTYPE)
    ctx.track_batch_bgr_host(np.ascontiguousarray(cL).ctypes.data, np.ascontiguousarray(cR).ctypes.data, 3 * W, n, res,
                             boxes=pkg.boxes_host(hb, hn))
    ctx.sync()
    assert res.tobytes() == got
    # and without boxes the records differ: the gating fired
    ctx.track_reset(cam)
    res0 = np.zeros(n, pkg.TRACK_DTYPE)
    ctx.track_batch_bgr_host(np.ascontiguousarray(cL).ctypes.data, np.ascontiguousarray(cR).ctypes.data, 3 * W, n, res0)
    ctx.sync()
    assert res0.tobytes() != got
    ctx.close()
    det.close()


@pytest.mark.gpu
def test_argument_checks(pkg, tmp_path):
    import torch
    net, params, w = _weights(tmp_path, YOLO3, 2)
    det = pkg.Detector(YOLO3, w, max_batch=2)
    lib = det.lib
    img = _image(1, 50, 40)
    p = img.ctypes.data_as(C.c_void_p)
    res = np.zeros(60, np.float32)
    rp = res.ctypes.data_as(C.c_void_p)
    n = C.c_int(0)
    assert lib.svo_det_detect(det.h, p, 50, 40, 2, 150, THRESH, rp, 60, C.byref(n)) == -1          # C != 1, 3
    assert lib.svo_det_detect(det.h, p, 50, 40, 4, 200, THRESH, rp, 60, C.byref(n)) == -1
    assert lib.svo_det_detect(det.h, p, 50, 40, 3, 149, THRESH, rp, 60, C.byref(n)) == -1          # stride < W * C
    assert lib.svo_det_detect(None, p, 50, 40, 3, 150, THRESH, rp, 60, C.byref(n)) == -1            # NULL det
    assert lib.svo_det_detect(det.h, p, 50, 40, 3, 150, THRESH, rp, -1, C.byref(n)) == -1           # negative result_sz
    d = torch.zeros(3 * 40 * 150, dtype=torch.uint8, device="cuda")
    r = torch.zeros(600, dtype=torch.float32, device="cuda")
    dn = torch.zeros(3, dtype=torch.int32, device="cuda")
    assert lib.svo_det_batch_dev(det.h, C.c_void_p(d.data_ptr()), 50, 40, 3, 150, 3, THRESH, C.c_void_p(r.data_ptr()), 10,
                                 C.c_void_p(dn.data_ptr()), None, None) == -5                      # B > max_batch
    assert lib.svo_det_batch_dev(None, C.c_void_p(d.data_ptr()), 50, 40, 3, 150, 1, THRESH, C.c_void_p(r.data_ptr()), 10,
                                 C.c_void_p(dn.data_ptr()), None, None) == -1
    assert lib.svo_det_debug_tensor(det.h, 99, 0, rp) == -1
    # a small result_sz truncates like YoloDetect: result_idx * 6 + 5 < result_sz
    full = det.detect(img, 0.3, result_sz=6000)
    assert len(full) >= 2, "the seeded case must give two records for the truncation check"
    part = det.detect(img, 0.3, result_sz=11)
    assert part.tobytes() == full[:1].tobytes()
    assert lib.svo_det_destroy(None) == -1
    det.close()
