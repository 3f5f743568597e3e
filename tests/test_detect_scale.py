"""Decode, NMS and the record loop of the device detector (k_det_decode) past its 1024-candidate chunk, byte for byte.

Probe heads (detect_cases.py): one 1 x 1 linear convolution whose weight rows hold one power of two each, then [yolo] or
[region], on an image of the network's size - every logit is one exact product plus a bias, the same float on darknet, numpy
and the MFMA path, so no score flutters round a threshold.  Every case asserts its precondition (T, total, m, ...) from the
restatement on the DEVICE's tensors before it compares: conditions, not measurements.
 - every case: records, counts and box arrays equal the restatement's on the device's own tensors;
 - when oracle/_ref/libref_darknet.so is there: records also equal the reference's YoloDetectFromImage end to end
   (detect_cases.compare_with_darknet: byte for byte on a libc whose qsort is probed stable, which the order of darknet's
   zero-score detections rests on; the tie-free cases assert that no two non-zero scores of a class are equal).  Each case
   prints which darknet comparison ran, or that the library is absent."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import darknet_ref as ref  # noqa: E402
import detect_cases as dc  # noqa: E402
import svo_loader  # noqa: E402
from oracle import binding as ob  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
D53 = os.path.join(GOLD, "darknet53_coco.cfg")
FILL = -7
SMALL_ANCHORS = ((3, 4), (5, 4), (4, 6))


@pytest.fixture(scope="module")
def pkg():
    return svo_loader.load()


def _run(pkg, cfg, wts, imgs, thresh, max_records, box_stride=64):
    """One svo_det_batch_dev call -> records (B x max_records x 6), counts, box arrays, and every image's layer tensors."""
    import torch
    B = len(imgs)
    H, W = imgs[0].shape[:2]
    det = pkg.Detector(cfg, wts, max_batch=B)
    d_img = torch.from_numpy(np.stack(imgs)).cuda()
    rec = torch.full((B * max(max_records, 1) * 6,), float(FILL), dtype=torch.float32, device="cuda")
    nrec = torch.full((B,), FILL, dtype=torch.int32, device="cuda")
    bx = torch.full((B, box_stride, 4), FILL, dtype=torch.int32, device="cuda")
    bn = torch.full((B,), FILL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    det.batch_dev(d_img.data_ptr(), W, H, 3, 3 * W, B, thresh, rec.data_ptr(), max_records, nrec.data_ptr(),
                  boxes=pkg.boxes_dev(bx.data_ptr(), bn.data_ptr(), box_stride))
    det.sync()
    # (a deep network: only the output layers' tensors, which are all the decode reads)
    wanted = [len(det.layers) < 20 or int(L["type"]) in (ref.YOLO, ref.REGION) for L in det.layers]
    outs = [[det.debug_tensor(li, b) if wanted[li] else None for li in range(len(det.layers))] for b in range(B)]
    x = [det.debug_tensor(-1, b) for b in range(B)]
    det.close()
    return dict(rec=rec.cpu().numpy().reshape(B, max(max_records, 1), 6), nrec=nrec.cpu().numpy(), bx=bx.cpu().numpy(),
                bn=bn.cpu().numpy(), outs=outs, x=x, W=W, H=H)


def _compare(net, r, b, thresh, max_records, box_stride=64, stats=None):
    """Image b of a run against the restatement on the device's own tensors.  -> (stats, expected records)"""
    st = stats or dc.decode_stats(net, r["outs"][b], r["W"], r["H"], thresh)
    want = dc.records_from(st, r["W"], r["H"], thresh, max_records)
    n = int(r["nrec"][b])
    assert n == len(want), "image %d: %d records, restatement %d" % (b, n, len(want))
    assert r["rec"][b, :n].tobytes() == want.tobytes(), "image %d: records differ from the restatement" % b
    if max_records > 0:
        assert (r["rec"][b, n:] == FILL).all(), "image %d: a record written past the count" % b
    cap = min(64, box_stride)
    assert r["bn"][b] == min(n, cap)
    assert r["bx"][b, :r["bn"][b]].tobytes() == ref.tracker_boxes(want, cap).tobytes()
    assert (r["bx"][b, r["bn"][b]:] == FILL).all(), "image %d: a box written past the count" % b
    return st, want


def _probe(tmp_path, name, w, h, kind="yolo", classes=2, anchors=SMALL_ANCHORS, softmax=0, seed=1, **kw):
    params = dc.probe_params(len(anchors), classes, seed=seed, **kw)
    return dc.write_case(tmp_path, name, dc.probe_cfg(w, h, kind, classes, anchors, softmax), params=params)


def _darknet_records(cfg, wts, img, thresh, result_sz):
    dn = ob.RefDarknet(cfg, wts)
    try:
        return dn.detect(ref.planar(img), thresh, result_sz)
    finally:
        dn.close()


def _darknet_leg(cfg, wts, img, thresh, cap, got, ties):
    """The end-to-end comparison with the reference's YoloDetectFromImage; -> the line that says what ran."""
    if ob.ref_darknet_lib() is None:
        return "darknet: NOT compared (oracle/_ref/libref_darknet.so is absent)"
    return dc.compare_with_darknet(got, _darknet_records(cfg, wts, img, thresh, 6 * cap), ties)


def _identity_input(r, imgs):
    for b, im in enumerate(imgs):      # the image has the network's size: the input tensor is byte / 255. bit for bit
        assert r["x"][b].tobytes() == ref.planar(im).tobytes() == ref.letterbox(im, im.shape[1], im.shape[0]).tobytes()


# name: (w, h, kind, classes, anchors, image options, precondition on the stats).  NOT_TIE_FREE: with 80 classes some two of the
# ~1000 scores of a class round to the same float; the other cases assert that they have no such pair.
CASES = {
    "T_1024": (48, 32, "yolo", 2, ((3, 4),), dict(n_hi=1024), lambda s: s["T"] == 1024),
    "T_1025": (48, 32, "yolo", 2, ((3, 4),), dict(n_hi=1025), lambda s: s["T"] == 1025),
    "T_over_2048_m_over_1024": (44, 32, "yolo", 2, SMALL_ANCHORS, dict(obj_share=0.6), lambda s: s["T"] > 2048 and s["m"] > 1024),
    "region_swapped_tail": (32, 24, "region", 2, ((1, 1.5), (2, 1), (1.5, 2.5)), dict(obj_share=0.4),
                            lambda s: s["T"] > 2048 and all((s["objs"][c:c + 1024] == 0).mean() > 0.3 for c in range(0, s["T"], 1024))),
    "80_classes": (32, 24, "yolo", 80, ((3, 4), (5, 4)), dict(obj_share=0.8), lambda s: s["T"] > 1024 and s["probs"].shape[1] == 80),
    "one_class": (44, 32, "yolo", 1, SMALL_ANCHORS, dict(obj_share=0.6, seed=20), lambda s: s["T"] > 2048 and s["m"] > 1024),
    # large anchors: few survivors, each suppressing neighbours at ranks past 1024
    "large_anchors": (44, 32, "yolo", 1, ((150, 120), (200, 160), (120, 200)), dict(obj_share=0.6, seed=20), lambda s: s["m"] > 1024),
}


NOT_TIE_FREE = {"80_classes"}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_decode_past_one_chunk(pkg, tmp_path, name):
    w, h, kind, classes, anchors, imopt, pre = CASES[name]
    cfg, wts, net, params = _probe(tmp_path, name, w, h, kind, classes, anchors)
    imopt = dict(imopt)
    img = dc.probe_image(imopt.pop("seed", 11), w, h, **imopt)
    r = _run(pkg, cfg, wts, [img], 0.5, 4000)
    _identity_input(r, [img])
    st = dc.decode_stats(net, r["outs"][0], w, h, 0.5)
    assert pre(st), "%s: precondition not met (T %d, total %d, m %d): the case shows nothing" % (name, st["T"], st["total"], st["m"])
    st, want = _compare(net, r, 0, 0.5, 4000, stats=st)
    print("%s: T %d, total %d, largest m %d, records %d, ties %s" % (name, st["T"], st["total"], st["m"], len(want), st["ties"]))
    assert len(want) > 0
    if name == "large_anchors":       # fewer survivors than m - 1024: a candidate ranked past 1024 was suppressed
        assert len(want) < st["m"] - 1024
    if name not in NOT_TIE_FREE:
        assert not st["ties"], "two equal non-zero scores in one class: qsort's order would decide"
    print(_darknet_leg(cfg, wts, img, 0.5, 4000, r["rec"][0, :len(want)], st["ties"]))


@pytest.mark.gpu
def test_two_output_layers_past_one_chunk_each(pkg, tmp_path):
    """conv 0 copies the image (weights 1: exact), head A + [yolo] on it, a route back to layer 0, head B + [yolo]."""
    w, h = 44, 32
    txt = (dc._net(w, h) + dc._conv(3, act="linear") + dc._conv(21, act="linear") +
           dc._yolo(2, 6, "0,1,2", "3,4,5,4,4,6,6,5,5,7,7,6") + "[route]\nlayers=0\n\n" + dc._conv(21, act="linear") +
           dc._yolo(2, 6, "3,4,5", "3,4,5,4,4,6,6,5,5,7,7,6"))
    eye = np.concatenate([np.zeros(3, np.float32), np.eye(3, dtype=np.float32).reshape(-1)])
    params = np.concatenate([eye, dc.probe_params(3, 2, seed=1), dc.probe_params(3, 2, seed=2, obj_bias=-3.5)])
    cfg, wts, net, params = dc.write_case(tmp_path, "two_heads", txt, params=params)
    img = dc.probe_image(12, w, h, obj_share=0.6)
    r = _run(pkg, cfg, wts, [img], 0.5, 4000)
    _identity_input(r, [img])
    assert r["outs"][0][0].tobytes() == r["x"][0].tobytes()
    per_layer = [int((r["outs"][0][li].reshape(3, 7, h, w)[:, 4] > np.float32(0.5)).sum()) for li in (2, 5)]
    assert min(per_layer) > 1024, per_layer
    st, want = _compare(net, r, 0, 0.5, 4000)
    print("two heads: per layer %s, T %d, largest m %d, records %d, ties %s" % (per_layer, st["T"], st["m"], len(want), st["ties"]))
    assert st["T"] == sum(per_layer) and len(want) > 0
    assert not st["ties"]
    print(_darknet_leg(cfg, wts, img, 0.5, 4000, r["rec"][0, :len(want)], st["ties"]))


@pytest.mark.gpu
def test_blocks_of_constant_colour_tie_in_the_documented_order(pkg, tmp_path):
    """Many cells tie exactly; compared with the restatement only (darknet's qsort leaves the order of ties open)."""
    w, h = 48, 32
    cfg, wts, net, params = _probe(tmp_path, "ties", w, h, "yolo", 2, SMALL_ANCHORS)
    small = dc.probe_image(13, w // 4, h // 4, obj_share=0.8)
    img = np.ascontiguousarray(small.repeat(4, axis=0).repeat(4, axis=1))
    r = _run(pkg, cfg, wts, [img], 0.5, 4000)
    st, want = _compare(net, r, 0, 0.5, 4000)
    print("ties: T %d, largest m %d, records %d" % (st["T"], st["m"], len(want)))
    assert st["ties"] and st["T"] > 2048 and st["m"] > 1024 and len(want) > 0
    nz = st["probs"][:, 0][st["probs"][:, 0] != 0]
    assert len(np.unique(nz)) * 8 <= len(nz), "the blocks must make most scores tie"


@pytest.mark.gpu
def test_batch_of_very_different_counts(pkg, tmp_path):
    w, h = 44, 32
    cfg, wts, net, params = _probe(tmp_path, "batch", w, h, "yolo", 2, SMALL_ANCHORS)
    imgs = [dc.probe_image(14, w, h, n_hi=0), dc.probe_image(15, w, h, n_hi=34), dc.probe_image(16, w, h, obj_share=0.6)]
    r = _run(pkg, cfg, wts, imgs, 0.5, 4000)
    _identity_input(r, imgs)
    T = []
    for b in range(3):
        st, want = _compare(net, r, b, 0.5, 4000)
        T.append(st["T"])
        print("batch image %d: T %d, largest m %d, records %d" % (b, st["T"], st["m"], len(want)))
    assert T[0] <= 30 and 50 <= T[1] <= 150 and T[2] > 2048, T      # about 0, about 100, past two chunks
    # the same three in another order: the per-image scratch offsets (b * tmax) do not leak between images
    r2 = _run(pkg, cfg, wts, imgs[::-1], 0.5, 4000)
    for b in range(3):
        n = int(r["nrec"][b])
        assert r2["nrec"][2 - b] == n and r2["rec"][2 - b, :n].tobytes() == r["rec"][b, :n].tobytes()


@pytest.mark.gpu
def test_max_records_and_box_strides(pkg, tmp_path):
    w, h = 44, 32
    cfg, wts, net, params = _probe(tmp_path, "cut", w, h, "yolo", 1, SMALL_ANCHORS)
    img = dc.probe_image(21, w, h, obj_share=0.6)
    r = _run(pkg, cfg, wts, [img], 0.5, 4000)
    st, full = _compare(net, r, 0, 0.5, 4000)
    order, probs = ref.nms_sort_fast(st["boxes"], st["objs"], st["probs"])
    passing = np.array([probs[d].max() > np.float32(0.5) for d in order])
    first = int(passing[:1024].sum())                # records found by the first chunk of the record loop
    assert st["T"] > 2048 and len(full) == passing.sum() and 0 < first < len(full) - 8, (st["T"], first, len(full))
    print("max_records: T %d, records %d, %d of them from the first chunk" % (st["T"], len(full), first))
    assert not st["ties"]
    legs = set()
    for cap in (0, 1, first, first + 5, len(full) - 1, len(full), len(full) + 1):
        rc = _run(pkg, cfg, wts, [img], 0.5, cap)
        _compare(net, rc, 0, 0.5, cap)
        assert rc["nrec"][0] == min(cap, len(full))
        if cap >= len(full) or dc._QSORT_STABLE is not False:     # (a cut set is comparable only in darknet's own order)
            legs.add(_darknet_leg(cfg, wts, img, 0.5, cap, rc["rec"][0, :rc["nrec"][0]], st["ties"]))   # result_idx * 6 + 5 < result_sz
    print("max_records:", sorted(legs))
    for stride in (7, 200, 1):
        rs = _run(pkg, cfg, wts, [img, img], 0.5, 300, box_stride=stride)
        for b in range(2):
            _compare(net, rs, b, 0.5, 300, box_stride=stride)
        assert rs["bn"][0] == min(64, stride)


@pytest.mark.gpu
@pytest.mark.parametrize("imw,imh", [(110, 40), (40, 110)])
def test_box_correction_wide_and_tall(pkg, tmp_path, imw, imh):
    """An ordinary letterbox (a wide and a tall image on a square network): both branches of correct_yolo_boxes."""
    cfg, wts, net, params = _probe(tmp_path, "sq", 48, 48, "yolo", 2, SMALL_ANCHORS)
    img = dc.probe_image(18, imw, imh, obj_share=0.7)
    r = _run(pkg, cfg, wts, [img], 0.5, 4000)
    assert r["x"][0].tobytes() == ref.letterbox(img, 48, 48).tobytes()
    st, want = _compare(net, r, 0, 0.5, 4000)
    print("letterboxed %d x %d: T %d, largest m %d, records %d" % (imw, imh, st["T"], st["m"], len(want)))
    assert st["T"] > 1024 and len(want) > 0


@pytest.mark.gpu
def test_darknet53_records_exact_from_device_tensors(pkg, tmp_path):
    """darknet53 at 416 (10,647 candidates, 80 classes), seeded weights, B = 2: records byte for byte against the restatement on
    the device's tensors.  (darknet's own forward of the same cfg, weights and size is compared with the restatement on the CPU,
    test_detect_ref.py::test_darknet53_at_416_against_darknet; the device's convolutions differ from darknet's in the last bits,
    so scores flutter round the threshold and the device's records are not comparable with darknet's end to end.)"""
    net = ref.parse_cfg(D53)
    # (head_scale: the seeded residual stack reaches activations of 5e6; the heads' kernels are scaled so that the w / h logits
    # stay within a few units - an overflowing exp would put inf into darknet's float-to-int conversion, which C leaves undefined)
    params = ref.seeded_params(net, 11, head_scale=1e-6)
    wts = str(tmp_path / "d53.weights")
    ref.write_weights(wts, params)
    imgs = [dc.sweep_image(30 + b, 160, 100) for b in range(2)]
    r = _run(pkg, D53, wts, imgs, 0.5, 1000)
    for b in range(2):
        st = dc.decode_stats(net, r["outs"][b], r["W"], r["H"], 0.5)
        assert np.isfinite(st["boxes"]).all(), "a box overflowed: the case would compare undefined conversions"
        st, want = _compare(net, r, b, 0.5, 1000, stats=st)
        print("darknet53 image %d: T %d, total %d, largest m %d, records %d" % (b, st["T"], st["total"], st["m"], len(want)))
        assert st["T"] > 1024 and len(want) > 0
