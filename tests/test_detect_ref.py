"""The numpy restatement of the detector (darknet_ref.py) against the reference's own darknet, compiled for the CPU by
oracle/Makefile.ref into oracle/_ref/libref_darknet.so: layer shapes and parameter counts, letterbox_image bit for bit, every
layer of the generated sweep networks (detect_cases.py) applied to darknet's own previous layer, and YoloDetectFromImage's
records byte for byte on the probe heads.  No GPU.

Ties: darknet sorts with libc qsort, whose order for equal scores is unspecified.  The probe-head comparisons with darknet
assert that no two non-zero scores of a class are equal; ties are tested against the restatement's documented stable order
only.  That assertion does not cover the zeros: do_nms_sort sorts every detection of a class, those with score 0 included, they
all compare equal, and their order after the last class's sort is the order of the records.  So every byte-for-byte
comparison of records with darknet on two or more classes rests on this libc's qsort being stable; detect_cases.
compare_with_darknet probes that once and otherwise falls back to multisets (and says which it did)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import darknet_ref as ref  # noqa: E402
import detect_cases as dc  # noqa: E402
import svo_loader  # noqa: E402
from oracle import binding as ob  # noqa: E402

needs_darknet = pytest.mark.skipif(ob.ref_darknet_lib() is None,
                                   reason="oracle/_ref not built (needs /root/reference at build time)")

GOLD = os.path.join(os.path.dirname(__file__), "golden")
SMALL = ["tiny_yolo3_small.cfg", "tiny_region_small.cfg"]
SWEEP = dc.sweep_cfgs()


@pytest.fixture(scope="module")
def pkg():
    return svo_loader.load()


def _shapes(layers):
    """(darknet's route layer does not record an input shape: only its output is compared)"""
    return [(int(L["type"]),) + (() if int(L["type"]) == ref.ROUTE else (int(L["in_w"]), int(L["in_h"]), int(L["in_c"]))) +
            (int(L["out_w"]), int(L["out_h"]), int(L["out_c"]), int(L["n_params"])) for L in layers]


@needs_darknet
@pytest.mark.parametrize("name", sorted(SWEEP) + SMALL)
def test_shapes_and_parameter_counts_agree(pkg, tmp_path, name):
    if name in SWEEP:
        cfg, w, net, params = dc.write_case(tmp_path, name, SWEEP[name])
    else:
        cfg = os.path.join(GOLD, name)
        net = ref.parse_cfg(cfg)
        params = ref.seeded_params(net, 1)
        w = str(tmp_path / "w.weights")
        ref.write_weights(w, params)
    dev, n_dev = pkg.Detector.describe(cfg, w)
    dn = ob.RefDarknet(cfg, w)
    try:
        assert (dn.w, dn.h, dn.c) == (net["w"], net["h"], net["c"])
        assert _shapes(dn.layers) == _shapes(net["layers"]) == _shapes(dev)
        assert sum(L["n_params"] for L in dn.layers) == ref.n_params(net) == n_dev == len(params)
    finally:
        dn.close()


# (image W x H, network w x h): downscale and upscale, wide and tall, image = network, one pixel wide / high, odd ratios.
# NOT covered, because unreachable: (int)sx reaching W - 1 before the last column.  sx = c * fl((W - 1) / (new_w - 1)) for
# c <= new_w - 2 stays below W - 1 unless float rounding lifts it by (W - 1) / (new_w - 1), which needs sizes near 2^24; and
# there darknet's get_pixel asserts ix + 1 < W and aborts.  The clamp the restatement and the device apply at (int)sx + 1 is
# therefore not checked against darknet; every case asserts that it does not reach it.
LETTERBOX = [(160, 100, 96, 64), (1241, 376, 416, 416), (40, 30, 96, 64), (30, 40, 64, 96), (100, 160, 96, 64), (96, 64, 96, 64),
             (64, 64, 64, 64), (77, 131, 96, 64), (1, 8, 16, 16), (8, 1, 16, 16), (1, 1, 8, 8), (2, 2, 33, 33), (3, 3, 64, 48),
             (7, 5, 50, 36), (11, 11, 111, 111), (50, 50, 99, 99), (37, 23, 416, 256), (640, 480, 20, 16), (101, 57, 35, 19)]


@needs_darknet
@pytest.mark.parametrize("W,H,nw,nh", LETTERBOX)
def test_letterbox_equals_darknet_bit_for_bit(W, H, nw, nh):
    """(Left out: images so elongated that new_w or new_h becomes 1 - darknet's scale is then x / 0 and 0 * inf = NaN indexes
    outside the image; the device refuses them.)"""
    new_w, new_h = ref.letterbox_geom(W, H, nw, nh)
    assert new_w >= 2 and new_h >= 2
    # darknet's get_pixel asserts ix + 1 < W: the case must not reach it (the restatement clamps there instead)
    sx = (np.arange(new_w - 1).astype(np.float32) * (np.float32(W - 1) / np.float32(new_w - 1))).astype(np.int64)
    sy = (np.arange(new_h - 1).astype(np.float32) * (np.float32(H - 1) / np.float32(new_h - 1))).astype(np.int64)
    assert W == 1 or sx.max(initial=0) + 1 < W
    assert H == 1 or sy.max(initial=0) + 1 < H
    img = dc.sweep_image(W * 1000 + H, W, H)
    pl = ref.planar(img)
    want = ob.ref_dn_letterbox(pl, nw, nh)
    assert ref.letterbox_planar(pl, nw, nh).tobytes() == want.tobytes()
    assert ref.letterbox(img, nw, nh).tobytes() == want.tobytes()
    if (W, H) == (nw, nh):
        assert want.tobytes() == pl.tobytes()       # image = network: the identity
    # a float image that is not byte / 255.
    fl = np.random.default_rng(W + H).random((3, H, W)).astype(np.float32)
    assert ref.letterbox_planar(fl, nw, nh).tobytes() == ob.ref_dn_letterbox(fl, nw, nh).tobytes()


@needs_darknet
@pytest.mark.parametrize("name", sorted(SWEEP) + SMALL)
def test_every_layer_against_darknet(tmp_path, name, record_property):
    """The restatement's layer l in float64 on darknet's layer l - 1 output against darknet's layer l: bit-identical for
    maxpool / route / upsample / shortcut, the derived bounds of detect_cases.py for the rest."""
    if name in SWEEP:
        cfg, w, net, params = dc.write_case(tmp_path, name, SWEEP[name], seed=3)
    else:
        cfg = os.path.join(GOLD, name)
        net = ref.parse_cfg(cfg)
        params = ref.seeded_params(net, 3)
        w = str(tmp_path / "w.weights")
        ref.write_weights(w, params)
    dn = ob.RefDarknet(cfg, w)
    try:
        worst = 0.0
        for seed in (1, 2):
            x = ref.letterbox(dc.sweep_image(seed, 50, 37), net["w"], net["h"])
            outs = [o[None] for o in dn.forward(x)]
            fails, conv_ratio, other_ratio = dc.network_check(net, params, x[None], outs)
            assert not fails, "\n".join(fails)
            worst = max(worst, conv_ratio)
            print("%s image %d: darknet's CPU gemm: largest convolution error / bound %.3f, other bounded layers %.3f" %
                  (name, seed, conv_ratio, other_ratio))
        record_property("conv_error_over_bound", worst)
        assert worst > 0, "no convolution erred at all: the comparison shows nothing"
    finally:
        dn.close()


# ---- records against YoloDetectFromImage ----
PROBES = {
    # name: (w, h, kind, classes, anchors, softmax, thresh, image seed, obj_share)
    "yolo_small": (16, 12, "yolo", 2, ((10, 14), (23, 27), (37, 58)), 0, 0.5, 1, 0.5),
    "yolo_1100": (44, 32, "yolo", 2, ((3, 4), (5, 4), (4, 6)), 0, 0.5, 2, 0.6),
    "yolo_80_classes": (12, 10, "yolo", 80, ((3, 4), (5, 4)), 0, 0.5, 3, 0.6),
    "yolo_one_class": (20, 16, "yolo", 1, ((3, 4), (5, 4), (4, 6)), 0, 0.5, 4, 0.5),
    "region_swapped_tail": (24, 20, "region", 2, ((1, 1.5), (2, 1), (1.5, 2.5)), 0, 0.5, 5, 0.4),
    "region_softmax": (16, 12, "region", 3, ((1, 1.5), (2, 1)), 1, 0.3, 6, 0.5),
}


def _probe(tmp_path, name):
    w, h, kind, classes, anchors, softmax, thresh, seed, share = PROBES[name]
    params = dc.probe_params(len(anchors), classes, seed=seed)
    cfg, wts, net, params = dc.write_case(tmp_path, name, dc.probe_cfg(w, h, kind, classes, anchors, softmax), params=params)
    return cfg, wts, net, params, dc.probe_image(seed, w, h, share), thresh


@needs_darknet
@pytest.mark.parametrize("name", sorted(PROBES))
def test_records_equal_yolo_detect_from_image(tmp_path, name):
    cfg, wts, net, params, img, thresh = _probe(tmp_path, name)
    H, W = img.shape[:2]
    pl = ref.planar(img)
    x = ref.letterbox(img, net["w"], net["h"])
    assert x.tobytes() == pl.tobytes()               # the image has the network's size: the letterbox is the identity
    dn = ob.RefDarknet(cfg, wts)
    try:
        outs_dn = dn.forward(x)
        outs = [o[0] for o in ref.forward(net, params, x[None], np.float32)]
        # one exact product plus a bias per logit: the head tensors are the same floats, so no score flutters round the threshold
        assert outs[0].tobytes() == outs_dn[0].tobytes()
        assert outs[1].tobytes() == outs_dn[1].tobytes() or net["layers"][1].get("softmax"), "the output layer differs from darknet's"
        st = dc.decode_stats(net, outs_dn, W, H, thresh)
        assert not st["ties"], "two equal non-zero scores in one class: qsort's order would decide"
        want = dn.detect(pl, thresh, 6 * 4000)
        got = dc.records_from(st, W, H, thresh, 4000)
        print("%s: T %d, total %d, largest m %d, records %d" % (name, st["T"], st["total"], st["m"], len(want)))
        assert len(want) > 0, "nothing passed: the case shows nothing"
        if name == "yolo_1100":
            assert st["T"] > 1024 and st["m"] > 1024
        if name == "region_swapped_tail":
            assert st["T"] > 1024 and st["T"] - st["total"] > 256
        print(dc.compare_with_darknet(got, want, st["ties"]))
        if not dc._QSORT_STABLE:
            print("%s: the cut result sizes are NOT compared (a cut set is comparable only in darknet's own order)" % name)
            return
        # truncation: result_idx * 6 + 5 < result_sz
        for sz in (0, 5, 6, 11, 6 * (len(want) - 1) + 5, 6 * len(want)):
            assert dn.detect(pl, thresh, sz).tobytes() == dc.records_from(st, W, H, thresh, sz // 6).tobytes()
    finally:
        dn.close()


@needs_darknet
@pytest.mark.parametrize("imw,imh", [(40, 16), (16, 40)])
def test_records_equal_darknet_through_a_letterbox(tmp_path, imw, imh):
    """Both branches of the box correction: a wide and a tall image on a square network."""
    params = dc.probe_params(3, 2, seed=7)
    cfg, wts, net, params = dc.write_case(tmp_path, "sq", dc.probe_cfg(24, 24, "yolo", 2), params=params)
    img = dc.probe_image(8, imw, imh)
    pl = ref.planar(img)
    dn = ob.RefDarknet(cfg, wts)
    try:
        outs_dn = dn.forward(ob.ref_dn_letterbox(pl, 24, 24))
        st = dc.decode_stats(net, outs_dn, imw, imh, 0.5)
        assert not st["ties"]
        want = dn.detect(pl, 0.5, 6000)
        assert len(want) > 0
        print(dc.compare_with_darknet(dc.records_from(st, imw, imh, 0.5, 1000), want, st["ties"]))
    finally:
        dn.close()


def test_this_libc_qsort_keeps_equal_elements_in_order():
    """What the byte-for-byte comparisons with darknet rest on (see the module docstring).  If this fails the comparisons fall
    back to multisets; the failure says why."""
    assert ob.ref_qsort_is_stable(), "libc qsort reorders equal elements: darknet's record order among zero scores is then open"


@needs_darknet
def test_darknet53_at_416_against_darknet(tmp_path):
    """darknet53 (tests/golden/darknet53_coco.cfg) at 416 x 416, seeded weights, one 160 x 100 image through
    YoloDetectFromImage: about 60 s of darknet's naive CPU gemm here (network_predict alone 34 s), so the full size is kept.
    The restatement's [yolo] layers on darknet's own previous tensors, and the restatement's records from darknet's [yolo]
    tensors against YoloDetectFromImage (10,647 candidates, 80 classes, equal scores included - see compare_with_darknet).
    (head_scale: the seeded residual stack reaches activations of 5e6; the heads' kernels are scaled so that the w / h logits
    stay within a few units - an overflowing exp would put inf into YoloDetect's float-to-int conversion, which C leaves
    undefined.)"""
    cfg = os.path.join(GOLD, "darknet53_coco.cfg")
    net = ref.parse_cfg(cfg)
    params = ref.seeded_params(net, 11, head_scale=1e-6)
    wts = str(tmp_path / "d53.weights")
    ref.write_weights(wts, params)
    img = dc.sweep_image(30, 160, 100)
    dn = ob.RefDarknet(cfg, wts)
    try:
        assert (dn.w, dn.h) == (416, 416) and len(dn.layers) == 107
        assert [(L["type"], L["out_w"], L["out_h"], L["out_c"], L["n_params"]) for L in dn.layers] == \
               [(L["type"], L["out_w"], L["out_h"], L["out_c"], L["n_params"]) for L in net["layers"]]
        want = dn.detect(ref.planar(img), 0.5, 6 * 1000)
        heads = [i for i, L in enumerate(net["layers"]) if L["type"] == ref.YOLO]
        # the tensors of the forward inside YoloDetectFromImage: the heads, the convolutions feeding them and their inputs
        need = set(heads) | {i - 1 for i in heads} | {i - 2 for i in heads}
        outs = dn.outputs(only=need)
        P = ref.split_params(net, params)
        for li in heads:
            for l in (li - 1, li):      # the last convolution (K = 1024 / 512 / 256) and the [yolo] layer, each on darknet's input
                ok, ratio, msg = dc.layer_check(net, P, l, outs[l - 1][None], [], outs[l][None])
                print("darknet53 layer %d: error / bound %.3f" % (l, ratio))
                assert ok, msg
        st = dc.decode_stats(net, outs, 160, 100, 0.5)
        assert np.isfinite(st["boxes"]).all()
        got = dc.records_from(st, 160, 100, 0.5, 1000)
        print("darknet53: T %d, total %d, largest m %d, records %d, ties %s" % (st["T"], st["total"], st["m"], len(got), st["ties"]))
        assert st["T"] > 1024 and st["m"] > 1024 and len(want) > 0
        print(dc.compare_with_darknet(got, want, st["ties"]))
    finally:
        dn.close()


# ---- the vectorised NMS against the scalar one, and the documented order on ties ----
@pytest.mark.parametrize("seed,n,classes,zero_share", [(1, 60, 1, 0.0), (2, 200, 3, 0.3), (3, 300, 2, 0.5), (4, 1, 2, 0.0), (5, 0, 2, 0.0)])
def test_vectorised_nms_equals_scalar(seed, n, classes, zero_share):
    rng = np.random.default_rng(seed)
    boxes = np.concatenate([rng.uniform(.2, .8, (n, 2)), rng.uniform(.05, .4, (n, 2))], axis=1).astype(np.float32)
    objs = rng.uniform(.5, 1, n).astype(np.float32)
    objs[rng.random(n) < zero_share] = 0
    probs = rng.uniform(.5, 1, (n, classes)).astype(np.float32)
    probs[rng.random((n, classes)) < .3] = 0
    probs[objs == 0] = 0
    if n > 10:       # exact ties, and degenerate boxes (0 / 0 in box_iou)
        probs[5] = probs[3]
        probs[9] = probs[3]
        boxes[7, 2:] = 0
        boxes[8, 2:] = 0
        boxes[8, :2] = boxes[7, :2]
    with np.errstate(invalid="ignore", divide="ignore"):
        o1, p1 = ref.nms_sort(boxes, objs, probs)
    o2, p2 = ref.nms_sort_fast(boxes, objs, probs)
    assert o1 == o2
    assert p1.tobytes() == p2.tobytes()


def test_ties_keep_the_order_before_the_sort():
    """The one documented departure from darknet (whose qsort leaves it open): equal scores stay in the order they had before
    the class's sort, so the earlier one suppresses the later one."""
    boxes = np.array([[.5, .5, .2, .2], [.5, .5, .2, .2], [.2, .2, .1, .1], [.8, .8, .1, .1]], np.float32)
    objs = np.array([.9, .9, .9, .9], np.float32)
    probs = np.array([[.7], [.7], [.6], [.6]], np.float32)
    for f in (ref.nms_sort, ref.nms_sort_fast):
        order, p = f(boxes, objs, probs)
        assert order == [0, 1, 2, 3]
        assert p[:, 0].tolist() == [pytest.approx(.7), 0, pytest.approx(.6), pytest.approx(.6)]
    # a second class re-sorts the order the first class left: the tie in class 1 follows class 0's ranking
    probs2 = np.array([[.6, .8], [.9, 0], [.7, .8], [0, .8]], np.float32)
    boxes2 = np.array([[.1, .1, .1, .1], [.3, .3, .1, .1], [.5, .5, .1, .1], [.7, .7, .1, .1]], np.float32)
    for f in (ref.nms_sort, ref.nms_sort_fast):
        order, _ = f(boxes2, objs, probs2)
        assert order == [2, 0, 3, 1]      # class 0 leaves 1, 2, 0, 3; class 1 ranks the .8s in that order, then the zero
