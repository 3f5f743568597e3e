"""Darknet detector, host side (no GPU): svo_det_describe's cfg parser and weights checks against the independent
restatement in darknet_ref.py, and the restatement's own hand-computed cases."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import darknet_ref as ref  # noqa: E402
import svo_loader  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
D53 = os.path.join(GOLD, "darknet53_coco.cfg")
SMALL = [os.path.join(GOLD, n) for n in ("tiny_yolo3_small.cfg", "tiny_region_small.cfg")]


@pytest.fixture(scope="module")
def pkg():
    return svo_loader.load()


def test_describe_darknet53(pkg):
    L, n = pkg.Detector.describe(D53)
    names = [pkg.DET_LAYER_TYPES[t] for t in L["type"]]
    assert len(L) == 107
    assert (names.count("convolutional"), names.count("shortcut"), names.count("route"), names.count("upsample"),
            names.count("yolo")) == (75, 23, 4, 2, 3)
    outs = [(int(l["out_w"]), int(l["out_h"]), int(l["out_c"])) for l in L if l["type"] == 5]
    assert outs == [(13, 13, 255), (26, 26, 255), (52, 52, 255)]
    # the oracle's independent count; the published yolov3.weights is 248,007,048 bytes = 20 + 4 * 62,001,757
    assert n == ref.n_params(ref.parse_cfg(D53)) == 62001757
    assert 20 + 4 * n == 248007048


@pytest.mark.parametrize("cfg", SMALL + [D53])
def test_describe_matches_oracle(pkg, cfg):
    L, n = pkg.Detector.describe(cfg)
    net = ref.parse_cfg(cfg)
    assert len(L) == len(net["layers"])
    for g, o in zip(L, net["layers"]):
        assert int(g["type"]) == o["type"]
        assert (g["in_w"], g["in_h"], g["in_c"], g["out_w"], g["out_h"], g["out_c"]) == \
               (o["in_w"], o["in_h"], o["in_c"], o["out_w"], o["out_h"], o["out_c"])
        assert int(g["n_params"]) == o["n_params"]
    assert n == ref.n_params(net)


def _cfg(tmp_path, body, name="t.cfg"):
    p = tmp_path / name
    p.write_text("[net]\nwidth=32\nheight=32\nchannels=3\n" + body)
    return str(p)


HEAD = "[convolutional]\nfilters=%d\nsize=1\nstride=1\nactivation=linear\n\n[yolo]\nmask=0\nanchors=10,10\nclasses=2\nnum=1\n" % 7


@pytest.mark.parametrize("body,needle", [
    ("[local]\nfilters=4\n" + HEAD, "[local]"),
    ("[convolutional]\nfilters=4\ngroups=2\n" + HEAD, "groups"),
    ("[convolutional]\nfilters=4\nbinary=1\n" + HEAD, "binary"),
    ("[convolutional]\nfilters=4\ndilation=2\n" + HEAD, "dilation"),
    ("[convolutional]\nfilters=4\nactivation=relu\n" + HEAD, "relu"),
    ("[convolutional]\nfilters=4\n[maxpool]\nsize=2\nstride=2\n[shortcut]\nfrom=-2\n" + HEAD, "different shapes"),
    ("[convolutional]\nfilters=4\n[upsample]\nstride=2\nscale=0.5\n" + HEAD, "scale"),
    ("[convolutional]\nfilters=45\n[region]\nclasses=4\ncoords=4\nnum=5\ntree=x.tree\n", "tree"),
])
def test_reject(pkg, tmp_path, body, needle):
    with pytest.raises(pkg.SvoError) as e:
        pkg.Detector.describe(_cfg(tmp_path, body))
    msg = str(e.value)
    assert needle in msg and "line" in msg, msg


def test_reject_names_the_line(pkg, tmp_path):
    p = _cfg(tmp_path, "[convolutional]\nfilters=4\n\n[convolutional]\nfilters=7\nxnor=1\n" + HEAD[HEAD.index("[yolo]"):])
    with pytest.raises(pkg.SvoError) as e:
        pkg.Detector.describe(p)
    assert "[convolutional] at line 8" in str(e.value), str(e.value)


@pytest.mark.parametrize("cfg", SMALL)
def test_weights_sizes_and_headers(pkg, tmp_path, cfg):
    net = ref.parse_cfg(cfg)
    params = ref.seeded_params(net, 1)
    assert len(params) == ref.n_params(net)
    # both header variants: size_t `seen` (major * 10 + minor >= 2) and int `seen`
    for major, minor, head in ((0, 2, 20), (0, 1, 16), (1, 0, 20)):
        w = tmp_path / ("w%d%d.weights" % (major, minor))
        ref.write_weights(str(w), params, major, minor)
        assert os.path.getsize(w) == head + 4 * len(params)
        _, n = pkg.Detector.describe(cfg, str(w))
        assert n == len(params)
    good = tmp_path / "w02.weights"
    data = good.read_bytes()
    for bad in (data[:-4], data + b"\0\0\0\0", data[:10]):
        (tmp_path / "bad.weights").write_bytes(bad)
        with pytest.raises(pkg.SvoError):
            pkg.Detector.describe(cfg, str(tmp_path / "bad.weights"))
    (tmp_path / "tr.weights").write_bytes(struct.pack("<iii", 0, 1001, 0) + data[12:])
    with pytest.raises(pkg.SvoError, match="transposed"):
        pkg.Detector.describe(cfg, str(tmp_path / "tr.weights"))


# ---- the oracle's own hand-computed cases ----

def test_oracle_letterbox_geometry():
    # 1241 x 376 into 416 x 416: new_w = 416, new_h = 376 * 416 / 1241 = 126 (int), embedded at dy = (416 - 126) / 2 = 145
    assert ref.letterbox_geom(1241, 376, 416, 416) == (416, 126)
    img = np.full((376, 1241, 3), 255, np.uint8)
    x = ref.letterbox(img, 416, 416)
    assert x.shape == (3, 416, 416)
    assert (x[:, :145] == np.float32(.5)).all() and (x[:, 145 + 126:] == np.float32(.5)).all()
    assert (x[:, 145:145 + 126] == np.float32(1)).all()
    # a horizontal ramp is resized linearly: the first and last columns are the source's
    ramp = np.tile(np.arange(8, dtype=np.uint8)[None, :, None] * 30, (4, 1, 3))
    y = ref.letterbox(ramp, 8, 8)
    assert y[0, 2, 0] == np.float32(0) and y[0, 2, 7] == np.float32(210 / 255.)


def test_oracle_yolo_box_correction():
    # one 1 x 1 yolo cell on a 32 x 32 network, image 64 x 32: new_w = 32, new_h = 16, dy = 8
    net = dict(w=32, h=32, layers=[dict(type=ref.YOLO, classes=1, n=1, anchors=[(np.float32(16), np.float32(8))])])
    o = np.zeros((6, 1, 1), np.float32)
    o[0] = o[1] = np.float32(.5)
    o[4] = o[5] = np.float32(.9)
    b, obj, pr = ref.network_boxes(net, [o], 64, 32, .5)
    # x = 0.5, y = (0.5 - 8/32) / (16/32) = 0.5; w = 1 * 16 / 32 * (32/32) = 0.5, h = 8/32 * (32/16) = 0.5
    assert np.array_equal(b, np.array([[.5, .5, .5, .5]], np.float32))
    assert obj[0] == np.float32(.9) and pr[0, 0] == np.float32(.9) * np.float32(.9)
    rec = ref.records(b, pr, [0], 64, 32, .5, 10)
    assert rec.tolist() == [[0, pytest.approx(.81), 16, 8, 32, 16]]


def test_oracle_nms_order_and_swap():
    boxes = np.array([[.5, .5, .2, .2], [.5, .5, .2, .2], [.1, .1, .1, .1], [.51, .5, .2, .2]], np.float32)
    objs = np.array([.9, 0, .8, .7], np.float32)
    probs = np.array([[.6], [0], [.8], [.7]], np.float32)
    order, p = ref.nms_sort(boxes, objs, probs)
    # the objectness-zero detection 1 swaps with the last (3), which is checked again and kept: [0, 3, 2 | 1]; sorting by
    # the score gives 2, 3, 0, then 3 suppresses 0 (IoU ~ 0.9 > 0.45) and 2 is far from both
    assert order == [2, 3, 0, 1]
    assert p[:, 0].tolist() == [0, 0, pytest.approx(.8), pytest.approx(.7)]


def test_oracle_record_truncation():
    boxes = np.array([[.5, .5, .4, .4]] * 3, np.float32)
    probs = np.array([[.9], [.8], [.7]], np.float32)
    full = ref.records(boxes, probs, [0, 1, 2], 100, 50, .5, 1000)
    assert len(full) == 3
    # result_idx * 6 + 5 < result_sz: result_sz = 12 holds two records, 11 one
    assert len(ref.records(boxes, probs, [0, 1, 2], 100, 50, .5, 12 // 6)) == 2
    assert len(ref.records(boxes, probs, [0, 1, 2], 100, 50, .5, 11 // 6)) == 1
    # (float32 0.4 / 2. lies just above 0.2: (0.5 - 0.2) * 100 = 29.99... truncates to 29, (0.5 + 0.2) * 100 to 70)
    assert full[0].tolist() == [0, pytest.approx(.9), 29, 14, 41, 21]
