"""Independent numpy restatement of the darknet detector path the device implements (svo_det_*): the .cfg shape rules,
the .weights layout, letterbox_image, every supported layer (in float64 and in float32 with darknet's own roundings),
get_network_boxes, do_nms_sort and YoloDetect's record loop.  Restated from darknet's parser.c, image.c, blas.c,
*_layer.c, box.c and yolo_v3.c - not from the library under test.

Ties: darknet sorts with libc qsort, whose order for equal scores is unspecified; here (as on the device) a stable sort."""
import struct

import numpy as np
import torch

CONV, MAXPOOL, ROUTE, SHORTCUT, UPSAMPLE, YOLO, REGION = range(7)
_TYPES = {"convolutional": CONV, "conv": CONV, "maxpool": MAXPOOL, "max": MAXPOOL, "route": ROUTE, "shortcut": SHORTCUT,
          "upsample": UPSAMPLE, "yolo": YOLO, "region": REGION}


def parse_cfg(path):
    secs = []
    for line in open(path):
        s = "".join(ch for ch in line if ch not in " \t\n\r")
        if not s or s[0] in "#;":
            continue
        if s[0] == "[":
            secs.append((s[1:-1], {}))
        else:
            k, v = s.split("=", 1)
            secs[-1][1].setdefault(k, v)
    net = secs[0][1]
    w, h, c = int(net["width"]), int(net["height"]), int(net["channels"])
    layers = []
    for typ, o in secs[1:]:
        t = _TYPES[typ]
        L = dict(type=t, in_w=w, in_h=h, in_c=c, n_params=0)
        gi = lambda k, d: int(o.get(k, d))
        if t == CONV:
            f, size, stride = gi("filters", 1), gi("size", 1), gi("stride", 1)
            pad = size // 2 if gi("pad", 0) else gi("padding", 0)
            bn = gi("batch_normalize", 0)
            L.update(filters=f, size=size, stride=stride, pad=pad, bn=bn, act=o.get("activation", "logistic"),
                     out_w=(w + 2 * pad - size) // stride + 1, out_h=(h + 2 * pad - size) // stride + 1, out_c=f)
            L["n_params"] = f * (4 if bn else 1) + f * c * size * size
        elif t == MAXPOOL:
            stride = gi("stride", 1)
            size = gi("size", stride)
            pad = gi("padding", (size - 1) // 2)
            L.update(size=size, stride=stride, pad=pad, out_w=(w + 2 * pad) // stride, out_h=(h + 2 * pad) // stride, out_c=c)
        elif t == ROUTE:
            idx = [int(x) for x in o["layers"].split(",")]
            idx = [i + len(layers) if i < 0 else i for i in idx]
            L.update(route=idx, out_w=layers[idx[0]]["out_w"], out_h=layers[idx[0]]["out_h"],
                     out_c=sum(layers[i]["out_c"] for i in idx))
        elif t == SHORTCUT:
            fr = int(o["from"])
            L.update(frm=fr + len(layers) if fr < 0 else fr, out_w=w, out_h=h, out_c=c)
        elif t == UPSAMPLE:
            s_ = gi("stride", 2)
            L.update(stride=s_, out_w=w * s_, out_h=h * s_, out_c=c)
        elif t == YOLO:
            total = gi("num", 1)
            mask = [int(x) for x in o["mask"].split(",")] if "mask" in o else list(range(total))
            biases = [.5] * (2 * total)
            if "anchors" in o:
                for i, x in enumerate(o["anchors"].split(",")):
                    biases[i] = float(x)
            b32 = np.array(biases, np.float32)
            L.update(classes=gi("classes", 20), n=len(mask), anchors=[(b32[2 * m], b32[2 * m + 1]) for m in mask],
                     out_w=w, out_h=h, out_c=c)
        elif t == REGION:
            num = gi("num", 1)
            biases = [.5] * (2 * num)
            if "anchors" in o:
                for i, x in enumerate(o["anchors"].split(",")):
                    biases[i] = float(x)
            b32 = np.array(biases, np.float32)
            L.update(classes=gi("classes", 20), n=num, softmax=gi("softmax", 0),
                     anchors=[(b32[2 * k], b32[2 * k + 1]) for k in range(num)], out_w=w, out_h=h, out_c=c)
        w, h, c = L["out_w"], L["out_h"], L["out_c"]
        layers.append(L)
    return dict(w=int(net["width"]), h=int(net["height"]), c=int(net["channels"]), layers=layers)


def n_params(net):
    return sum(L["n_params"] for L in net["layers"])


def seeded_params(net, seed, obj_bias=1.0, cls_bias=1.0, head_scale=0.3):
    """Per convolutional layer (biases, scales, mean, var, weights) keeping activations O(1): He-scaled kernels, BN scale and
    variance in [0.5, 1.5].  The convolutions feeding an output layer get small kernels and biases that put objectness and
    class scores around logistic(obj_bias) / logistic(cls_bias), so that some boxes pass a threshold and NMS has work."""
    rng = np.random.default_rng(seed)
    heads = {i - 1 for i, L in enumerate(net["layers"]) if L["type"] in (YOLO, REGION)}
    out = []
    for i, L in enumerate(net["layers"]):
        if L["type"] != CONV:
            continue
        f, k = L["filters"], L["in_c"] * L["size"] ** 2
        wt = rng.standard_normal((f, k)) * np.sqrt(2.0 / k)
        bias = rng.uniform(-0.1, 0.1, f)
        if i in heads:
            wt *= head_scale / np.sqrt(2.0)
            nxt = net["layers"][i + 1]
            E = nxt["classes"] + 5
            for a in range(nxt["n"]):
                bias[a * E + 4] = obj_bias
                bias[a * E + 5:(a + 1) * E] = cls_bias + rng.uniform(-1.5, 0.5, nxt["classes"])
        p = [bias]
        if L["bn"]:
            p += [rng.uniform(0.5, 1.5, f), rng.uniform(-0.1, 0.1, f), rng.uniform(0.5, 1.5, f)]
        p.append(wt.reshape(-1))
        out.append(np.concatenate(p).astype(np.float32))
    return np.concatenate(out)


def write_weights(path, params, major=0, minor=2, revision=0, seen=0):
    with open(path, "wb") as f:
        f.write(struct.pack("<iii", major, minor, revision))
        if major * 10 + minor >= 2 and major < 1000 and minor < 1000:
            f.write(struct.pack("<Q", seen))
        else:
            f.write(struct.pack("<i", seen))
        f.write(np.asarray(params, np.float32).tobytes())


def split_params(net, params):
    """{layer index: (bias, scale, mean, var, weights[f][c][s][s])} from the flat parameter array."""
    out, o = {}, 0
    for i, L in enumerate(net["layers"]):
        if L["type"] != CONV:
            continue
        f = L["filters"]
        bias = params[o:o + f]; o += f
        sc = mu = var = None
        if L["bn"]:
            sc, mu, var = params[o:o + f], params[o + f:o + 2 * f], params[o + 2 * f:o + 3 * f]
            o += 3 * f
        n = f * L["in_c"] * L["size"] ** 2
        out[i] = (bias, sc, mu, var, params[o:o + n].reshape(f, L["in_c"], L["size"], L["size"]))
        o += n
    assert o == len(params)
    return out


# ---- letterbox_image of an 8-bit interleaved image (ipl_to_image: data / 255. in double, stored as float) ----
def letterbox_geom(W, H, nw, nh):
    if np.float32(nw) / np.float32(W) < np.float32(nh) / np.float32(H):
        new_w, new_h = nw, (H * nw) // W
    else:
        new_w, new_h = (W * nh) // H, nh
    return new_w, new_h


def planar(img):
    """ipl_to_image: H x W (gray, replicated to three channels) or H x W x C uint8, channel k = byte k -> C x H x W float32."""
    a = img if img.ndim == 3 else np.repeat(img[:, :, None], 3, axis=2)
    return np.ascontiguousarray((a.astype(np.float64) / 255.).astype(np.float32).transpose(2, 0, 1))


def letterbox(img, nw, nh):
    """img: H x W (gray, replicated to three channels) or H x W x C uint8, channel k = byte k.  -> 3 x nh x nw float32."""
    return letterbox_planar(planar(img), nw, nh)


def letterbox_planar(im, nw, nh):
    """letterbox_image of darknet's planar float image (C x H x W float32) -> C x nh x nw float32.  darknet's resize_image
    reads column (int)sx + 1, which its get_pixel asserts to be inside the row; here it is clamped (the device does the same)."""
    im = np.asarray(im, np.float32)
    H, W = im.shape[1:]
    new_w, new_h = letterbox_geom(W, H, nw, nh)
    w_scale = np.float32(W - 1) / np.float32(new_w - 1)
    h_scale = np.float32(H - 1) / np.float32(new_h - 1)
    one = np.float32(1)
    # resize_image, first pass: 3 x H x new_w
    c = np.arange(new_w)
    sx = c.astype(np.float32) * w_scale
    ix = sx.astype(np.int64)
    dx = sx - ix.astype(np.float32)
    ix1 = np.minimum(ix + 1, W - 1)
    part = (one - dx) * im[:, :, ix] + dx * im[:, :, ix1]
    last = (c == new_w - 1) | (W == 1)
    part[:, :, last] = im[:, :, W - 1:W]
    # second pass
    r = np.arange(new_h)
    sy = r.astype(np.float32) * h_scale
    iy = sy.astype(np.int64)
    dy = (sy - iy.astype(np.float32))[None, :, None]
    res = (one - dy) * part[:, iy, :]
    add = dy * part[:, np.minimum(iy + 1, H - 1), :]
    keep = ~((r == new_h - 1) | (H == 1))
    res[:, keep, :] = res[:, keep, :] + add[:, keep, :]
    out = np.full((im.shape[0], nh, nw), np.float32(.5), np.float32)
    dx0, dy0 = (nw - new_w) // 2, (nh - new_h) // 2
    out[:, dy0:dy0 + new_h, dx0:dx0 + new_w] = res
    return out


# ---- forward ----
def _logistic(x, dt):
    return (1. / (1. + np.exp(-x.astype(np.float64)))).astype(dt)


def apply_layer(net, P, i, cur, outs, dtype):
    """Layer i of the network applied to `cur` (B x C x H x W, its input) in `dtype`; `outs`: the earlier layers' outputs
    (route and shortcut read them).  P: split_params(net, params)."""
    dt = np.dtype(dtype)
    L = net["layers"][i]
    cur = cur.astype(dt)
    t = L["type"]
    if t == CONV:
        bias, sc, mu, var, wt = P[i]
        y = torch.nn.functional.conv2d(torch.from_numpy(np.ascontiguousarray(cur)), torch.from_numpy(wt.astype(dt)),
                                       stride=L["stride"], padding=L["pad"]).numpy()
        f = lambda a: a.astype(dt)[None, :, None, None]
        if L["bn"]:
            if dt == np.float64:
                y = (y - f(mu)) / (np.sqrt(f(var)) + np.float64(np.float32(.000001))) * f(sc) + f(bias)
            else:
                den = np.sqrt(var.astype(np.float64)) + np.float64(np.float32(.000001))
                y = ((y - f(mu)).astype(np.float64) / den[None, :, None, None]).astype(dt)
                y = y * f(sc)
                y = y + f(bias)
        else:
            y = y + f(bias)
        if L["act"] == "leaky":
            y = np.where(y > 0, y, (.1 * y.astype(np.float64)).astype(dt))
        elif L["act"] == "logistic":
            y = _logistic(y, dt)
    elif t == MAXPOOL:
        p, s, k = L["pad"], L["stride"], L["size"]
        B, C, H, W = cur.shape
        oh, ow = L["out_h"], L["out_w"]
        padded = np.full((B, C, H + 2 * p + k, W + 2 * p + k), np.finfo(np.float32).min, dt)
        padded[:, :, p:p + H, p:p + W] = cur
        y = np.full((B, C, oh, ow), np.finfo(np.float32).min, dt)
        for n in range(k):
            for m in range(k):
                y = np.maximum(y, padded[:, :, n:n + oh * s:s, m:m + ow * s:s][:, :, :oh, :ow])
    elif t == ROUTE:
        y = np.concatenate([outs[j].astype(dt) for j in L["route"]], axis=1)
    elif t == SHORTCUT:
        y = cur + outs[L["frm"]].astype(dt)
    elif t == UPSAMPLE:
        s = L["stride"]
        y = cur.repeat(s, axis=2).repeat(s, axis=3)
    elif t == YOLO:
        B, C, H, W = cur.shape
        E = L["classes"] + 5
        y = cur.reshape(B, L["n"], E, H, W).copy()
        for e in [0, 1] + list(range(4, E)):
            y[:, :, e] = _logistic(y[:, :, e], dt)
        y = y.reshape(B, C, H, W)
    elif t == REGION:
        B, C, H, W = cur.shape
        E = L["classes"] + 5
        y = cur.reshape(B, L["n"], E, H, W).copy()
        for e in (0, 1, 4):
            y[:, :, e] = _logistic(y[:, :, e], dt)
        cl = y[:, :, 5:]
        if L["softmax"]:
            if dt == np.float32:     # blas.c softmax: float largest, e = (float)exp(x - largest), float sum in class order
                largest = cl.max(axis=2, keepdims=True)
                e = np.exp((cl - largest).astype(np.float64)).astype(np.float32)
                ssum = np.zeros_like(e[:, :, 0:1])
                for j in range(L["classes"]):
                    ssum = ssum + e[:, :, j:j + 1]
                y[:, :, 5:] = e / ssum
            else:
                e = np.exp(cl - cl.max(axis=2, keepdims=True))
                y[:, :, 5:] = e / e.sum(axis=2, keepdims=True)
        else:
            y[:, :, 5:] = _logistic(cl, dt)
        y = y.reshape(B, C, H, W)
    else:
        raise ValueError(t)
    return y


def forward(net, params, x, dtype):
    """x: B x 3 x h x w.  Every layer's output (B x C x H x W) in `dtype`: float64 (exact reference) or float32 (darknet's
    roundings, a different summation order)."""
    P = split_params(net, params)
    outs = []
    cur = x
    for i in range(len(net["layers"])):
        cur = apply_layer(net, P, i, cur, outs, dtype)
        outs.append(cur)
    return outs


# ---- get_network_boxes + do_nms_sort + YoloDetect (float32 with darknet's double steps) ----
def _f(x):
    return np.float32(x)


def network_boxes(net, outs_img, imw, imh, thresh):
    """outs_img: every layer's output of ONE image (float32, C x H x W).  -> (boxes [x, y, w, h], objectness, probs)."""
    netw, neth = net["w"], net["h"]
    classes = next(L["classes"] for L in net["layers"] if L["type"] in (YOLO, REGION))
    new_w, new_h = letterbox_geom(imw, imh, netw, neth)
    boxes, objs, probs = [], [], []
    th = _f(thresh)
    for li, L in enumerate(net["layers"]):
        if L["type"] not in (YOLO, REGION):
            continue
        o = outs_img[li].astype(np.float32)
        H, W = o.shape[1:]
        E = L["classes"] + 5
        o = o.reshape(L["n"], E, H, W)
        if L["type"] == YOLO:
            order = [(i, n) for i in range(W * H) for n in range(L["n"])]
        else:
            order = [(i, n) for n in range(L["n"]) for i in range(W * H)]
        for i, n in order:
            row, col = divmod(i, W)
            v = o[n, :, row, col]
            ob = v[4]
            if L["type"] == YOLO and not ob > th:
                continue
            bx = (_f(col) + v[0]) / _f(W)
            by = (_f(row) + v[1]) / _f(H)
            dw, dh = (netw, neth) if L["type"] == YOLO else (W, H)
            bw = _f(np.exp(np.float64(v[2])) * np.float64(L["anchors"][n][0]) / dw)
            bh = _f(np.exp(np.float64(v[3])) * np.float64(L["anchors"][n][1]) / dh)
            if L["type"] == YOLO:
                obj = ob
                pr = ob * v[5:]
                pr = np.where(pr > th, pr, _f(0))
            else:
                obj = ob if ob > th else _f(0)
                pr = np.zeros(classes, np.float32)
                if obj != 0:
                    pr = ob * v[5:]
                    pr = np.where(pr > th, pr, _f(0))
            bx = _f((np.float64(bx) - (netw - new_w) / 2. / netw) / np.float64(_f(new_w) / _f(netw)))
            by = _f((np.float64(by) - (neth - new_h) / 2. / neth) / np.float64(_f(new_h) / _f(neth)))
            bw = bw * (_f(netw) / _f(new_w))
            bh = bh * (_f(neth) / _f(new_h))
            boxes.append((bx, by, bw, bh))
            objs.append(obj)
            probs.append(pr.astype(np.float32))
    return (np.array(boxes, np.float32).reshape(-1, 4), np.array(objs, np.float32),
            np.array(probs, np.float32).reshape(-1, classes))


def _overlap(x1, w1, x2, w2):
    l1, l2 = x1 - w1 / _f(2), x2 - w2 / _f(2)
    left = l1 if l1 > l2 else l2
    r1, r2 = x1 + w1 / _f(2), x2 + w2 / _f(2)
    right = r1 if r1 < r2 else r2
    return right - left


def box_iou(a, b):
    w = _overlap(a[0], a[2], b[0], b[2])
    h = _overlap(a[1], a[3], b[1], b[3])
    i = _f(0) if (w < 0 or h < 0) else w * h
    u = a[2] * a[3] + b[2] * b[3] - i
    return i / u


def nms_sort(boxes, objs, probs, thresh=.45):
    """do_nms_sort: -> (final order as detection indices, probs after suppression).  Stable sorts (see module doc)."""
    probs = probs.copy()
    T = len(objs)
    perm = list(range(T))
    k = T - 1
    i = 0
    while i <= k:
        if objs[perm[i]] == 0:
            perm[i], perm[k] = perm[k], perm[i]
            k -= 1
            i -= 1
        i += 1
    total = k + 1
    head, tail = perm[:total], perm[total:]
    th = _f(thresh)
    for c in range(probs.shape[1]):
        head.sort(key=lambda d: -float(probs[d, c]))
        m = sum(1 for d in head if probs[d, c] != 0)
        for a in range(m):
            if probs[head[a], c] == 0:
                continue
            A = boxes[head[a]]
            for b in range(a + 1, m):
                if box_iou(A, boxes[head[b]]) > th:
                    probs[head[b], c] = 0
    return head + tail, probs


def _overlap_v(x1, w1, x2, w2):
    l1, l2 = x1 - w1 / _f(2), x2 - w2 / _f(2)
    left = np.where(l1 > l2, l1, l2)
    r1, r2 = x1 + w1 / _f(2), x2 + w2 / _f(2)
    right = np.where(r1 < r2, r1, r2)
    return right - left


def box_iou_v(a, b):
    """box_iou of one box against n (n x 4 float32): float32 elementwise, the operations and their order as in box_iou."""
    w = _overlap_v(a[0], a[2], b[:, 0], b[:, 2])
    h = _overlap_v(a[1], a[3], b[:, 1], b[:, 3])
    i = np.where((w < 0) | (h < 0), _f(0), w * h)
    u = a[2] * a[3] + b[:, 2] * b[:, 3] - i
    with np.errstate(divide="ignore", invalid="ignore"):
        return i / u


def nms_sort_fast(boxes, objs, probs, thresh=.45):
    """nms_sort with the inner loop as float32 numpy elementwise operations (for thousands of candidates per class)."""
    probs = probs.copy()
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    T = len(objs)
    perm = list(range(T))
    k = T - 1
    i = 0
    while i <= k:
        if objs[perm[i]] == 0:
            perm[i], perm[k] = perm[k], perm[i]
            k -= 1
            i -= 1
        i += 1
    total = k + 1
    head, tail = np.array(perm[:total], np.int64), perm[total:]
    th = _f(thresh)
    for c in range(probs.shape[1]):
        head = head[np.argsort(-probs[head, c], kind="stable")]
        m = int((probs[head, c] != 0).sum())
        for a in range(m):
            if probs[head[a], c] == 0:
                continue
            rest = head[a + 1:m]
            hit = box_iou_v(boxes[head[a]], boxes[rest]) > th
            probs[rest[hit], c] = 0
    return [int(d) for d in head] + tail, probs


def records(boxes, probs, order, imw, imh, thresh, max_records):
    """YoloDetect's loop: -> n x 6 float32 [class, prob, left, top, right - left, bot - top]."""
    out = []
    th = _f(thresh)
    for d in order:
        p = probs[d]
        cid = 0
        for j in range(1, len(p)):
            if p[j] > p[cid]:
                cid = j
        pr = p[cid]
        b = boxes[d]
        left = int((np.float64(b[0]) - np.float64(b[2]) / 2.) * imw)
        right = int((np.float64(b[0]) + np.float64(b[2]) / 2.) * imw)
        top = int((np.float64(b[1]) - np.float64(b[3]) / 2.) * imh)
        bot = int((np.float64(b[1]) + np.float64(b[3]) / 2.) * imh)
        left = max(left, 0)
        right = min(right, imw - 1)
        top = max(top, 0)
        bot = min(bot, imh - 1)
        if pr > th and len(out) < max_records:
            out.append((cid, pr, left, top, right - left, bot - top))
    return np.array(out, np.float32).reshape(-1, 6)


def detect_from_outputs(net, outs_img, imw, imh, thresh, max_records=1000, fast=False):
    boxes, objs, probs = network_boxes(net, outs_img, imw, imh, thresh)
    order, probs = (nms_sort_fast if fast else nms_sort)(boxes, objs, probs)
    return records(boxes, probs, order, imw, imh, thresh, max_records)


def tracker_boxes(rec, cap=64):
    """svo_boxes_dev rows {left, right, top, bottom} of the first min(n, cap) records."""
    r = rec[:cap].astype(np.int64)
    return np.stack([r[:, 2], r[:, 2] + r[:, 4], r[:, 3], r[:, 3] + r[:, 5]], axis=1).astype(np.int32).reshape(-1, 4)
