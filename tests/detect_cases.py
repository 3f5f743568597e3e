"""Generated detector networks and the per-layer checks shared by test_detect_ref.py (restatement against the reference's
darknet on the CPU), test_detect_layers.py (every device layer kernel alone) and test_detect_scale.py (decode / NMS /
records past the 1024-candidate chunk).  Nothing here is collected by pytest.

Per-layer rule: layer l of the restatement is applied in float64 to the implementation's OWN layer l - 1 output, so an error
does not widen with depth and a small error in a late layer is seen.
 - maxpool, route, upsample move or compare floats: bit-identical.  shortcut is one float add: bit-identical (the float64 sum
   of two floats rounded to float is the float sum: 53 >= 2 * 24 + 2 bits make the double rounding innocuous).
 - convolution: the forward-error bound every summation order satisfies (conv_check).
 - logistic / yolo / region entries: ulps of float32 around the float64 value (logistic_bound, region softmax in layer_check)."""
import os

import numpy as np
import torch

import darknet_ref as ref

U = 2.0 ** -24            # unit roundoff of float32 (round to nearest)
UD = 2.0 ** -50           # room for the double steps (exp, add, divide: a few units of 2^-53 each), see logistic_bound


def _gamma(n):
    return n * U / (1 - n * U)


def _round(v, e, u=U):
    """Error bound after one rounding of a computed value whose exact counterpart is v and whose error so far is e."""
    return e + u * (np.abs(v) + e)


def logistic_bound(v, e_in=0.0):
    """|(float)(1. / (1. + exp((double)-x))) - logistic(v)| for an input x with |x - v| <= e_in.  Counted: logistic' <= 1/4
    carries e_in; the double exp (1 ulp of double on either side), add and divide stay below 2^-50 relative; one rounding to
    float is half a float ulp of the result (<= 2^-24 relative).  A device exp one double ulp off moves the double result by
    2^-53 relative, far inside the 2^-50 term, and can only flip the float rounding when the double lies within that distance
    of a rounding boundary - where both neighbours are within half an ulp + 2^-50."""
    with np.errstate(over="ignore"):
        y = 1. / (1. + np.exp(-v))
    return y, e_in / 4 + (U + UD) * y + 2.0 ** -149


def conv_check(L, P, x):
    """-> (float64 value, bound) of a convolutional layer on the float32 input x (B x C x H x W).
    acc = sum of K float products in any order: |acc - S| <= gamma_K * conv(|w|, |x|), gamma_K = K u / (1 - K u), u = 2^-24
    (K roundings of products and K - 1 of sums reach at most K per term; zero padding adds exact zeros).  Then the epilogue's
    roundings, each u * |result| on top of the carried error, counted from the operations:
      batch_normalize: (acc - mean) 1, the double divide by sqrt(var) + .000001f rounded to float 1, * scale 1, + bias 1  -> c = 4
      without:         + bias 1                                                                                      -> c = 1
      leaky adds 1 ((float)(.1 * x); where the sign of x is inside its error the two branches differ by 0.9 |x|), logistic
      see logistic_bound.  The error before the divide is carried through |scale| / (sqrt(var) + .000001f)."""
    bias, sc, mu, var, wt = P
    K = wt.shape[1] * wt.shape[2] * wt.shape[3]
    x64 = torch.from_numpy(np.ascontiguousarray(x.astype(np.float64)))
    w64 = wt.astype(np.float64)
    S = torch.nn.functional.conv2d(x64, torch.from_numpy(w64), stride=L["stride"], padding=L["pad"]).numpy()
    A = torch.nn.functional.conv2d(x64.abs(), torch.from_numpy(np.abs(w64)), stride=L["stride"], padding=L["pad"]).numpy()
    f = lambda a: a.astype(np.float64)[None, :, None, None]
    e = _gamma(K) * A
    if L["bn"]:
        den = np.sqrt(f(var)) + np.float64(np.float32(.000001))
        v = S - f(mu)
        e = _round(v, e)
        v = v / den
        e = _round(v, e / den, U + UD)
        v = v * f(sc)
        e = _round(v, e * np.abs(f(sc)))
        v = v + f(bias)
        e = _round(v, e)
    else:
        v = S + f(bias)
        e = _round(v, e)
    if L["act"] == "leaky":
        flip = np.abs(v) <= e
        v5 = np.where(v > 0, v, .1 * v)
        e = _round(v5, e, U + UD) + np.where(flip, 0.9 * np.abs(v), 0.)
        v = v5
    elif L["act"] == "logistic":
        v, e = logistic_bound(v, e)
    return v, e


def layer_check(net, P, li, cur, outs, got):
    """Implementation output `got` (B x C x H x W float32) of layer li against the restatement applied to the implementation's
    own input `cur` and earlier outputs `outs`.  -> (ok, largest error / bound or None for the bit-identical kinds, message)."""
    L = net["layers"][li]
    t = L["type"]
    got = np.asarray(got, np.float32)
    if t in (ref.MAXPOOL, ref.ROUTE, ref.UPSAMPLE, ref.SHORTCUT):
        want = ref.apply_layer(net, P, li, cur, outs, np.float64).astype(np.float32)
        if want.shape != got.shape:
            return False, None, "layer %d: shape %s, restatement %s" % (li, got.shape, want.shape)
        same = want.tobytes() == got.tobytes()
        return same, None, "" if same else "layer %d (type %d): %d of %d values differ from the restatement (must be bit-identical)" % (
            li, t, int((want.view(np.uint32) != got.view(np.uint32)).sum()), want.size)
    if t == ref.CONV:
        v, e = conv_check(L, P[li], cur)
    else:
        B, C, H, W = cur.shape
        E = L["classes"] + 5
        x = cur.astype(np.float64).reshape(B, L["n"], E, H, W)
        v, e = logistic_bound(x)
        v[:, :, 2:4] = x[:, :, 2:4]          # w, h are copied
        e[:, :, 2:4] = 0
        if t == ref.REGION and L["softmax"]:
            # blas.c softmax: d = fl(x - largest) (exp(d (1 + delta)) = exp(d) (1 + |d| u)), e = (float)exp(d) (u), the sum in
            # class order (each term's error + classes - 1 adds), one divide (u):
            # relative (|d_j| + 1) + (max |d| + 1) + (classes - 1) + 1 roundings, as gamma_n
            cl = x[:, :, 5:]
            d = cl - cl.max(axis=2, keepdims=True)
            ex = np.exp(d)
            sm = ex / ex.sum(axis=2, keepdims=True)
            n = np.abs(d) + np.abs(d).max(axis=2, keepdims=True) + L["classes"] + 2
            v[:, :, 5:] = sm
            e[:, :, 5:] = (n * U / (1 - n * U) + UD) * sm + 2.0 ** -149
        v, e = v.reshape(B, C, H, W), e.reshape(B, C, H, W)
    if v.shape != got.shape:
        return False, None, "layer %d: shape %s, restatement %s" % (li, got.shape, v.shape)
    err = np.abs(got.astype(np.float64) - v)
    bad = ~(err <= e)         # (a NaN fails)
    exact = e == 0
    ratio = float((err[~exact] / e[~exact]).max()) if (~exact).any() else 0.0
    msg = ""
    if bad.any():
        k = np.unravel_index(np.argmax(np.where(bad, err - e, -np.inf)), err.shape)
        msg = "layer %d (type %d): %d of %d values outside the bound; worst at %s: got %.9g, float64 %.9g, error %.3g > bound %.3g" % (
            li, t, int(bad.sum()), bad.size, k, got[k], v[k], err[k], e[k])
    return not bad.any(), ratio, msg


def network_check(net, params, x, outs_impl):
    """Every layer of one forward: x the network input (B x 3 x h x w), outs_impl[l] the implementation's layer outputs
    (B x C x H x W).  -> (messages of the layers that fail, largest convolution ratio, largest ratio of the other bounded)."""
    P = ref.split_params(net, params)
    fails, conv_ratio, other_ratio = [], 0.0, 0.0
    for li, L in enumerate(net["layers"]):
        cur = x if li == 0 else outs_impl[li - 1]
        ok, ratio, msg = layer_check(net, P, li, cur, outs_impl[:li], outs_impl[li])
        if not ok:
            fails.append(msg)
        if ratio is not None:
            if L["type"] == ref.CONV:
                conv_ratio = max(conv_ratio, ratio)
            else:
                other_ratio = max(other_ratio, ratio)
    return fails, conv_ratio, other_ratio


# ---- the sweep networks: one or two layers under test behind a leading convolution that sets in_c ----
def _net(w, h):
    return "[net]\nwidth=%d\nheight=%d\nchannels=3\n\n" % (w, h)


def _conv(filters, size=1, stride=1, pad=None, padding=None, bn=0, act="leaky"):
    s = "[convolutional]\n"
    if bn:
        s += "batch_normalize=1\n"
    s += "filters=%d\nsize=%d\nstride=%d\n" % (filters, size, stride)
    if pad is not None:
        s += "pad=%d\n" % pad
    if padding is not None:
        s += "padding=%d\n" % padding
    if act is not None:            # (absent: darknet's default, logistic)
        s += "activation=%s\n" % act
    return s + "\n"


def _yolo(classes=2, num=1, mask="0", anchors="10,14"):
    s = "[yolo]\n"
    if mask is not None:
        s += "mask=%s\n" % mask
    if anchors is not None:
        s += "anchors=%s\n" % anchors
    return s + "classes=%d\nnum=%d\n\n" % (classes, num)


def _head(classes=2, n=1, **kw):
    return _conv(n * (classes + 5), act="linear") + _yolo(classes=classes, **kw)


def sweep_cfgs():
    """name -> cfg text.  Maps stay at or below 64 x 64."""
    c = {}
    # activations and batch_normalize: logistic by default (no key), leaky without BN, logistic with BN, linear with BN
    c["act"] = (_net(20, 12) + _conv(6, 3, 1, pad=1, act=None) + _conv(5, 3, 1, pad=1, bn=0, act="leaky") +
                _conv(4, 1, 1, bn=1, act="logistic") + _conv(6, 3, 1, pad=1, bn=1, act="linear") + _head())
    # explicit padding= (wider than size / 2, and none), sizes 2, 5 and 7, strides 2 and 3, and darknet53's downsampling
    # convolution (size 3, stride 2, pad=1) on an odd map
    c["sizes"] = (_net(31, 23) + _conv(6, 3, 2, pad=1, bn=1) + _conv(5, 3, 2, pad=1, bn=1) + _conv(4, 3, 1, pad=1, bn=1) +
                  _head())
    c["sizes2"] = (_net(31, 23) + _conv(3, 2, 1, padding=0, bn=1) + _conv(4, 5, 3, pad=1, bn=1) +
                  _conv(5, 7, 2, padding=3, bn=0) + _conv(3, 3, 1, padding=2, bn=1) + _conv(4, 2, 2, padding=1) + _head())
    # in_c of 1 and 2, K of 1, 2, 3 (below one MFMA step), 9 and 18
    c["small_k"] = (_net(16, 10) + _conv(1, 1, 1, bn=1) + _conv(2, 1, 1, bn=1) + _conv(3, 1, 1, bn=1) + _conv(1, 1, 1) +
                    _conv(2, 3, 1, pad=1, bn=1) + _conv(4, 3, 1, pad=1, bn=1) + _head())
    # K around the 16-wide slice: 15, 16, 17, then 33 = two slices and one
    c["k_slice"] = (_net(12, 9) + _conv(15, 1, 1, bn=1) + _conv(16, 1, 1, bn=1) + _conv(17, 1, 1, bn=1) +
                    _conv(33, 1, 1, bn=1) + _conv(8, 1, 1, bn=1) + _head())
    # M of 1, 63, 64, 65 (and 130: three tiles of rows)
    c["m_tile"] = (_net(11, 7) + _conv(63, 3, 1, pad=1, bn=1) + _conv(64, 1, 1, bn=1) + _conv(65, 1, 1, bn=1) +
                   _conv(1, 1, 1, bn=1) + _conv(130, 3, 1, pad=1) + _head())
    # N = B * out_h * out_w of 1 (3 in a batch of 3): an 8 x 8 kernel over the whole 8 x 8 map
    c["n_one"] = _net(8, 8) + _conv(4, 3, 1, pad=1, bn=1) + _conv(7, 8, 8, padding=0, bn=1) + _head()
    # N exactly on the 64 tile (8 x 8; 192 = three whole tiles at B = 3) and just over it (13 x 5 = 65; 195 at B = 3, where
    # a tile straddles two images)
    c["n_64"] = _net(8, 8) + _conv(5, 3, 1, pad=1, bn=1) + _conv(6, 1, 1, bn=1) + _head()
    c["n_65"] = _net(13, 5) + _conv(5, 3, 1, pad=1, bn=1) + _conv(6, 1, 1, bn=1) + _head()
    # maxpool: 3 / 2, 2 / 2, 2 / 1 (tiny-yolo's last), explicit padding, size alone defaulting from stride
    c["maxpool"] = (_net(27, 19) + _conv(5, 3, 1, pad=1, bn=1) + "[maxpool]\nsize=3\nstride=2\n\n" + "[maxpool]\nsize=2\nstride=2\n\n" +
                    "[maxpool]\nsize=2\nstride=1\n\n" + "[maxpool]\nsize=3\nstride=1\npadding=2\n\n" + "[maxpool]\nstride=3\n\n" +
                    "[maxpool]\nsize=4\nstride=2\npadding=0\n\n" + _head())
    # the SPP block: 5 / 9 / 13 at stride 1 with darknet's (size - 1) / 2 padding; (w + 2 * pad) / stride GROWS the map, so the
    # three pools cannot be routed together with their source (yolov3-spp relies on a later darknet's rule); each is checked alone
    c["spp"] = (_net(19, 13) + _conv(4, 1, 1, bn=1) + "[maxpool]\nsize=5\nstride=1\n\n" + "[route]\nlayers=-2\n\n" +
                "[maxpool]\nsize=9\nstride=1\n\n" + "[route]\nlayers=0\n\n" + "[maxpool]\nsize=13\nstride=1\n\n" + _head())
    # upsample strides 1, 3, 4
    c["upsample"] = (_net(6, 4) + _conv(3, 1, 1, bn=1) + "[upsample]\nstride=1\n\n" + "[upsample]\nstride=3\n\n" +
                     "[upsample]\nstride=4\n\n" + _head())
    # routes of 3 and 4 sources with unequal channel counts, absolute and relative indices, and a shortcut
    c["route"] = (_net(14, 10) + _conv(3, 3, 1, pad=1, bn=1) + _conv(7, 1, 1, bn=1) + _conv(2, 3, 1, pad=1, bn=1) + _conv(5, 1, 1, bn=1) +
                  "[route]\nlayers=-1,1,-2\n\n" + "[route]\nlayers=0,-2,3,-1\n\n" + _conv(5, 1, 1, bn=1) +
                  "[shortcut]\nfrom=3\nactivation=linear\n\n" + _head())
    # [yolo] without mask (every anchor), anchors shorter than 2 * num (the rest stay 0.5)
    c["yolo_nomask"] = _net(10, 6) + _conv(4, 3, 1, pad=1, bn=1) + _conv(3 * 8, act="linear") + _yolo(classes=3, num=3, mask=None, anchors="4,5,6")
    # [yolo] of one class with a mask that picks anchors out of order
    c["yolo_one_class"] = _net(10, 6) + _conv(4, 3, 1, pad=1, bn=1) + _conv(2 * 6, act="linear") + _yolo(classes=1, num=4, mask="3,1",
                                                                                                         anchors="2,3,4,5,6,7,8,9")
    # [region]: softmax=0 (logistic classes), one class with softmax, anchors shorter than 2 * num
    region = lambda classes, num, softmax, anchors: (_conv(num * (classes + 5), act="linear") +
                                                     "[region]\nanchors=%s\nclasses=%d\ncoords=4\nnum=%d\nsoftmax=%d\n\n" % (anchors, classes, num, softmax))
    c["region_logistic"] = _net(9, 7) + _conv(4, 3, 1, pad=1, bn=1) + region(3, 2, 0, "1.5,2,3,2.5")
    c["region_one_class"] = _net(9, 7) + _conv(4, 3, 1, pad=1, bn=1) + region(1, 2, 1, "1.5,2,3")
    c["region_softmax"] = _net(9, 7) + _conv(4, 3, 1, pad=1, bn=1) + region(6, 3, 1, "1,2,3,4")
    return c


SWEEP_THRESH = 0.3


def write_case(tmp_path, name, text, seed=1, params=None):
    """-> (cfg path, weights path, parsed net, parameter array)"""
    cfg = str(tmp_path / (name + ".cfg"))
    with open(cfg, "w") as f:
        f.write(text)
    net = ref.parse_cfg(cfg)
    if params is None:
        params = ref.seeded_params(net, seed)
    w = str(tmp_path / (name + ".weights"))
    ref.write_weights(w, params)
    return cfg, w, net, params


def sweep_image(seed, W, H):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (H, W, 3)).astype(np.uint8)


# ---- probe heads: one 1 x 1 linear convolution and an output layer, every logit one exact product plus a bias ----
def probe_cfg(w, h, kind="yolo", classes=2, anchors=((10, 14), (23, 27), (37, 58)), softmax=0):
    n = len(anchors)
    an = ",".join("%g,%g" % a for a in anchors)
    s = _net(w, h) + _conv(n * (classes + 5), act="linear")
    if kind == "yolo":
        s += _yolo(classes=classes, num=n, mask=",".join(str(i) for i in range(n)), anchors=an)
    else:
        s += "[region]\nanchors=%s\nclasses=%d\ncoords=4\nnum=%d\nsoftmax=%d\n\n" % (an, classes, n, softmax)
    return s


def probe_params(n, classes, obj_gain=8.0, obj_bias=-4.0, cls_gain=8.0, cls_bias=-3.0, size_gain=1.0, size_bias=-0.5, seed=0):
    """The 1 x 1 convolution of a probe head: (biases, weights[filters][3]) flattened in file order.  Each weight row has one
    non-zero entry, a power of two: image channel 0 drives objectness, channel 1 the x / y offsets and the class scores, channel
    2 the box sizes.  Biases differ by anchor and class, so that scores do not repeat across them."""
    for g in (obj_gain, cls_gain, size_gain):
        assert g == 2.0 ** round(np.log2(g))
    rng = np.random.default_rng(seed)
    E = classes + 5
    wt = np.zeros((n * E, 3), np.float32)
    bias = np.zeros(n * E, np.float32)
    for a in range(n):
        r = a * E
        wt[r + 0, 1] = 4.0; bias[r + 0] = -2.0
        wt[r + 1, 1] = 2.0; bias[r + 1] = -1.0
        wt[r + 2, 2] = size_gain; bias[r + 2] = size_bias + 0.125 * a
        wt[r + 3, 2] = size_gain; bias[r + 3] = size_bias - 0.0625 * a
        wt[r + 4, 0] = obj_gain; bias[r + 4] = obj_bias + 0.03125 * a
        for k in range(classes):
            wt[r + 5 + k, 1] = cls_gain / 2 ** (k % 3)      # (softmax: the classes must not move together)
            bias[r + 5 + k] = cls_bias + rng.uniform(0, 2)
    return np.concatenate([bias, wt.reshape(-1)]).astype(np.float32)


def probe_image(seed, w, h, obj_share=0.5, n_hi=None):
    """Random bytes with every cell's (channel 0, channel 1) pair different from every other cell's (w * h <= 65536), so that two
    cells of one anchor never share objectness and class logits; about `obj_share` of the cells get channel 0 >= 128 (a positive
    objectness logit under the default probe_params)."""
    rng = np.random.default_rng(seed)
    assert w * h <= 32768
    hi = rng.random(w * h) < obj_share
    if n_hi is not None:           # exactly n_hi cells with a positive objectness logit
        hi = np.zeros(w * h, bool)
        hi[rng.choice(w * h, n_hi, replace=False)] = True
    pairs = np.empty(w * h, np.int64)
    pairs[hi] = 32768 + rng.choice(32768, int(hi.sum()), replace=False)
    pairs[~hi] = rng.choice(32768, int((~hi).sum()), replace=False)
    img = np.zeros((h, w, 3), np.uint8)
    img[:, :, 0] = (pairs >> 8).reshape(h, w)
    img[:, :, 1] = (pairs & 255).reshape(h, w)
    img[:, :, 2] = rng.integers(0, 256, (h, w))
    return img


def decode_stats(net, outs_img, imw, imh, thresh):
    """What the restatement sees of one image's output tensors: T candidates, total after the zero-objectness swap, the largest
    per-class count m of non-zero scores, whether two non-zero scores of one class are equal (ties)."""
    boxes, objs, probs = ref.network_boxes(net, outs_img, imw, imh, thresh)
    T = len(objs)
    total = int((objs != 0).sum())
    m = [int((probs[:, c] != 0).sum()) for c in range(probs.shape[1])] if T else [0]
    ties = False
    for c in range(probs.shape[1] if T else 0):
        nz = probs[:, c][probs[:, c] != 0]
        ties = ties or len(np.unique(nz)) != len(nz)
    return dict(T=T, total=total, m=max(m), ties=ties, boxes=boxes, objs=objs, probs=probs)


def records_from(stats, imw, imh, thresh, max_records):
    order, probs = ref.nms_sort_fast(stats["boxes"], stats["objs"], stats["probs"])
    return ref.records(stats["boxes"], probs, order, imw, imh, thresh, max_records)


_QSORT_STABLE = None


def compare_with_darknet(got, dn, ties):
    """Records `got` against YoloDetectFromImage's `dn`.  -> which comparison ran (for the test's printed line).
    do_nms_sort qsorts ALL detections of a class, the many with score 0 included; they compare equal, and their order after the
    last class's sort is the order of the records.  C leaves the order of equal elements open, so a byte-for-byte comparison
    with darknet rests on this libc's qsort keeping it (glibc's merge sort does), as the device and the restatement do.  That
    is probed once (oracle.binding.ref_qsort_is_stable), not assumed:
     - stable: byte for byte, equal non-zero scores included;
     - not stable, no two equal non-zero scores in a class: suppression still sees one order, so the same records come out in
       an order the zeros leave open: compared as multisets (only when nothing was cut by max_records);
     - not stable, ties: darknet's own result is open; not compared."""
    global _QSORT_STABLE
    from oracle import binding as ob
    if _QSORT_STABLE is None:
        _QSORT_STABLE = ob.ref_qsort_is_stable()
    if _QSORT_STABLE:
        assert got.shape == dn.shape, "%d records, darknet's YoloDetectFromImage %d" % (len(got), len(dn))
        assert got.tobytes() == dn.tobytes(), "records differ from the reference's YoloDetectFromImage"
        return "darknet: byte for byte (libc qsort probed stable)"
    if ties:
        return "darknet: NOT compared (libc qsort not stable, and equal non-zero scores)"
    key = lambda r: sorted(map(tuple, r.tolist()))
    assert key(got) == key(dn), "records differ from the reference's YoloDetectFromImage as multisets"
    return "darknet: as multisets (libc qsort not stable)"
