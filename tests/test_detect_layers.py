"""Every layer kernel of the device detector alone, over the shape sweep of detect_cases.py: layer l of the restatement in
float64 on the device's OWN debug_tensor(l - 1) against the device's layer l, at B = 1 and B = 3 (a 64-wide tile of the implicit
GEMM then straddles images).  maxpool / route / upsample / shortcut bit-identical, convolution within the forward-error bound
of any summation order, logistic / yolo / region within counted float32 ulps (all derived in detect_cases.py).

The non-GPU tests at the end perturb the restatement and require the same check to reject the result: the sweep can fail."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import darknet_ref as ref  # noqa: E402
import detect_cases as dc  # noqa: E402
import svo_loader  # noqa: E402

SWEEP = dc.sweep_cfgs()


@pytest.fixture(scope="module")
def pkg():
    return svo_loader.load()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SWEEP))
def test_every_layer_kernel_alone(pkg, tmp_path, name):
    import torch
    cfg, w, net, params = dc.write_case(tmp_path, name, SWEEP[name], seed=5)
    W, H = 50, 37
    worst = 0.0
    for B in (1, 3):
        imgs = [dc.sweep_image(20 + b, W, H) for b in range(B)]
        det = pkg.Detector(cfg, w, max_batch=B)
        d_img = torch.from_numpy(np.stack(imgs)).cuda()
        rec = torch.zeros(B * 50 * 6, dtype=torch.float32, device="cuda")
        nrec = torch.zeros(B, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        det.batch_dev(d_img.data_ptr(), W, H, 3, 3 * W, B, dc.SWEEP_THRESH, rec.data_ptr(), 50, nrec.data_ptr())
        det.sync()
        x = np.stack([det.debug_tensor(-1, b) for b in range(B)])
        assert x.tobytes() == np.stack([ref.letterbox(im, net["w"], net["h"]) for im in imgs]).tobytes()
        outs = [np.stack([det.debug_tensor(li, b) for b in range(B)]) for li in range(len(net["layers"]))]
        det.close()
        fails, conv_ratio, other_ratio = dc.network_check(net, params, x, outs)
        print("%s B=%d: device: largest convolution error / bound %.3f, other bounded layers %.3f" % (name, B, conv_ratio, other_ratio))
        assert not fails, "B = %d:\n%s" % (B, "\n".join(fails))
        worst = max(worst, conv_ratio)
    assert worst > 0, "no convolution erred at all: the comparison shows nothing"


# ---- sensitivity (no GPU): a subtly wrong layer must fall outside the per-layer check ----
def _restated(tmp_path, name, seed=5):
    cfg, w, net, params = dc.write_case(tmp_path, name, SWEEP[name], seed=seed)
    x = ref.letterbox(dc.sweep_image(20, 50, 37), net["w"], net["h"])[None]
    return net, params, x, ref.forward(net, params, x, np.float32)


@pytest.mark.parametrize("name", sorted(SWEEP))
def test_float32_restatement_passes_the_per_layer_check(tmp_path, name):
    """The check accepts an honest float32 implementation with another summation order (the restatement's own)."""
    net, params, x, outs = _restated(tmp_path, name)
    fails, conv_ratio, _ = dc.network_check(net, params, x, outs)
    assert not fails, "\n".join(fails)
    assert conv_ratio <= 1


def test_dropping_the_last_k_of_a_17_wide_convolution_is_rejected(tmp_path):
    net, params, x, outs = _restated(tmp_path, "k_slice")
    li = next(i for i, L in enumerate(net["layers"]) if L["type"] == ref.CONV and L["in_c"] * L["size"] ** 2 == 17)
    P = ref.split_params(net, params)
    assert dc.layer_check(net, P, li, outs[li - 1], outs[:li], outs[li])[0]
    short = dict(P)
    wt = P[li][4].copy()
    wt[:, -1] = 0                                    # k = 16, the one entry past the 16-wide slice, never accumulated
    short[li] = P[li][:4] + (wt,)
    wrong = ref.apply_layer(net, short, li, outs[li - 1], outs[:li], np.float32)
    ok, ratio, msg = dc.layer_check(net, P, li, outs[li - 1], outs[:li], wrong)
    assert not ok and ratio > 1, "a convolution that drops its last k passed the bound"
    # even when only one output row does it
    wrong1 = outs[li].copy()
    wrong1[:, 3] = wrong[:, 3]
    assert not dc.layer_check(net, P, li, outs[li - 1], outs[:li], wrong1)[0]


@pytest.mark.parametrize("change", ["window_shifted_by_one", "size_over_2_padding"])
def test_a_wrong_maxpool_is_rejected(tmp_path, change):
    net, params, x, outs = _restated(tmp_path, "maxpool")
    P = ref.split_params(net, params)
    pools = [i for i, L in enumerate(net["layers"]) if L["type"] == ref.MAXPOOL]
    rejected = 0
    for li in pools:
        L = net["layers"][li]
        assert dc.layer_check(net, P, li, outs[li - 1], outs[:li], outs[li])[0]
        bad = copy.deepcopy(net)
        if change == "window_shifted_by_one":
            bad["layers"][li]["pad"] = L["pad"] + 1
        else:
            if L["pad"] != (L["size"] - 1) // 2 or L["size"] // 2 == L["pad"]:
                continue                              # (explicit padding; odd sizes: size / 2 = (size - 1) / 2, nothing to tell apart)
            bad["layers"][li]["pad"] = L["size"] // 2
        wrong = ref.apply_layer(bad, P, li, outs[li - 1], outs[:li], np.float32)
        assert wrong.shape == outs[li].shape
        assert not dc.layer_check(net, P, li, outs[li - 1], outs[:li], wrong)[0], "layer %d: the wrong maxpool passed" % li
        rejected += 1
    assert rejected >= 2
