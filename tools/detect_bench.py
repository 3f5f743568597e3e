"""Detector throughput on one GPU (svo_det_batch_dev), with seeded weights, from 1241 x 376 BGR images in HBM:
  - whole-call images/s at each batch size, for darknet53_coco at 416 and the yolov2-tiny-shaped test network at 416;
  - one profiled call per batch size (svo_det_profile: HIP events around every launch): per-layer kernel times, the
    forward (input + layers) apart from the decode + NMS, and the convolutions' own TFLOP/s (multiply-adds counted as two,
    summed over the convolution layers' own times) against the 157 TF f32 matrix peak;
  - the detect + track rate with the tracker as `consumer` (svo_track_batch_bgr_dev on the synthetic sequence's frames,
    no host sync between the two) against track-only on the same frames.
Prints one JSON line.

    python tools/detect_bench.py [--batches 1,8,32,128] [--iters 10]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import darknet_ref as ref  # noqa: E402
import svo_loader  # noqa: E402

PEAK_TF = 157.3


def conv_flops(net):
    return sum(2 * L["filters"] * L["in_c"] * L["size"] ** 2 * L["out_w"] * L["out_h"] for L in net["layers"] if L["type"] == ref.CONV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32,128")
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    import torch
    pkg = svo_loader.load()
    batches = [int(x) for x in a.batches.split(",")]
    W, H = 1241, 376
    rng = np.random.default_rng(0)
    imgs = torch.from_numpy(rng.integers(0, 256, (max(batches), H, W, 3), dtype=np.uint8)).cuda()
    out = {"metric": "detector images/s (1241x376 BGR in HBM, f32 MFMA convolutions)", "peak_tf_f32": PEAK_TF, "nets": {}}
    tmp = tempfile.mkdtemp()
    region416 = os.path.join(tmp, "region416.cfg")
    txt = open(os.path.join(ROOT, "tests", "golden", "tiny_region_small.cfg")).read()
    open(region416, "w").write(txt.replace("width=64", "width=416").replace("height=64", "height=416"))
    for name, cfg in (("darknet53_coco_416", os.path.join(ROOT, "tests", "golden", "darknet53_coco.cfg")),
                      ("yolov2_tiny_shaped_416", region416)):
        net = ref.parse_cfg(cfg)
        wpath = os.path.join(tmp, name + ".weights")
        ref.write_weights(wpath, ref.seeded_params(net, 1))
        fl = conv_flops(net)
        conv_idx = [i for i, L in enumerate(net["layers"]) if L["type"] == ref.CONV]
        ref_names = [["conv", "maxpool", "route", "shortcut", "upsample", "yolo", "region"][L["type"]] for L in net["layers"]]
        res = {"gflop_per_image": fl / 1e9, "batches": {}}
        det = pkg.Detector(cfg, wpath, max_batch=max(batches))
        rec = torch.zeros(max(batches) * 100 * 6, dtype=torch.float32, device="cuda")
        nrec = torch.zeros(max(batches), dtype=torch.int32, device="cuda")
        for B in batches:
            run = lambda: det.batch_dev(imgs.data_ptr(), W, H, 3, 3 * W, B, 0.8, rec.data_ptr(), 100, nrec.data_ptr())
            for _ in range(2):
                run()
            det.sync()
            times = []
            for _ in range(3):
                t0 = time.perf_counter()
                for _ in range(a.iters):
                    run()
                det.sync()
                times.append((time.perf_counter() - t0) / a.iters)
            t = float(np.median(times))
            det.profile(True)
            run()
            lt = det.layer_times()
            det.profile(False)
            conv_ms = sum(lt[1 + i] for i in conv_idx)
            fwd_ms = float(lt[:-1].sum())
            res["batches"][str(B)] = {
                "ms_per_call": t * 1e3, "images_per_s_whole_call": B / t,
                "profiled_forward_ms": fwd_ms, "profiled_decode_nms_ms": float(lt[-1]),
                "images_per_s_forward_only": B / (fwd_ms / 1e3),
                "conv_ms": float(conv_ms), "conv_tflops": float(fl * B / (conv_ms * 1e-3) / 1e12) if conv_ms > 0 else None,
                "conv_pct_of_f32_peak": float(100 * fl * B / (conv_ms * 1e-3) / 1e12 / PEAK_TF) if conv_ms > 0 else None,
                "slowest_layers_ms": sorted(((float(lt[1 + i]), i, ref_names[i]) for i in range(len(net["layers"]))), reverse=True)[:5],
            }
            if B == max(batches):
                res["layer_ms_at_max_batch"] = [float(x) for x in lt]
            print(name, B, {k: v for k, v in res["batches"][str(B)].items() if k != "slowest_layers_ms"}, file=sys.stderr, flush=True)
        det.close()
        out["nets"][name] = res
    out["detect_track"] = detect_track(pkg, tmp, a.iters)
    print("detect_track", out["detect_track"], file=sys.stderr, flush=True)
    print(json.dumps(out))


def detect_track(pkg, tmp, iters, B=32):
    """frames/s of svo_det_batch_dev(consumer = ctx) -> svo_track_batch_bgr_dev against svo_track_batch_bgr_dev alone, on the
    synthetic sequence's frames (BGR), the yolov3-tiny-shaped test network at its own size, threshold 0.8."""
    import importlib
    import torch
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    L, R, _ = synth.render_sequence(B)
    L, R = L.numpy(), R.numpy()
    H, W = L.shape[1:]
    col = lambda a: np.stack([np.stack([x, np.clip(x.astype(np.int32) + 9, 0, 255).astype(np.uint8), x], axis=2) for x in a])
    dL, dR = torch.from_numpy(col(L)).cuda(), torch.from_numpy(col(R)).cuda()
    cfg = os.path.join(ROOT, "tests", "golden", "tiny_yolo3_small.cfg")
    net = ref.parse_cfg(cfg)
    w = os.path.join(tmp, "tiny_yolo3.weights")
    ref.write_weights(w, ref.seeded_params(net, 5, obj_bias=2.5, cls_bias=2.5))
    det = pkg.Detector(cfg, w, max_batch=B)
    ctx = pkg.Svo(W, H, max_batch=B)
    cam = pkg.Camera(**pkg.KITTI_00_02)
    drec = torch.zeros(B * 64 * 6, dtype=torch.float32, device="cuda")
    dn = torch.zeros(B, dtype=torch.int32, device="cuda")
    bx = torch.zeros((B, 64, 4), dtype=torch.int32, device="cuda")
    bn = torch.zeros(B, dtype=torch.int32, device="cuda")
    out = torch.zeros(B * pkg.TRACK_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    bd = pkg.boxes_dev(bx.data_ptr(), bn.data_ptr(), 64)
    torch.cuda.synchronize()
    rates = {}
    for mode in ("track_only", "detect_track"):
        best = 0.0
        for rep in range(3):
            ctx.track_reset(cam)
            t0 = time.perf_counter()
            for _ in range(iters):
                if mode == "detect_track":
                    det.batch_dev(dL.data_ptr(), W, H, 3, 3 * W, B, 0.8, drec.data_ptr(), 64, dn.data_ptr(), boxes=bd, consumer=ctx)
                ctx.track_batch_bgr_dev(dL.data_ptr(), dR.data_ptr(), 3 * W, B, out.data_ptr(), boxes=bd if mode == "detect_track" else None)
            ctx.sync()
            best = max(best, B * iters / (time.perf_counter() - t0))
        rates[mode + "_frames_per_s"] = best
    rates["boxes_per_frame"] = float(bn.float().mean().item())
    rates["note"] = "the same %d frames re-tracked %d times per repeat (a fresh sequence per repeat); best of 3" % (B, iters)
    det.close()
    ctx.close()
    return rates


if __name__ == "__main__":
    main()
