"""Semi-global block matching on one MI355X: latency of one pair host to host (svo_sgbm_process), pairs/s of
svo_sgbm_batch_dev over 64 resident pairs, frames/s of svo_track_batch_dev at depth_source 3 over 256 frames.  Every figure is
the median of --repeats timed runs after a warm-up, with the spread (min .. max) beside it.  Prints one JSON line.
Usage: python tools/sgbm_bench.py [--repeats N] [--only latency|batch|track]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import svo_loader  # noqa: E402
import util  # noqa: E402
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--only", choices=["latency", "batch", "track"], default=None)
a = ap.parse_args()
svo = svo_loader.load()
dev = torch.device("cuda", 0)
stride = 1280


def timed(fn, repeats):
    fn()                                         # warm-up: allocations, code objects, clocks
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def spread(vals, digits):
    return {"median": round(statistics.median(vals), digits), "min": round(min(vals), digits), "max": round(max(vals), digits)}


out = {"workload": "semi-global block matching, 1241x376, D = 48", "repeats": a.repeats}
L, R = util.urban_pair()
H, W = L.shape
if a.only in (None, "latency"):
    ctx = svo.Svo(W, H)
    ts = timed(lambda: ctx.sgbm_process(L, R), a.repeats)
    out["one_pair_host_to_host_ms"] = spread([1e3 * t for t in ts], 3)
    ctx.close()
if a.only in (None, "batch"):
    B = a.batch
    ctx = svo.Svo(W, H)
    dL = torch.zeros((B, H, stride), dtype=torch.uint8, device=dev); dR = torch.zeros_like(dL)
    dL[:, :, :W] = torch.from_numpy(L).to(dev); dR[:, :, :W] = torch.from_numpy(R).to(dev)
    D = torch.zeros((B, H, W), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ts = timed(lambda: ctx.sgbm_batch_dev(dL.data_ptr(), dR.data_ptr(), stride, W, H, B, D.data_ptr()), a.repeats)
    out["batch_%d_pairs_per_s" % B] = spread([B / t for t in ts], 1)
    assert np.array_equal(D[B - 1].cpu().numpy(), ctx.sgbm_process(L, R)[1])
    ctx.close()
if a.only in (None, "track"):
    N = a.frames
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    dL = torch.zeros((N, H, stride), dtype=torch.uint8, device=dev); dR = torch.zeros_like(dL)
    for c0 in range(0, N, 64):
        c = min(64, N - c0)
        Ls, Rs, _ = synth.render_sequence(c, device=dev, start=c0)
        dL[c0:c0 + c, :, :W] = Ls; dR[c0:c0 + c, :, :W] = Rs
    res = torch.zeros((N, svo.TRACK_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    ctx = svo.Svo(W, H, max_batch=N)
    ctx.set_option("depth_source", 3)
    cam = svo.Camera(**svo.KITTI_00_02)
    torch.cuda.synchronize()

    def run():
        ctx.track_reset(cam)
        ctx.track_batch_dev(dL.data_ptr(), dR.data_ptr(), stride, N, res.data_ptr())
        ctx.sync()

    ts = timed(run, a.repeats)
    out["track_%d_frames_per_s" % N] = spread([N / t for t in ts], 1)
    rec = res.cpu().numpy().view(svo.TRACK_DTYPE).reshape(-1)
    out["track_last_frame"] = {"n_stereo": int(rec[-1]["n_stereo"]), "n_lm_edges": int(rec[-1]["n_lm_edges"])}
    assert ctx.track_overflowed() == 0
    ctx.close()
print(json.dumps(out))
