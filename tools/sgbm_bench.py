"""Semi-global block matching on one MI355X: latency of one pair host to host (svo_sgbm_process), pairs/s of
svo_sgbm_batch_dev over 64 resident pairs, frames/s of svo_track_batch_dev at depth_source 3 over 256 frames.  Every figure is
the median of --repeats timed runs after a warm-up, with the spread (min .. max) beside it.  Prints one JSON line.
--bgr: the same three figures for the cn = 3 solver on 8UC3 pairs (svo_sgbm_process_bgr, svo_sgbm_batch_bgr_dev,
svo_track_batch_bgr_dev with "sgbm_colour" 1).  --both: gray and colour in one session, and the colour / gray ratios of the
medians (time per pair or frame: above 1 means colour is slower).
--mode hh: the figures of the eight-direction mode (svo_sgbm_*_mode with SVO_SGBM_MODE_HH, "sgbm_mode" 1 in the tracker).
--modes: MODE_SGBM and MODE_HH in one session, and the hh / sgbm ratios of the medians (time: above 1 means hh is slower); with
--bgr for the colour solver.
Usage: python tools/sgbm_bench.py [--repeats N] [--only latency|batch|track] [--bgr | --both] [--mode sgbm|hh | --modes]"""
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
ap.add_argument("--bgr", action="store_true", help="the cn = 3 solver on 8UC3 pairs")
ap.add_argument("--both", action="store_true", help="gray and colour in one session, and their ratios")
ap.add_argument("--mode", choices=["sgbm", "hh"], default="sgbm", help="five directions in one pass, or all eight in two")
ap.add_argument("--modes", action="store_true", help="both modes in one session, and their ratios")
a = ap.parse_args()
if a.modes and a.both:
    ap.error("--modes and --both: one comparison per session")
svo = svo_loader.load()
dev = torch.device("cuda", 0)


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


def colourise(g):
    """(..., H, W) gray -> (..., H, W, 3): three channels that are no copies of each other (torch or numpy).  The complement
    goes into B, which BGR2GRAY weighs least: the gray the tracker makes keeps 0.75 of the texture (in G it would cancel it)."""
    if isinstance(g, np.ndarray):
        g = g.astype(np.int32)
        return np.stack([128 + (128 - g) // 2, g, np.clip(3 * g // 4 + 32, 0, 255)], -1).astype(np.uint8)
    g = g.to(torch.int32)
    return torch.stack([128 + torch.div(128 - g, 2, rounding_mode="floor"), g, torch.clamp(torch.div(3 * g, 4, rounding_mode="floor") + 32, 0, 255)], -1).to(torch.uint8)


def measure(colour, mode=0):
    cn = 3 if colour else 1
    out = {}
    L, R = util.urban_pair()
    H, W = L.shape
    stride = 3840 if colour else 1280
    if colour:
        L, R = colourise(L), colourise(R)
    process = (lambda c: c.sgbm_process_bgr(L, R, mode=mode)) if colour else (lambda c: c.sgbm_process(L, R, mode=mode))
    if a.only in (None, "latency"):
        ctx = svo.Svo(W, H)
        ts = timed(lambda: process(ctx), a.repeats)
        out["one_pair_host_to_host_ms"] = spread([1e3 * t for t in ts], 3)
        ctx.close()
    if a.only in (None, "batch"):
        B = a.batch
        ctx = svo.Svo(W, H)
        dL = torch.zeros((B, H, stride), dtype=torch.uint8, device=dev); dR = torch.zeros_like(dL)
        dL[:, :, :cn * W] = torch.from_numpy(L.reshape(H, cn * W)).to(dev); dR[:, :, :cn * W] = torch.from_numpy(R.reshape(H, cn * W)).to(dev)
        D = torch.zeros((B, H, W), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        entry = ctx.sgbm_batch_bgr_dev if colour else ctx.sgbm_batch_dev
        ts = timed(lambda: entry(dL.data_ptr(), dR.data_ptr(), stride, W, H, B, D.data_ptr(), mode=mode), a.repeats)
        out["batch_%d_pairs_per_s" % B] = spread([B / t for t in ts], 1)
        assert np.array_equal(D[B - 1].cpu().numpy(), process(ctx)[1])
        ctx.close()
    if a.only in (None, "track"):
        N = a.frames
        synth = importlib.import_module("stereo_semantic_vo_amd.synth")
        dL = torch.zeros((N, H, stride), dtype=torch.uint8, device=dev); dR = torch.zeros_like(dL)
        for c0 in range(0, N, 64):
            c = min(64, N - c0)
            Ls, Rs, _ = synth.render_sequence(c, device=dev, start=c0)
            if colour:
                Ls, Rs = colourise(Ls).reshape(c, H, 3 * W), colourise(Rs).reshape(c, H, 3 * W)
            dL[c0:c0 + c, :, :cn * W] = Ls; dR[c0:c0 + c, :, :cn * W] = Rs
        res = torch.zeros((N, svo.TRACK_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        ctx = svo.Svo(W, H, max_batch=N)
        ctx.set_option("depth_source", 3)
        ctx.set_option("sgbm_colour", 1 if colour else 0)
        ctx.set_option("sgbm_mode", mode)
        cam = svo.Camera(**svo.KITTI_00_02)
        torch.cuda.synchronize()
        entry = ctx.track_batch_bgr_dev if colour else ctx.track_batch_dev

        def run():
            ctx.track_reset(cam)
            entry(dL.data_ptr(), dR.data_ptr(), stride, N, res.data_ptr())
            ctx.sync()

        ts = timed(run, a.repeats)
        out["track_%d_frames_per_s" % N] = spread([N / t for t in ts], 1)
        rec = res.cpu().numpy().view(svo.TRACK_DTYPE).reshape(-1)
        out["track_last_frame"] = {"n_stereo": int(rec[-1]["n_stereo"]), "n_lm_edges": int(rec[-1]["n_lm_edges"])}
        assert ctx.track_overflowed() == 0
        ctx.close()
    return out


def time_ratios(base, other):
    """other / base of the medians, as times per pair or frame."""
    ratios = {}
    for k, g in base.items():
        if k == "track_last_frame":
            continue
        b = other[k]["median"]
        ratios[k.replace("_ms", "").replace("_per_s", "") + "_time"] = round(b / g["median"] if k.endswith("_ms") else g["median"] / b, 3)
    return ratios


MODE = 1 if a.mode == "hh" else 0
what = "semi-global block matching, 1241x376, D = 48"
if a.both:
    out = {"workload": what + ", gray (cn = 1) and 8UC3 (cn = 3)" + (", MODE_HH" if MODE else ""), "repeats": a.repeats,
           "gray": measure(False, MODE), "bgr": measure(True, MODE)}
    out["bgr_over_gray"] = time_ratios(out["gray"], out["bgr"])
elif a.modes:
    out = {"workload": what + (", 8UC3 (cn = 3)" if a.bgr else "") + ", MODE_SGBM (5 directions) and MODE_HH (8 directions)",
           "repeats": a.repeats, "sgbm": measure(a.bgr, 0), "hh": measure(a.bgr, 1)}
    out["hh_over_sgbm"] = time_ratios(out["sgbm"], out["hh"])
else:
    out = {"workload": what + (", 8UC3 (cn = 3)" if a.bgr else "") + (", MODE_HH" if MODE else ""), "repeats": a.repeats}
    out.update(measure(a.bgr, MODE))
print(json.dumps(out))
