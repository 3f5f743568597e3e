#!/usr/bin/env python3
"""ba_bench.py - what the windowed bundle adjustment (svo_ba_*) costs and what it does to the poses, in one session on one GPU.

256 synthetic frames (bench.py's, gray, depth_source 0) tracked once by svo_track_batch_dev with svo_track_map_out; then
  window_host     one window of 8 frames, host to host (svo_ba_window: upload, two launches, download)
  windows_dev     windows of 8 at step 4 over the resident frames in one svo_ba_windows_dev call (63 windows), to svo_ba_sync
  tracker         svo_track_batch_dev with svo_track_map_out alone
  tracker_ba      the same followed at once by svo_ba_windows_dev(producer = ctx), to the later of the two syncs
Medians of --reps runs after one warm-up, with spreads (max - min).  Per window, the error of the last frame's pose relative to the
first against the synthetic ground truth (translation of inv(T_rel_gt) T_rel), before (the tracker's poses) and after: mean and
worst over the windows.  Prints one JSON line."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--step", type=int, default=4)
    args = ap.parse_args()
    import torch
    import bench
    import svo_loader
    pkg = svo_loader.load()
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    dev = torch.device("cuda", 0)
    n, W, H, P, K, Wn = args.frames, bench.W, bench.H, bench.PITCH, 500, args.window
    gL, gR, T_gt = bench.render_frames(synth, n, dev, synth.BASE_SEED)
    T_gt = T_gt.cpu().numpy().astype(np.float64).reshape(n, 4, 4)
    cam = pkg.Camera(**pkg.KITTI_00_02)
    bx, keep = bench.boxes_hbm(pkg, n, dev)
    rec = pkg.TRACK_DTYPE.itemsize
    res = torch.zeros((n, rec), dtype=torch.uint8, device=dev)
    obs = torch.zeros((n, K, 32), dtype=torch.uint8, device=dev)
    counts = torch.zeros(n, dtype=torch.int32, device=dev)
    nw = (n - Wn) // args.step + 1
    oT = torch.zeros((nw, Wn, 16), dtype=torch.float64, device=dev)
    oP = torch.zeros((nw * (Wn * K // 2) * 32,), dtype=torch.uint8, device=dev)
    oS = torch.zeros((nw * 48,), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    svo = pkg.Svo(W, H, max_batch=n)
    ba = pkg.BundleAdjuster(K, nw)
    par = pkg.BaParams.default(window=Wn)
    ba.stream

    def track(adjust):
        svo.track_reset(cam)
        svo.sync()
        t0 = time.perf_counter()
        svo.track_map_out(obs.data_ptr(), counts.data_ptr())
        svo.track_batch_dev(gL.data_ptr(), gR.data_ptr(), P, n, res.data_ptr(), boxes=bx)
        if adjust:
            ba.windows_dev(cam, par, obs, counts, K, res, rec, 0, nw, args.step, oT, oP, oS, producer=svo)
            ba.sync()
        svo.sync()
        return (time.perf_counter() - t0) * 1e3

    def timed(fn):
        v = [fn() for _ in range(args.reps + 1)][1:]
        return {"median": float(np.median(v)), "spread": float(max(v) - min(v))}

    t_tracker = timed(lambda: track(False))
    t_both = timed(lambda: track(True))
    t_tracker_again = timed(lambda: track(False))
    h_res = res.cpu().numpy().reshape(-1).view(pkg.TRACK_DTYPE)
    h_obs = obs.cpu().numpy().reshape(n, K * 32).view(pkg.MAP_OBS_DTYPE).reshape(n, K)
    h_counts = counts.cpu().numpy()

    def windows():
        t0 = time.perf_counter()
        ba.windows_dev(cam, par, obs, counts, K, res, rec, 0, nw, args.step, oT, oP, oS)
        ba.sync()
        return (time.perf_counter() - t0) * 1e3
    t_windows = timed(windows)
    f0 = (n // 2 // args.step) * args.step
    Tin = h_res["Tcw"][f0:f0 + Wn].reshape(Wn, 4, 4)

    def one():
        t0 = time.perf_counter()
        one.out = ba.window(cam, par, h_obs[f0:f0 + Wn], h_counts[f0:f0 + Wn], Tin)
        return (time.perf_counter() - t0) * 1e3
    t_one = timed(one)
    T = oT.cpu().numpy().reshape(nw, Wn, 4, 4)
    st = oS.cpu().numpy().view(pkg.BA_STATS_DTYPE)
    same = bool(np.array_equal(one.out[0], T[f0 // args.step]))

    def rel_err(Tf, Tl, g0, g1):
        rel = Tl @ np.linalg.inv(Tf)
        gt = np.linalg.inv(g1) @ g0          # T_cw(last) T_wc(first)
        return float(np.linalg.norm((np.linalg.inv(gt) @ rel)[:3, 3]))
    before, after = [], []
    for w in range(nw):
        a = w * args.step
        tr = h_res["Tcw"][a:a + Wn].reshape(Wn, 4, 4).astype(np.float64)
        before.append(rel_err(tr[0], tr[-1], T_gt[a], T_gt[a + Wn - 1]))
        after.append(rel_err(T[w, 0], T[w, -1], T_gt[a], T_gt[a + Wn - 1]))
    ba.close()
    svo.close()
    out = {
        "tool": "ba_bench", "frames": n, "reps": args.reps, "window": Wn, "step": args.step, "windows": nw,
        "ms": {"window_host": t_one, "windows_dev": t_windows, "tracker": t_tracker, "tracker_ba": t_both, "tracker_again": t_tracker_again},
        "us_per_window_dev": t_windows["median"] * 1e3 / nw,
        "ratio_tracker_ba_over_tracker": t_both["median"] / t_tracker["median"],
        "per_window": {"points_mean": float(st["n_points"].mean()), "edges_mean": float(st["n_edges"].mean()),
                       "iterations_mean": float(st["iterations"].mean()), "trials_mean": float(st["trials_total"].mean()),
                       "status_ok": int((st["status"] == 0).sum())},
        "relative_pose_error_m": {"before_mean": float(np.mean(before)), "before_worst": float(np.max(before)),
                                  "after_mean": float(np.mean(after)), "after_worst": float(np.max(after))},
        "host_window_equals_its_window_of_the_call": same,
    }
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
