#!/usr/bin/env python3
"""map_bench.py - what svo_track_map_out (each tracked frame's map points and observations) costs, in one session on one GPU.

256 synthetic frames with bench.py's moving boxes, resident in HBM, gray, depth_source 0, one svo_track_batch_dev call per
measurement:
  off        the call without the attachment
  on         the same call armed (svo_track_map_out before every call), records left in HBM
  off_again  off once more, after on: the drift of the session
Medians of --reps runs after one warm-up, us per frame, and the ratio on / off; --dynamic: the same three with the
dynamic-keypoint loop on (its lists attached in all three).  The result records with the attachment must equal those without,
and the counts must equal matched + created of the run's debug records.  Prints one JSON line."""
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
    ap.add_argument("--dynamic", action="store_true", help="with the dynamic-keypoint loop on (svo_track_dynamic)")
    args = ap.parse_args()
    import torch
    import bench
    import svo_loader
    pkg = svo_loader.load()
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    dev = torch.device("cuda", 0)
    n, W, H, P, K = args.frames, bench.W, bench.H, bench.PITCH, 500
    gL, gR, _ = bench.render_frames(synth, n, dev, synth.BASE_SEED)
    cam = pkg.Camera(**pkg.KITTI_00_02)
    bx, keep = bench.boxes_hbm(pkg, n, dev)
    rec = pkg.TRACK_DTYPE.itemsize
    res = torch.zeros((n, rec), dtype=torch.uint8, device=dev)
    obs = torch.zeros((n, K, 32), dtype=torch.uint8, device=dev); counts = torch.zeros(n, dtype=torch.int32, device=dev)
    lists = torch.zeros((n, 512, 2), dtype=torch.float32, device=dev)
    dcounts = torch.zeros(n, dtype=torch.int32, device=dev); dropped = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    svo = pkg.Svo(W, H, max_batch=n)
    if args.dynamic:
        p = pkg.dyn_default_params()
        p.enable, p.max_pts = 1, 512
        svo.track_dynamic(p)

    def tracker(on):
        times = []
        for r in range(args.reps + 1):
            svo.track_reset(cam)
            svo.sync()
            t0 = time.perf_counter()
            if on:
                svo.track_map_out(obs.data_ptr(), counts.data_ptr())
            if args.dynamic:
                svo.track_dynamic_out(lists.data_ptr(), dcounts.data_ptr(), dropped.data_ptr())
            svo.track_batch_dev(gL.data_ptr(), gR.data_ptr(), P, n, res.data_ptr(), boxes=bx)
            svo.sync()
            times.append((time.perf_counter() - t0) * 1e6 / n)
        return times[1:], res.cpu().numpy().tobytes()

    t_off, rec_off = tracker(False)
    t_on, rec_on = tracker(True)
    dbg = svo.debug_track_frames(0, n)
    c = counts.cpu().numpy()
    nkp = np.frombuffer(rec_on, pkg.TRACK_DTYPE)["n_kp"]
    want = np.array([(dbg[k]["match_gid"][:nkp[k]] >= 0).sum() + (dbg[k]["new_gid"][:nkp[k]] >= 0).sum() for k in range(n)])
    o = obs.cpu().numpy().reshape(n, K * 32)
    new = sum(int((o[k, :c[k] * 32].view(pkg.MAP_OBS_DTYPE)["flags"] & pkg.MAP_NEW).sum()) for k in range(n))
    t_off2, _ = tracker(False)
    svo.close()
    med = lambda v: float(np.median(v))
    spread = lambda v: float(max(v) - min(v))
    off, on = med(t_off), med(t_on)
    ok = rec_on == rec_off and bool(np.array_equal(c, want))
    out = {
        "tool": "map_bench", "frames": n, "reps": args.reps, "dynamic_loop": bool(args.dynamic),
        "us_per_frame": {"off": off, "on": on, "off_again": med(t_off2)},
        "spread_us": {"off": spread(t_off), "on": spread(t_on), "off_again": spread(t_off2)},
        "frames_per_s": {"off": 1e6 / off, "on": 1e6 / on},
        "ratio_on_off": on / off,
        "records_per_frame": float(c.mean()), "new_points": new, "bytes_per_frame": float(c.mean()) * 32,
        "records_identical_on_off": rec_on == rec_off, "counts_equal_debug_records": bool(np.array_equal(c, want)),
    }
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
