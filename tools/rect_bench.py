#!/usr/bin/env python3
"""rect_bench.py - what rectification on the device costs, in one session on one GPU.  Prints one JSON line.

  pair_host      one 752 x 480 gray pair through svo_rect_process, host to host (uploads, kernel, downloads, one synchronisation)
  resident_gray  64 resident 752 x 480 pairs per svo_rect_batch_dev call, gray: pairs/s, and the bytes the call has to move
  resident_bgr   (source pixels read once, destination pixels written, the fixed-point maps read once per RECT_BI = 4 images
                 of a side, 6 bytes a pixel) per second against the 8 TB/s HBM peak
  track          --frames (256) synthetic KITTI-sized frames resident in HBM: svo_rect_batch_dev(consumer) + svo_track_batch_dev
                 with no host call in between, against svo_track_batch_dev alone on the same frames already rectified; the two
                 alternate within one session, medians of --reps (7) after a warm-up, and the ratio with its spread
The records of rectify + track must equal those of track alone on the rectified frames."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MAP_BYTES, BI = 6, 4   # svo_rect.hip: bytes of fixed-point map per destination pixel, images served per read of them


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    import bench
    import svo_loader
    pkg = svo_loader.load()
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    dev = torch.device("cuda", 0)
    med = lambda v: float(np.median(v))
    out = {"tool": "rect_bench", "reps": args.reps, "map_bytes_per_output_pixel": MAP_BYTES, "images_per_map_read": BI}

    # ---- 752 x 480, the EuRoC-like calibration of the tests
    s = pkg.load_rect_settings(os.path.join(ROOT, "tests", "golden", "rect_euroc_like.yaml"))
    w, h = s["src_w"], s["src_h"]
    rect = pkg.Rectifier(w, h, s["left"], s["right"])
    rng = np.random.default_rng(3)
    L, R = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)
    ts = []
    for _ in range(args.reps + 1):
        t0 = time.perf_counter()
        rect.process(L, R)
        ts.append((time.perf_counter() - t0) * 1e6)
    out["pair_host_us"] = {"median": med(ts[1:]), "min": min(ts[1:]), "max": max(ts[1:])}
    B = 64
    for cn, key in ((1, "resident_gray"), (3, "resident_bgr")):
        dL = torch.randint(0, 256, (B, h, cn * w), dtype=torch.uint8, device=dev)
        dR = torch.randint(0, 256, (B, h, cn * w), dtype=torch.uint8, device=dev)
        oL, oR = torch.zeros_like(dL), torch.zeros_like(dR)
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            rect.batch_dev(dL, dR, cn * w, cn, B, oL, oR, cn * w)
            rect.sync()
            ts.append(time.perf_counter() - t0)
        t = med(ts[1:])
        moved = 2 * B * w * h * (2 * cn) + 2 * ((B + BI - 1) // BI) * w * h * MAP_BYTES
        out[key] = {"pairs_per_call": B, "us_per_pair": t * 1e6 / B, "pairs_per_s": B / t, "bytes_moved_per_call": moved,
                    "bytes_per_s": moved / t, "fraction_of_hbm_peak": moved / t / (bench.HBM_PEAK_GBS * 1e9),
                    "spread_us_per_pair": (max(ts[1:]) - min(ts[1:])) * 1e6 / B}
        del dL, dR, oL, oR
    rect.close()

    # ---- rectify + track against track alone, KITTI-sized frames taken as raw, a mild calibration
    n, W, H, P = args.frames, bench.W, bench.H, bench.PITCH
    gL, gR, _ = bench.render_frames(synth, n, dev, synth.BASE_SEED)
    k = pkg.KITTI_00_02
    cam_l = pkg.rect_cam((k["fx"], k["fy"], k["cx"], k["cy"]), (-0.05, 0.01, 0.0005, -0.0003, 0.0), None,
                         (k["fx"] * 0.97, k["fy"] * 0.97, k["cx"], k["cy"]))
    rect = pkg.Rectifier(W, H, cam_l, cam_l)
    cam = rect.camera(k["bf"] * 0.97)
    rL, rR = torch.zeros_like(gL), torch.zeros_like(gR)
    rec = pkg.TRACK_DTYPE.itemsize
    res = torch.zeros((n, rec), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    svo = pkg.Svo(W, H, max_batch=n)

    def run(rectify):
        svo.track_reset(cam)
        svo.sync()
        t0 = time.perf_counter()
        if rectify:
            rect.batch_dev(gL, gR, P, 1, n, rL, rR, P, consumer=svo)
        svo.track_batch_dev(rL.data_ptr(), rR.data_ptr(), P, n, res.data_ptr())
        svo.sync()
        return (time.perf_counter() - t0) * 1e6 / n, res.cpu().numpy().tobytes()

    run(True)
    both, alone, same = [], [], True
    for _ in range(args.reps):   # (alternating: a drift of the session touches both series alike)
        tb, rb = run(True)
        ta, ra = run(False)
        both.append(tb); alone.append(ta)
        same = same and rb == ra
    svo.close(); rect.close()
    ratios = [b / a for b, a in zip(both, alone)]
    out["track"] = {"frames": n, "us_per_frame": {"rectify_and_track": med(both), "track_alone": med(alone)},
                    "spread_us": {"rectify_and_track": max(both) - min(both), "track_alone": max(alone) - min(alone)},
                    "ratio": med(both) / med(alone), "ratio_min": min(ratios), "ratio_max": max(ratios),
                    "records_identical": same}
    print(json.dumps(out))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
