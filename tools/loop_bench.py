#!/usr/bin/env python3
"""loop_bench.py - what loop verification (svo_loop_*) costs, in one session on one GPU.  First figures: nothing is gated on them.

  verify_host      one pair of 500-keypoint frames host to host (svo_loop_verify: uploads, two launches, downloads)
  match_dev        256 x 4 = 1024 candidate pairs of resident frames in one svo_loop_match_dev call, to svo_loop_sync:
                   500 keypoints over 100 nodes (what levelsup 2 .. 4 of a real tree gives), and the same frames with ONE node
                   holding every feature (the root: levelsup 4 on an L = 4 tree)
  solve_dev        the same 1024 pairs through svo_loop_solve_dev from the matches
  tracker          svo_track_batch_dev alone over 256 synthetic frames (bench.py's)
  tracker_loop     svo_frontend_batch_dev + svo_track_tail_dev with svo_track_map_out armed + svo_bow_transform_dev +
                   svo_bow_query_dev (every frame a query, gap 10, top_k 4) + svo_loop_pairs_dev + svo_loop_verify_dev through
                   svo_loop_wait, to the last sync; alternating with `tracker`
and the matches, inliers and status counts of those 1024 pairs (a straight drive: a candidate 10 frames back shares little).
The planted frames are tests/loop_cases.py's: copies of one another with up to 24 flipped bits, 80 % of the keypoints with a
map point, one rigid motion.  Medians of --reps runs after one warm-up, with spreads (max - min).  Prints one JSON line and
writes it to --out."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_loop_bench.json"))
    args = ap.parse_args()
    import torch
    import bench
    import bow_ref
    import loop_cases as Cs
    import loop_ref as R
    import svo_loader
    pkg = svo_loader.load()
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    dev = torch.device("cuda", 0)
    K, TOP = 500, 4

    def timed(fn):
        v = [fn() for _ in range(args.reps + 1)][1:]
        return {"median": float(np.median(v)), "spread": float(max(v) - min(v))}

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)

    # ---- planted pairs -------------------------------------------------------------------------------------------------------------
    n_pairs = 1024
    cam = pkg.Camera(bf=0.0, **Cs.CAM)
    P = pkg.LoopParams.default()
    ver = pkg.LoopVerifier(max_kp=K, max_pairs=n_pairs)
    out_ms, stats = {}, {}
    for name, sizes in (("nodes100", [(5, 5)] * 100), ("root", [(500, 500)])):
        c = Cs.planted(60, sizes=sizes, S=K, n_pairs=16, pad=0)
        sc = c["scene"]
        if name == "root":
            sc["fv"]["node"] = 0
        d = {k: up(a) for k, a in sc.items()}
        pairs = np.array([(2 * (p % 16), 2 * (p % 16) + 1) for p in range(n_pairs)], np.int32)
        d_pairs = up(pairs)
        match = torch.zeros((n_pairs, K), dtype=torch.int32, device=dev)
        match_n = torch.zeros(n_pairs, dtype=torch.int32, device=dev)
        res = torch.zeros(n_pairs * pkg.LOOP_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        inl = torch.zeros((n_pairs, K), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

        def match_dev():
            t0 = time.perf_counter()
            ver.match_dev(P, d["desc"], d["kp"], d["n"], K, d["fv"], d["fv_n"], d["obs"], d["obs_n"], K, d_pairs, n_pairs, match, match_n)
            ver.sync()
            return (time.perf_counter() - t0) * 1e3

        def solve_dev():
            t0 = time.perf_counter()
            ver.solve_dev(cam, P, d["kp"], d["obs"], d["obs_n"], K, d["Tcw"], 64, d_pairs, n_pairs, match, K, res, inl)
            ver.sync()
            return (time.perf_counter() - t0) * 1e3

        out_ms["match_dev_" + name] = timed(match_dev)
        out_ms["solve_dev_" + name] = timed(solve_dev)
        h = res.cpu().numpy().view(pkg.LOOP_RESULT_DTYPE)
        stats[name] = {"matches_mean": float(match_n.cpu().numpy().mean()), "inliers_mean": float(h["n_inliers"].mean()),
                       "visited_mean": float(h["visited"].mean()), "status_counts": np.bincount(h["status"], minlength=4).tolist()}
        if name == "nodes100":
            f = [0, 1]

            def verify_host():
                t0 = time.perf_counter()
                ver.verify(cam, P, sc["desc"][f], sc["kp"][f], sc["n"][f], sc["fv"][f], sc["fv_n"][f], sc["obs"][f], sc["obs_n"][f],
                           sc["Tcw"][f])
                return (time.perf_counter() - t0) * 1e3
            out_ms["verify_host"] = timed(verify_host)
    ver.close()

    # ---- behind the tracker ------------------------------------------------------------------------------------------------------
    n, W, H, PITCH = args.frames, bench.W, bench.H, bench.PITCH
    gL, gR, _ = bench.render_frames(synth, n, dev, synth.BASE_SEED)
    kcam = pkg.Camera(**pkg.KITTI_00_02)
    bx, _ = bench.boxes_hbm(pkg, n, dev)
    rec = pkg.TRACK_DTYPE.itemsize
    v = bow_ref.random_tree(7, 10, 4, stop=0.02)
    voc = pkg.Vocabulary.from_arrays(v.k, v.L, v.weighting, v.parent, v.desc, v.weight, max_kp=K, max_frames=n)
    n_pairs = n * TOP
    ver = pkg.LoopVerifier(max_kp=K, max_pairs=n_pairs)
    voc.stream, ver.stream
    svo = pkg.Svo(W, H, max_batch=n)

    def z(shape, dt=torch.uint8):
        return torch.zeros(shape, dtype=dt, device=dev)
    tres, kp, desc, fn = z((n, rec)), z((n, K, 28)), z((n, K, 32)), z((n,), torch.int32)
    depth, obs, obs_n = z((n, K), torch.float32), z((n, K, 32)), z((n,), torch.int32)
    vec, vec_n, fv, fv_n = z((n, K, 16)), z((n,), torch.int32), z((n, K, 8)), z((n,), torch.int32)
    cand, cand_n, pairs = z((n, TOP, 16)), z((n,), torch.int32), z((n_pairs, 2), torch.int32)
    match, match_n = z((n_pairs, K), torch.int32), z((n_pairs,), torch.int32)
    res, inl = z(n_pairs * pkg.LOOP_RESULT_DTYPE.itemsize), z((n_pairs, K))
    torch.cuda.synchronize()

    def tracker():
        svo.track_reset(kcam)
        svo.sync()
        t0 = time.perf_counter()
        svo.track_batch_dev(gL.data_ptr(), gR.data_ptr(), PITCH, n, tres.data_ptr(), boxes=bx)
        svo.sync()
        return (time.perf_counter() - t0) * 1e3

    def tracker_loop():
        svo.track_reset(kcam)
        svo.sync()
        t0 = time.perf_counter()
        svo.frontend_batch_dev(gL.data_ptr(), gR.data_ptr(), PITCH, n, kcam, kp.data_ptr(), desc.data_ptr(), fn.data_ptr(), None,
                               depth.data_ptr())
        voc.transform_dev(desc, fn, K, n, 2, None, vec, vec_n, fv, fv_n, producer=svo)      # (behind the front end, beside the tail)
        voc.query_dev(vec, vec_n, K, n, 0, n, 10, 0.0, TOP, cand, cand_n)
        svo.track_map_out(obs.data_ptr(), obs_n.data_ptr())
        svo.track_tail_dev(kp.data_ptr(), desc.data_ptr(), fn.data_ptr(), depth.data_ptr(), K, n, tres.data_ptr(), boxes=bx)
        ver.wait(voc.stream)
        ver.wait(svo.stream)
        ver.pairs_dev(cand, cand_n, 0, n, TOP, pairs)
        ver.verify_dev(kcam, P, desc, kp, fn, K, fv, fv_n, obs, obs_n, K, tres, rec, pairs, n_pairs, match, match_n, res, inl)
        ver.sync()
        voc.sync()
        svo.sync()
        return (time.perf_counter() - t0) * 1e3

    a, b = [], []
    for _ in range(args.reps + 1):
        a.append(tracker())
        b.append(tracker_loop())
    out_ms["tracker"] = {"median": float(np.median(a[1:])), "spread": float(max(a[1:]) - min(a[1:]))}
    out_ms["tracker_loop"] = {"median": float(np.median(b[1:])), "spread": float(max(b[1:]) - min(b[1:]))}
    h = res.cpu().numpy().view(pkg.LOOP_RESULT_DTYPE)
    hp = pairs.cpu().numpy()
    real = hp[:, 0] >= 0
    stats["revisit"] = {"pairs": int(real.sum()), "matches_mean": float(match_n.cpu().numpy()[real].mean()) if real.any() else 0.0,
                        "inliers_mean": float(h["n_inliers"][real].mean()) if real.any() else 0.0,
                        "status_counts": np.bincount(h["status"], minlength=4).tolist(),
                        "status_names": ["OK", "FEW", "REJECTED", "SKIPPED"], "th_low": 50, "nn_ratio": 0.75}
    svo.close()
    ver.close()
    voc.close()
    out = {"tool": "loop_bench", "frames": n, "reps": args.reps, "pairs_a_call": 1024, "keypoints": K, "ms": out_ms, "pairs": stats,
           "us_per_pair": {k: out_ms[k]["median"] * 1e3 / 1024 for k in out_ms if k.startswith(("match_dev", "solve_dev"))},
           "ratio_tracker_loop_over_tracker": out_ms["tracker_loop"]["median"] / out_ms["tracker"]["median"]}
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
