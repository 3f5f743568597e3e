#!/usr/bin/env python3
"""dyn_bench.py - what the dynamic-keypoint loop inside the tracker (svo_track_dynamic) costs, in one session on one GPU.

256 synthetic frames with bench.py's moving boxes, resident in HBM, one call per measurement:
  off      svo_track_batch_dev (--bgr: svo_track_batch_bgr_dev) with the loop off
  on       the same call with the loop on, lists left in HBM
  chain    svo_lk_chain_dev (--bgr: svo_lk_chain_bgr_dev) alone on the same left frames, with the seeds the run produced
           (restated on the host from the front end's keypoints and the run's debug records; its lists must equal the run's)
  host     the frame-by-frame path: svo_track_frame + svo_lk_track host to host, erase and append on the host (32 frames, once)
Medians of --reps runs after one warm-up; prints one JSON line.  The yardstick: on <= off + chain (the parent's way to the same
output on resident frames), margin = the larger of the two components' min..max spreads.

--sequences S [--steps T] [--bgr] [--pipeline 0|1]: the many-sequence mode instead - S staggered sequences (sequence q walks
frames q, q + 1, ... with that frame's moving boxes) advanced by svo_track_multi_step_dev (--bgr: svo_track_multi_step_bgr_dev),
T steps per run; per STEP the median time with the loop off, on (lists left in HBM, attached at every step), and off again, in
one session; the records with the loop on must equal those with it off."""
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


def many(args):
    import torch
    import bench
    import svo_loader
    pkg = svo_loader.load()
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    dev = torch.device("cuda", 0)
    S, T, W, H, P, mp = args.sequences, args.steps, bench.W, bench.H, bench.PITCH, args.max_pts
    n = S + T
    gL, gR, _ = bench.render_frames(synth, n, dev, synth.BASE_SEED)
    cam = pkg.Camera(**pkg.KITTI_00_02)
    _, (tb, tn) = bench.boxes_hbm(pkg, n, dev)   # frame k's boxes: sequence q's at step t are frame t + q's
    if args.bgr:   # B = R = the gray, G a little brighter: rows 3 W bytes apart
        def colour(g):
            c = torch.stack([g[:, :, :W], torch.clamp(g[:, :, :W].to(torch.int32) + 9, 0, 255).to(torch.uint8), g[:, :, :W]], dim=3)
            return c.reshape(n, H, 3 * W).contiguous()
        dL, dR, pitch = colour(gL), colour(gR), 3 * W
    else:
        dL, dR, pitch = gL, gR, P
    rec = pkg.TRACK_DTYPE.itemsize
    res = torch.zeros((T, S, rec), dtype=torch.uint8, device=dev)
    lists = torch.zeros((T, S, mp, 2), dtype=torch.float32, device=dev)
    counts = torch.zeros((T, S), dtype=torch.int32, device=dev); dropped = torch.zeros((T, S), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    svo = pkg.Svo(W, H, max_batch=S)
    svo.set_option("multi_pipeline", args.pipeline)
    entry = svo.track_multi_step_bgr_dev if args.bgr else svo.track_multi_step_dev

    def run(on):
        p = pkg.dyn_default_params()
        p.enable, p.colour, p.seed_frames, p.max_pts = int(on), int(args.bgr), args.seed_frames, mp
        svo.track_dynamic(p)
        times = []
        for r in range(args.reps + 1):
            svo.track_multi_reset(S, cam)
            svo.sync()
            t0 = time.perf_counter()
            for t in range(T):
                if on:
                    svo.track_dynamic_out(lists[t].data_ptr(), counts[t].data_ptr(), dropped[t].data_ptr())
                entry(dL.data_ptr() + t * H * pitch, dR.data_ptr() + t * H * pitch, pitch, S, res[t].data_ptr(),
                      boxes=pkg.boxes_dev(tb.data_ptr() + t * 2 * 16, tn.data_ptr() + t * 4, 2))
            svo.sync()
            times.append((time.perf_counter() - t0) * 1e6 / T)
        return times[1:], res.cpu().numpy().tobytes()

    t_off, rec_off = run(False)
    t_on, rec_on = run(True)
    c, d = counts.cpu().numpy(), dropped.cpu().numpy()
    t_off2, _ = run(False)   # (off once more, after on: drift of the session)
    svo.close()
    med = lambda v: float(np.median(v))
    spread = lambda v: float(max(v) - min(v))
    off, on = med(t_off), med(t_on)
    out = {
        "tool": "dyn_bench", "mode": "many sequences", "sequences": S, "steps": T, "reps": args.reps, "bgr": bool(args.bgr),
        "multi_pipeline": args.pipeline, "seed_frames": args.seed_frames, "max_pts": mp,
        "us_per_step": {"off": off, "on": on, "off_again": med(t_off2)},
        "spread_us": {"off": spread(t_off), "on": spread(t_on), "off_again": spread(t_off2)},
        "us_per_frame": {"off": off / S, "on": on / S},
        "frames_per_s": {"off": 1e6 * S / off, "on": 1e6 * S / on},
        "ratio_on_off": on / off,
        "mean_list_length": float(c.mean()), "last_step_mean_list_length": float(c[-1].mean()), "seeds_dropped": int(d.sum()),
        "records_identical_on_off": rec_on == rec_off,
    }
    print(json.dumps(out))
    return 0 if rec_on == rec_off else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--bgr", action="store_true")
    ap.add_argument("--seed-frames", type=int, default=2)
    ap.add_argument("--max-pts", type=int, default=512)
    ap.add_argument("--host-frames", type=int, default=32)
    ap.add_argument("--sequences", type=int, default=0, help="many-sequence mode: S sequences advanced together")
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--pipeline", type=int, default=1, help="many-sequence mode: the multi_pipeline option")
    args = ap.parse_args()
    if args.sequences > 0:
        return many(args)
    import torch
    import bench
    import dyn_ref
    import svo_loader
    pkg = svo_loader.load()
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    dev = torch.device("cuda", 0)
    n, W, H, P, mp = args.frames, bench.W, bench.H, bench.PITCH, args.max_pts
    gL, gR, _ = bench.render_frames(synth, n, dev, synth.BASE_SEED)
    cam = pkg.Camera(**pkg.KITTI_00_02)
    bx, keep = bench.boxes_hbm(pkg, n, dev)
    boxes_of = lambda k: np.array(bench.moving_boxes(k), np.int32)
    cn = 3 if args.bgr else 1
    if args.bgr:   # B = R = the gray, G a little brighter: rows 3 W bytes apart
        def colour(g):
            c = torch.stack([g[:, :, :W], torch.clamp(g[:, :, :W].to(torch.int32) + 9, 0, 255).to(torch.uint8), g[:, :, :W]], dim=3)
            return c.reshape(n, H, 3 * W).contiguous()
        dL, dR, pitch = colour(gL), colour(gR), 3 * W
    else:
        dL, dR, pitch = gL, gR, P
    rec = pkg.TRACK_DTYPE.itemsize
    res = torch.zeros((n, rec), dtype=torch.uint8, device=dev)
    lists = torch.zeros((n, mp, 2), dtype=torch.float32, device=dev)
    counts = torch.zeros(n, dtype=torch.int32, device=dev); dropped = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    svo = pkg.Svo(W, H, max_batch=n)
    entry = svo.track_batch_bgr_dev if args.bgr else svo.track_batch_dev

    def tracker(on):
        p = pkg.dyn_default_params()
        p.enable, p.colour, p.seed_frames, p.max_pts = int(on), int(args.bgr), args.seed_frames, mp
        svo.track_dynamic(p)
        times = []
        for r in range(args.reps + 1):
            svo.track_reset(cam)
            svo.sync()
            t0 = time.perf_counter()
            if on:
                svo.track_dynamic_out(lists.data_ptr(), counts.data_ptr(), dropped.data_ptr())
            entry(dL.data_ptr(), dR.data_ptr(), pitch, n, res.data_ptr(), boxes=bx)
            svo.sync()
            times.append((time.perf_counter() - t0) * 1e6 / n)
        return times[1:], res.cpu().numpy().tobytes()

    t_off, rec_off = tracker(False)
    t_on, rec_on = tracker(True)
    has_mp = svo.debug_track_frames(0, n)["match_gid"] >= 0
    run_lists, run_counts, run_dropped = lists.cpu().numpy(), counts.cpu().numpy(), dropped.cpu().numpy()
    t_off2, _ = tracker(False)   # (off once more, after on: drift of the session)
    # the seeds of the run, restated: the front end's keypoints, the run's map-point indices, the boxes
    fe = pkg.Svo(W, H, max_batch=n)
    if args.bgr:
        hL, hR = dL.cpu().numpy().reshape(n, H, W, 3), dR.cpu().numpy().reshape(n, H, W, 3)
        q = torch.zeros((2, n, H, P), dtype=torch.uint8, device=dev)
        for k in range(n):
            q[0, k, :, :W] = torch.from_numpy(fe.bgr_to_gray(hL[k])).to(dev); q[1, k, :, :W] = torch.from_numpy(fe.bgr_to_gray(hR[k])).to(dev)
        fL, fR = q[0], q[1]
    else:
        fL, fR = gL, gR
    kp = torch.zeros((n, 500, pkg.KP_DTYPE.itemsize), dtype=torch.uint8, device=dev); nk = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    fe.frontend_batch_dev(fL.data_ptr(), fR.data_ptr(), P, n, cam, d_kpL=kp.data_ptr(), d_nL=nk.data_ptr())
    fe.sync()
    kph = kp.cpu().numpy().view(pkg.KP_DTYPE).reshape(n, 500); nkh = nk.cpu().numpy()
    S = 1024
    seeds = np.zeros((n, S, 2), np.float32); nseed = np.zeros(n, np.int32)
    for k in range(n):
        xy = np.stack([kph[k, :nkh[k]]["x"], kph[k, :nkh[k]]["y"]], 1).astype(np.float32)
        init, create = dyn_ref.frame_seeds(xy, has_mp[k, :nkh[k]], boxes_of(k), k, args.seed_frames)
        s = np.concatenate([init, create])
        seeds[k, :len(s)] = s; nseed[k] = len(s)
    d_seeds, d_nseed = torch.from_numpy(seeds).to(dev), torch.from_numpy(nseed).to(dev)
    c_lists = torch.zeros_like(lists); c_counts = torch.zeros_like(counts); c_dropped = torch.zeros_like(dropped)
    torch.cuda.synchronize()
    chain = fe.lk_chain_bgr_dev if args.bgr else fe.lk_chain_dev
    t_chain = []
    for r in range(args.reps + 1):
        fe.sync()
        t0 = time.perf_counter()
        chain(dL.data_ptr(), pitch, W, H, n, d_seeds.data_ptr(), d_nseed.data_ptr(), S, mp, c_lists.data_ptr(), c_counts.data_ptr(),
              c_dropped.data_ptr())   # (synchronises)
        t_chain.append((time.perf_counter() - t0) * 1e6 / n)
    t_chain = t_chain[1:]
    cl, cc, cd = c_lists.cpu().numpy(), c_counts.cpu().numpy(), c_dropped.cpu().numpy()
    identical = bool(np.array_equal(cc, run_counts) and np.array_equal(cd, run_dropped) and
                     all(np.array_equal(cl[k, :cc[k]].view(np.uint32), run_lists[k, :cc[k]].view(np.uint32)) for k in range(n)))
    # the frame-by-frame host path, for scale
    m = min(args.host_frames, n)
    hgL, hgR = fL[:m, :, :W].cpu().numpy(), fR[:m, :, :W].cpu().numpy()
    one = pkg.Svo(W, H, max_batch=1)
    one.track_reset(cam)
    cur = np.zeros((0, 2), np.float32)
    t0 = time.perf_counter()
    for k in range(m):
        if len(cur):
            nx, st, _ = one.lk_track_bgr(hL[k - 1], hL[k], cur) if args.bgr else one.lk_track(hgL[k - 1], hgL[k], cur)
            cur = nx[st != 0]
        r = one.track_frame_bgr(hL[k], hR[k], boxes=boxes_of(k)) if args.bgr else one.track_frame(hgL[k], hgR[k], boxes=boxes_of(k))
        one.debug_track_matches()   # (the synchronising probe the host loop needs for its seeds; they are the restated ones)
        cur, _ = dyn_ref.append(cur, seeds[k, :nseed[k]], mp)
    t_host = (time.perf_counter() - t0) * 1e6 / m
    host_identical = bool(len(cur) == run_counts[m - 1] and np.array_equal(cur.view(np.uint32), run_lists[m - 1, :len(cur)].view(np.uint32)))
    one.close(); fe.close(); svo.close()
    med = lambda v: float(np.median(v))
    spread = lambda v: float(max(v) - min(v))
    off, on, ch = med(t_off), med(t_on), med(t_chain)
    out = {
        "tool": "dyn_bench", "frames": n, "reps": args.reps, "bgr": bool(args.bgr), "seed_frames": args.seed_frames, "max_pts": mp,
        "us_per_frame": {"off": off, "on": on, "off_again": med(t_off2), "lk_chain_alone": ch, "off_plus_chain": off + ch,
                         "host_frame_by_frame_once": t_host},
        "spread_us": {"off": spread(t_off), "on": spread(t_on), "off_again": spread(t_off2), "lk_chain_alone": spread(t_chain)},
        "frames_per_s": {"off": 1e6 / off, "on": 1e6 / on},
        "ratio_on_off": on / off,
        "on_within_off_plus_chain": bool(on <= off + ch + max(spread(t_off), spread(t_chain))),
        "mean_list_length": float(run_counts.mean()), "last_list_length": int(run_counts[-1]), "seeds_dropped": int(run_dropped.sum()),
        "records_identical_on_off": rec_on == rec_off,
        "chain_lists_identical": identical, "host_lists_identical": host_identical,
    }
    print(json.dumps(out))
    return 0 if (identical and rec_on == rec_off) else 1


if __name__ == "__main__":
    sys.exit(main())
