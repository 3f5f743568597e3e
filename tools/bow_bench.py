#!/usr/bin/env python3
"""bow_bench.py - what the bag of words (svo_bow_*) costs, in one session on one GPU.

256 synthetic frames (bench.py's, gray) through the device front end; a vocabulary of k = 10, L = 4 trained from their descriptors
(tools/bow_train.py's procedure, assignment steps on the device) and the training time; then
  transform_host   one frame of 500 descriptors host to host (svo_bow_transform: upload, two launches, download)
  transform_dev    the 256 resident frames in one svo_bow_transform_dev call, to svo_bow_sync (both vocabularies)
  query_dev        svo_bow_query_dev of the last 256 of 4,541 resident vectors, gap 100, top_k 4 (the 256 frames' vectors tiled)
  tracker          svo_track_batch_dev alone
  tracker_bow      svo_frontend_batch_dev + svo_track_tail_dev + svo_bow_transform_dev(producer = ctx), to the later of the two syncs
The second vocabulary has the size of a real one (k = 10, L = 6: 1,111,111 nodes): a COMPLETE RANDOM tree, not a trained one - the
walk's timing does not care what the centres are, training that size would.  Medians of --reps runs after one warm-up, with spreads
(max - min); the two tracker legs alternate.  Prints one JSON line and writes it to --out."""
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


def complete_random_tree(pkg, k, L, seed, **kw):
    n = (k ** (L + 1) - 1) // (k - 1)
    rng = np.random.default_rng(seed)
    parent = (np.arange(n, dtype=np.int64) - 1) // k
    parent[0] = -1
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    weight = np.log(50.0 / rng.integers(1, 50, n))
    return pkg.Vocabulary.from_arrays(k, L, 0, parent.astype(np.int32), desc, weight, **kw), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--database", type=int, default=4541)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_bow_bench.json"))
    args = ap.parse_args()
    import torch
    import bench
    import bow_ref
    import bow_train
    import svo_loader
    pkg = svo_loader.load()
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    dev = torch.device("cuda", 0)
    n, W, H, P, K = args.frames, bench.W, bench.H, bench.PITCH, 500
    gL, gR, _ = bench.render_frames(synth, n, dev, synth.BASE_SEED)
    cam = pkg.Camera(**pkg.KITTI_00_02)
    bx, _ = bench.boxes_hbm(pkg, n, dev)
    rec = pkg.TRACK_DTYPE.itemsize
    _, h_desc, h_n, _ = bench.frontend_outputs(pkg, cam, gL, gR, n, dev)
    docs = [h_desc[f, :h_n[f]].copy() for f in range(n)]

    def timed(fn):
        v = [fn() for _ in range(args.reps + 1)][1:]
        return {"median": float(np.median(v)), "spread": float(max(v) - min(v))}

    t0 = time.perf_counter()
    assign = bow_train.DeviceAssign(pkg)
    v4 = bow_ref.train(docs, 10, 4, 0, 0, assign_fn=assign)
    t_train = time.perf_counter() - t0
    voc4 = pkg.Vocabulary.from_arrays(v4.k, v4.L, 0, v4.parent, v4.desc, v4.weight, max_kp=K, max_frames=n)
    voc6, nodes6 = complete_random_tree(pkg, 10, 6, 1, max_kp=K, max_frames=n)

    d_desc = torch.from_numpy(h_desc).to(dev)
    d_n = torch.from_numpy(h_n).to(dev)
    words = torch.zeros((n, K), dtype=torch.int32, device=dev)
    vec = torch.zeros((n, K, 16), dtype=torch.uint8, device=dev)
    vec_n = torch.zeros(n, dtype=torch.int32, device=dev)
    fv = torch.zeros((n, K, 8), dtype=torch.uint8, device=dev)
    fv_n = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def transform_dev(voc):
        def run():
            t0 = time.perf_counter()
            voc.transform_dev(d_desc, d_n, K, n, 2, words, vec, vec_n, fv, fv_n)
            voc.sync()
            return (time.perf_counter() - t0) * 1e3
        return run

    def transform_host(voc):
        f = int(np.argmax(h_n))

        def run():
            t0 = time.perf_counter()
            voc.transform(docs[f], 2)
            return (time.perf_counter() - t0) * 1e3
        return run, int(h_n[f])

    voc6.stream
    t_dev6 = timed(transform_dev(voc6))
    t_dev4 = timed(transform_dev(voc4))          # (last: its vectors stay in vec / vec_n for the query)
    run_h, n_host = transform_host(voc4)
    t_host4 = timed(run_h)
    t_host6 = timed(transform_host(voc6)[0])
    n_desc = int(h_n.sum())
    words_mean = float(vec_n.cpu().numpy().mean())

    # the database: the 256 frames' vectors tiled to --database frames
    N, Q = args.database, min(256, args.database)
    idx = torch.arange(N, device=dev) % n
    db, db_n = vec[idx].contiguous(), vec_n[idx].contiguous()
    cand = torch.zeros((Q, 4, 16), dtype=torch.uint8, device=dev)
    cand_n = torch.zeros(Q, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def query():
        t0 = time.perf_counter()
        voc4.query_dev(db, db_n, K, N, N - Q, Q, 100, 0.0, 4, cand, cand_n)
        voc4.sync()
        return (time.perf_counter() - t0) * 1e3
    t_query = timed(query)
    h_cand = cand.cpu().numpy().reshape(-1).view(pkg.BOW_CAND_DTYPE).reshape(Q, 4)
    pairs = int(sum(max(q - 100, 0) for q in range(N - Q, N)))

    svo = pkg.Svo(W, H, max_batch=n)
    res = torch.zeros((n, rec), dtype=torch.uint8, device=dev)
    kp = torch.zeros((n, K, 28), dtype=torch.uint8, device=dev)
    fe_desc = torch.zeros((n, K, 32), dtype=torch.uint8, device=dev)
    fe_n = torch.zeros(n, dtype=torch.int32, device=dev)
    depth = torch.zeros((n, K), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    def tracker():
        svo.track_reset(cam)
        svo.sync()
        t0 = time.perf_counter()
        svo.track_batch_dev(gL.data_ptr(), gR.data_ptr(), P, n, res.data_ptr(), boxes=bx)
        svo.sync()
        return (time.perf_counter() - t0) * 1e3

    def tracker_bow():
        svo.track_reset(cam)
        svo.sync()
        t0 = time.perf_counter()
        svo.frontend_batch_dev(gL.data_ptr(), gR.data_ptr(), P, n, cam, kp.data_ptr(), fe_desc.data_ptr(), fe_n.data_ptr(), None, depth.data_ptr())
        voc4.transform_dev(fe_desc, fe_n, K, n, 2, words, vec, vec_n, fv, fv_n, producer=svo)   # (behind the front end, beside the tail)
        svo.track_tail_dev(kp.data_ptr(), fe_desc.data_ptr(), fe_n.data_ptr(), depth.data_ptr(), K, n, res.data_ptr(), boxes=bx)
        voc4.sync()
        svo.sync()
        return (time.perf_counter() - t0) * 1e3

    a, b = [], []
    for _ in range(args.reps + 1):
        a.append(tracker())
        b.append(tracker_bow())
    t_tr = {"median": float(np.median(a[1:])), "spread": float(max(a[1:]) - min(a[1:]))}
    t_tb = {"median": float(np.median(b[1:])), "spread": float(max(b[1:]) - min(b[1:]))}
    svo.close()
    out = {
        "tool": "bow_bench", "frames": n, "reps": args.reps, "descriptors": n_desc,
        "vocabulary_trained": dict(v4.describe(), training_s=t_train, assignment_calls=assign.calls),
        "vocabulary_complete_random": {"k": 10, "L": 6, "nodes": nodes6, "descriptor_bytes": nodes6 * 32,
                                       "note": "a complete random tree of a real vocabulary's size, not a trained one"},
        "gather_bytes_per_descriptor": {"k10_L4": 10 * 32 * 4, "k10_L6": 10 * 32 * 6},
        "ms": {"transform_host_k10_L4": t_host4, "transform_host_k10_L6": t_host6, "transform_dev_k10_L4": t_dev4,
               "transform_dev_k10_L6": t_dev6, "query_dev": t_query, "tracker": t_tr, "tracker_bow": t_tb},
        "transform_host_descriptors": n_host,
        "ns_per_descriptor_dev": {"k10_L4": t_dev4["median"] * 1e6 / n_desc, "k10_L6": t_dev6["median"] * 1e6 / n_desc},
        "gathered_GB_per_s": {"k10_L4": n_desc * 1280 / (t_dev4["median"] * 1e6), "k10_L6": n_desc * 1920 / (t_dev6["median"] * 1e6)},
        "words_per_frame_mean": words_mean,
        "query": {"database": N, "queries": Q, "gap": 100, "top_k": 4, "pairs": pairs, "ns_per_pair": t_query["median"] * 1e6 / max(pairs, 1),
                  "vectors": "the %d frames' vectors tiled" % n, "candidates_mean": float(cand_n.cpu().numpy().mean()),
                  "best_score_mean": float(h_cand["score"][:, 0].mean())},
        "ratio_tracker_bow_over_tracker": t_tb["median"] / t_tr["median"],
    }
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
