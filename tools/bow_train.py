#!/usr/bin/env python3
"""bow_train.py - train a DBoW2 vocabulary for this library's descriptors and write it in DBoW2's text format.

ORB-SLAM2's published vocabulary was trained on the learned rBRIEF pattern and does not fit the descriptors of this library
(include/svo_brief_pattern.h), so a vocabulary has to be made from the tracker's own descriptors.  The procedure is the contract's
(DESIGN.md section 8 "Bag of words", Training; restated in tests/bow_ref.py): DBoW2's create / HKmeansStep / kmeans++ / bit-majority
mean / idf, with the kmeans++ draws from a numpy Generator (PCG64) seeded by --seed.

Input, one of
  --descriptors d.npy --documents b.npy   (n, 32) uint8 descriptors and the documents' boundaries: document i is rows b[i] .. b[i + 1]
  --frames N                              the first N frames of the synthetic sequence (of KITTI 00 when KITTI_ROOT is set) through
                                          the device front end, a frame a document
The assignment steps (every descriptor against up to k centres) run on the GPU through svo_bow_assign_dev, or with --cpu in numpy;
both write the same file."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


class DeviceAssign:
    """svo_bow_assign_dev behind the twin's assign(descs, centres) -> (index, distance).  The entry belongs to a vocabulary object:
    a two-node one serves."""

    def __init__(self, pkg, device=0):
        import torch
        self.torch = torch
        self.voc = pkg.Vocabulary.from_arrays(2, 1, 0, [-1, 0], np.zeros((2, 32), np.uint8), [0.0, 1.0], max_kp=1, device=device)
        self.calls = 0

    def __call__(self, descs, centres):
        torch = self.torch
        descs = np.ascontiguousarray(descs, np.uint8).reshape(-1, 32)
        centres = np.ascontiguousarray(centres, np.uint8).reshape(-1, 32)
        n = len(descs)
        if n == 0:
            return np.zeros(0, np.int32), np.zeros(0, np.int32)
        d_desc, d_c = torch.from_numpy(descs).cuda(), torch.from_numpy(centres).cuda()
        idx = torch.zeros(n, dtype=torch.int32, device="cuda")
        dist = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self.voc.assign_dev(d_desc, n, d_c, len(centres), idx, dist)
        self.voc.sync()
        self.calls += 1
        return idx.cpu().numpy(), dist.cpu().numpy()


def frontend_documents(pkg, n_frames):
    import torch
    import bench
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    dev = torch.device("cuda", 0)
    dL, dR, _ = bench.render_frames(synth, n_frames, dev, synth.BASE_SEED)
    cam = pkg.Camera(**pkg.KITTI_00_02)
    _, desc, n, _ = bench.frontend_outputs(pkg, cam, dL, dR, n_frames, dev)
    return [desc[f, :n[f]].copy() for f in range(n_frames)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--descriptors")
    ap.add_argument("--documents")
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--L", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--weighting", type=int, default=0, help="0 TF_IDF, 1 TF, 2 IDF, 3 BINARY")
    ap.add_argument("--cpu", action="store_true", help="assignment steps in numpy instead of svo_bow_assign_dev")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    import bow_ref
    if not 2 <= args.k <= 20 or not 1 <= args.L <= 10 or not 0 <= args.weighting <= 3:
        ap.error("k must be 2 .. 20, L 1 .. 10, weighting 0 .. 3")
    if bool(args.descriptors) == bool(args.frames):
        ap.error("give either --descriptors with --documents, or --frames")
    pkg = None
    if args.frames or not args.cpu:
        import svo_loader
        pkg = svo_loader.load()
    if args.descriptors:
        if not args.documents:
            ap.error("--descriptors needs --documents")
        d = np.load(args.descriptors)
        b = np.load(args.documents).astype(np.int64)
        if d.dtype != np.uint8 or d.ndim != 2 or d.shape[1] != 32:
            ap.error("descriptors must be (n, 32) uint8")
        if b.ndim != 1 or len(b) < 2 or b[0] != 0 or b[-1] != len(d) or (np.diff(b) < 0).any():
            ap.error("documents must be ascending boundaries from 0 to n")
        docs = [d[s:e] for s, e in zip(b[:-1], b[1:])]
    else:
        docs = frontend_documents(pkg, args.frames)
    assign = None if args.cpu else DeviceAssign(pkg)
    t0 = time.perf_counter()
    voc = bow_ref.train(docs, args.k, args.L, args.weighting, args.seed, assign_fn=assign)
    dt = time.perf_counter() - t0
    with open(args.out, "w") as f:
        f.write(bow_ref.format_text(voc))
    d = voc.describe()
    sys.stderr.write("bow_train: %d documents, %d descriptors -> %d nodes, %d words (k = %d, L = %d) in %.1f s%s\n" %
                     (len(docs), sum(len(x) for x in docs), d["nodes"], d["words"], args.k, args.L, dt,
                      "" if assign is None else ", %d assignment calls on the device" % assign.calls))
    return 0


if __name__ == "__main__":
    sys.exit(main())
