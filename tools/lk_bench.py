"""Timings of the pyramidal Lucas-Kanade entries (svo_lk_*): one 1241 x 376 pair with 500 points host to host, 64 resident
frames x 500 points through the batch entry, and the chain entry over the same frames.  Median and min .. max of 7 timed runs
after a warm-up; one JSON line.  --bgr: the same three on 8UC3 frames through the _bgr entries (the gray frames as the G channel,
B and R from two other textures); --both: gray, then colour, and the colour / gray ratios of the medians, in one line.
--out FILE also writes the line to FILE."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _timed(fn, runs=7):
    fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)
    return dict(median_ms=1e3 * float(np.median(t)), min_ms=1e3 * min(t), max_ms=1e3 * max(t))


def measure(pkg, bgr):
    import torch
    import util
    W, H, B, n = 1241, 376, 64, 500
    if bgr:
        base = np.stack([util.blocky_image(s, W + 2 * B, H) for s in (4, 3, 5)], axis=2)
    else:
        base = util.blocky_image(3, W + 2 * B, H)
    frames = np.stack([np.ascontiguousarray(base[:, 2 * b:2 * b + W]) for b in range(B)])
    rng = np.random.default_rng(0)
    pts = rng.uniform((30, 30), (W - 30, H - 30), (B, n, 2)).astype(np.float32)
    svo = pkg.Svo(W, H, max_batch=1)
    track, batch, chain = ((svo.lk_track_bgr, svo.lk_batch_bgr_dev, svo.lk_chain_bgr_dev) if bgr else
                           (svo.lk_track, svo.lk_batch_dev, svo.lk_chain_dev))
    W = 3 * W if bgr else W                                  # from here on: a row's bytes
    out = {"pair_host_to_host": _timed(lambda: track(frames[0], frames[1], pts[0]))}
    dev = torch.device("cuda", 0)
    d_f = torch.from_numpy(frames).to(dev)
    d_pts = torch.from_numpy(pts).to(dev); d_cnt = torch.full((B,), n, dtype=torch.int32, device=dev)
    d_next = torch.zeros((B, n, 2), dtype=torch.float32, device=dev); d_st = torch.zeros((B, n), dtype=torch.uint8, device=dev)
    d_err = torch.zeros((B, n), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    r = _timed(lambda: batch(d_f.data_ptr(), W, W // (3 if bgr else 1), H, B, d_pts.data_ptr(), d_cnt.data_ptr(), n, d_next.data_ptr(),
                            d_st.data_ptr(), d_err.data_ptr()))
    r["pairs_per_s"] = (B - 1) / (r["median_ms"] * 1e-3)
    out["batch_64_frames"] = r
    d_sc = torch.zeros((B,), dtype=torch.int32, device=dev); d_sc[0] = n
    d_lists = torch.zeros((B, n, 2), dtype=torch.float32, device=dev)
    d_lc = torch.zeros((B,), dtype=torch.int32, device=dev); d_dr = torch.zeros((B,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    r = _timed(lambda: chain(d_f.data_ptr(), W, W // (3 if bgr else 1), H, B, d_pts.data_ptr(), d_sc.data_ptr(), n, n, d_lists.data_ptr(),
                            d_lc.data_ptr(), d_dr.data_ptr()))
    r["frames_per_s"] = B / (r["median_ms"] * 1e-3)
    r["last_list"] = int(d_lc.cpu()[-1])
    out["chain_64_frames"] = r
    svo.close()
    return out


def main():
    import svo_loader
    pkg = svo_loader.load()
    args = sys.argv[1:]
    if "--both" in args:
        gray, colour = measure(pkg, False), measure(pkg, True)
        ratio = {k: colour[k]["median_ms"] / gray[k]["median_ms"] for k in gray}
        line = json.dumps({"lk_bench": gray, "lk_bench_bgr": colour, "bgr_over_gray_median": ratio})
    elif "--bgr" in args:
        line = json.dumps({"lk_bench_bgr": measure(pkg, True)})
    else:
        line = json.dumps({"lk_bench": measure(pkg, False)})
    print(line)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
