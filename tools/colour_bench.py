"""Gray against colour (8UC3 BGR) input of the batched tracker, in one process with warm-up: the same synthetic sequence (synth-kitti
frames at 1241 x 376; the colour frames are a deterministic colourisation of them - per-channel look-up tables of the gray value
plus a tint that depends on the row) tracked through svo_track_batch_dev / svo_track_batch_bgr_dev (device-resident) and
svo_track_batch_host / svo_track_batch_bgr_host (pinned and pageable host memory) at depth_source 0, the gray and colour legs
alternating, plus a short depth_source 2 (MSA) leg.  Prints one JSON line of frames/s.

k_bgr2gray's own time comes from a separate run under `rocprofv3 --kernel-trace --stats`; give its kernel_stats.csv to
`--stats` and the tool prints the conversion's achieved bandwidth, 4 W H images / kernel time (3 bytes read and 1 written per
pixel), against the HBM peak.

usage: python tools/colour_bench.py [--frames 1024] [--batch 128] [--reps 2] [--msa-frames 32] [--legs dev,pinned,pageable,msa]
       python tools/colour_bench.py --stats <kernel_stats.csv> --images <converted images in that run>"""
import argparse
import csv
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1241, 376
PITCH = 1280                         # gray rows in HBM / host memory
CPITCH = 3776                        # colour rows: 3 W = 3723 bytes rounded up to 64
HBM_PEAK_GBS = 8000.0                # MI355X: HBM3E 8 TB/s spec (6.3 TB/s achievable)


def colourise(gray):
    """(n, H, W) uint8 gray tensor -> (n, H, CPITCH) uint8 BGR rows, on the gray tensor's device."""
    import torch
    v = gray.to(torch.int32)
    row = torch.arange(gray.shape[1], dtype=torch.int32, device=gray.device)[None, :, None]
    b = ((v * 7) // 8 + 16 + row % 9).clamp(0, 255)
    g = (v + row % 5 - 2).clamp(0, 255)
    r = ((v * v) // 255 + 12 + (row // 3) % 11).clamp(0, 255)
    out = torch.zeros((gray.shape[0], gray.shape[1], CPITCH), dtype=torch.uint8, device=gray.device)
    out[:, :, :3 * gray.shape[2]] = torch.stack([b, g, r], -1).to(torch.uint8).reshape(gray.shape[0], gray.shape[1], -1)
    return out


def render(n, dev):
    """n consecutive synth-kitti pairs, colourised; the gray legs get the gray of the colour frames (cv::cvtColor's fixed point:
    what the colour legs' ORB sees), so that both walk the same computation."""
    import torch
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    gL = torch.zeros((n, H, PITCH), dtype=torch.uint8, device=dev); gR = torch.zeros_like(gL)
    cL = torch.zeros((n, H, CPITCH), dtype=torch.uint8, device=dev); cR = torch.zeros_like(cL)

    def gray_of(c):
        c = c[:, :, :3 * W].reshape(c.shape[0], H, W, 3).to(torch.int32)
        return ((c[..., 0] * 1868 + c[..., 1] * 9617 + c[..., 2] * 4899 + 8192) >> 14).to(torch.uint8)
    step = 64
    for k0 in range(0, n, step):
        m = min(step, n - k0)
        L, R, _ = synth.render_sequence(m, device=dev, start=k0)
        cL[k0:k0 + m] = colourise(L); cR[k0:k0 + m] = colourise(R)
        gL[k0:k0 + m, :, :W] = gray_of(cL[k0:k0 + m]); gR[k0:k0 + m, :, :W] = gray_of(cR[k0:k0 + m])
    return gL, gR, cL, cR


def run_leg(pkg, ctx, cam, kind, colour, imgs, n, B, rec_dev, rec_host):
    """One pass over the n frames in calls of B; frames/s from the first call to the records being complete."""
    import torch
    aL, aR = imgs
    pitch = CPITCH if colour else PITCH
    fb = H * pitch
    ctx.track_reset(cam)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k0 in range(0, n, B):
        b = min(B, n - k0)
        pl = (aL.data_ptr() if hasattr(aL, "data_ptr") else aL.ctypes.data) + k0 * fb
        pr = (aR.data_ptr() if hasattr(aR, "data_ptr") else aR.ctypes.data) + k0 * fb
        if kind == "dev":
            f = ctx.track_batch_bgr_dev if colour else ctx.track_batch_dev
            f(pl, pr, pitch, b, rec_dev.data_ptr() + k0 * pkg.TRACK_DTYPE.itemsize)
        else:
            f = ctx.track_batch_bgr_host if colour else ctx.track_batch_host
            f(pl, pr, pitch, b, rec_host[k0:k0 + b])
    ctx.sync()
    dt = time.perf_counter() - t0
    return n / dt, (rec_dev[:n * pkg.TRACK_DTYPE.itemsize].cpu().numpy().tobytes() if kind == "dev" else rec_host[:n].tobytes())


def bench(args):
    import numpy as np
    import torch
    import svo_loader
    pkg = svo_loader.load()
    dev = torch.device("cuda", 0)
    n, B = args.frames, args.batch
    t_r = time.perf_counter()
    gL, gR, cL, cR = render(n, dev)
    render_s = time.perf_counter() - t_r
    cam = pkg.Camera(**pkg.KITTI_00_02)
    legs = set(args.legs.split(","))
    out = {"tool": "colour_bench", "W": W, "H": H, "frames_per_leg": n, "frames_per_call": B, "reps": args.reps,
           "render_s": round(render_s, 1)}
    rec_dev = torch.zeros(n * pkg.TRACK_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    rec_host = np.zeros(n, pkg.TRACK_DTYPE)
    ctx = pkg.Svo(W, H, max_batch=B)
    sources = {}
    if "dev" in legs:
        sources["dev"] = {False: (gL, gR), True: (cL, cR)}
    if "pinned" in legs or "pageable" in legs:
        hg = (gL.cpu(), gR.cpu()); hc = (cL.cpu(), cR.cpu())
        if "pinned" in legs:
            sources["pinned"] = {False: (hg[0].pin_memory(), hg[1].pin_memory()), True: (hc[0].pin_memory(), hc[1].pin_memory())}
        if "pageable" in legs:
            sources["pageable"] = {False: (hg[0].numpy(), hg[1].numpy()), True: (hc[0].numpy(), hc[1].numpy())}
    same = True
    images = 0   # colour images k_bgr2gray converted (for --stats of a profiled run)
    for name, src in sources.items():
        kind = "dev" if name == "dev" else "host"
        for colour in (False, True):   # warm-up: allocations, stream picks, the colour staging
            run_leg(pkg, ctx, cam, kind, colour, src[colour], min(n, 2 * B), B, rec_dev, rec_host)
        images += 2 * min(n, 2 * B) + 2 * n * args.reps
        rates = {False: [], True: []}
        recs = {}
        for _ in range(args.reps):
            for colour in (False, True):
                r, rec = run_leg(pkg, ctx, cam, kind, colour, src[colour], n, B, rec_dev, rec_host)
                rates[colour].append(r)
                recs[colour] = rec
        same &= recs[False] == recs[True]
        for colour in (False, True):
            key = "%s_%s_fps" % (name, "colour" if colour else "gray")
            out[key] = round(float(np.median(rates[colour])), 1)
            out[key + "_all"] = [round(x, 1) for x in rates[colour]]
        out["%s_colour_over_gray" % name] = round(out["%s_colour_fps" % name] / out["%s_gray_fps" % name], 4)
    out["depth0_records_equal"] = bool(same)
    ctx.close()
    if "msa" in legs and args.msa_frames > 0:
        m = args.msa_frames
        ctx = pkg.Svo(W, H, max_batch=m)
        ctx.set_option("depth_source", 2)
        for colour in (False, True):
            run_leg(pkg, ctx, cam, "dev", colour, (cL, cR) if colour else (gL, gR), min(m, 4), m, rec_dev, rec_host)
        images += 2 * min(m, 4) + 2 * m
        for colour in (False, True):
            r, _ = run_leg(pkg, ctx, cam, "dev", colour, (cL, cR) if colour else (gL, gR), m, m, rec_dev, rec_host)
            out["msa_dev_%s_fps" % ("colour" if colour else "gray")] = round(r, 2)
        out["msa_frames"] = m
        ctx.close()
    out["colour_images_converted"] = images
    print(json.dumps(out))


def stats(args):
    """k_bgr2gray's total time in a rocprofv3 kernel_stats.csv -> achieved bytes/s of the conversion."""
    row = None
    with open(args.stats) as f:
        for r in csv.DictReader(f):
            if "k_bgr2gray" in r.get("Name", ""):
                row = r
    if row is None:
        print(json.dumps({"tool": "colour_bench", "k_bgr2gray": "not in " + args.stats}))
        return
    total_ns = float(row["TotalDurationNs"])
    calls = int(row["Calls"])
    gbs = 4.0 * W * H * args.images / total_ns   # bytes per ns = GB/s
    print(json.dumps({"tool": "colour_bench", "k_bgr2gray_calls": calls, "k_bgr2gray_total_us": round(total_ns / 1e3, 1),
                      "k_bgr2gray_avg_us": round(total_ns / 1e3 / calls, 2), "images": args.images,
                      "us_per_pair": round(total_ns / 1e3 / (args.images / 2), 3), "achieved_GBps": round(gbs, 1),
                      "of_hbm_peak": round(gbs / HBM_PEAK_GBS, 3)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--msa-frames", type=int, default=32)
    ap.add_argument("--legs", default="dev,pinned,pageable,msa")
    ap.add_argument("--stats", help="rocprofv3 kernel_stats.csv of a run of this tool")
    ap.add_argument("--images", type=int, default=0, help="with --stats: images k_bgr2gray converted in that run")
    a = ap.parse_args()
    if a.stats:
        stats(a)
    else:
        bench(a)
