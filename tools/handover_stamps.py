"""The fused pose launch's hand-over from the RANSAC samples to the LM, over 256 frames of the headline sequence: rt[5] of
svo_debug_track_frames (latest announcement of an awaited sample -> the LM's first build; 10 ns ticks, printed in us), the frame
part rt[3] - rt[4], and the cycle columns of tools/pose_stamps.py (last frame of every call of 64; k cycles).
SVO_LIB_PATH=<another build of the library> gives the same for that build."""
import os, sys, importlib, ctypes as C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, svo_loader, bench
pkg = svo_loader.load()
synth = importlib.import_module("stereo_semantic_vo_amd.synth")
dev = torch.device("cuda", 0)
N, B = 256, 64
dL, dR, T = bench.render_frames(synth, N, dev, synth.BASE_SEED)
cam = pkg.Camera(**pkg.KITTI_00_02)
rec = pkg.TRACK_DTYPE.itemsize
fb = bench.H * bench.PITCH
s = pkg.Svo(bench.W, bench.H, device=0, max_kp=500, max_batch=B)
res = torch.zeros((N, rec), dtype=torch.uint8, device=dev)
for rep in range(2):   # (the first pass warms the caches and clocks up; the second is reported)
    s.track_reset(cam)
    dbg, rows = [], []
    for c0 in range(0, N, B):
        s.track_batch_dev(dL.data_ptr() + c0 * fb, dR.data_ptr() + c0 * fb, bench.PITCH, B, res.data_ptr() + c0 * rec)
        dbg.append(s.debug_track_frames(0, B).copy())
        ts = (C.c_int64 * 16)()
        s.lib.svo_debug_track_pose_stamps(s.h, ts)
        t = np.array(list(ts), np.float64) / 1000.0
        r = res[c0 + B - 1].cpu().numpy().view(pkg.TRACK_DTYPE)[0]
        rows.append((t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3], t[9] - t[8], t[10] - t[9], t[11] - t[10], int(r["n_lm_edges"]), int(r["lm_iterations"])))
dbg = np.concatenate(dbg)
rt = dbg["rt"].astype(np.int64)


def line(name, v):
    v = np.asarray(v, np.float64) * 0.01
    print("%-44s n = %3d   mean %7.2f   median %7.2f   p95 %7.2f   min %7.2f   max %7.2f  us" %
          (name, len(v), v.mean(), np.median(v), np.percentile(v, 95), v.min(), v.max()))


early = rt[:, 5] > 0
line("hand-over rt[5] (frames decided early)", rt[early, 5])
line("frame part rt[3] - rt[4] (those frames)", (rt[:, 3] - rt[:, 4])[early])
line("frame part rt[3] - rt[4] (all frames)", rt[:, 3] - rt[:, 4])
line("samples rt[4] - rt[2] (RANSAC frames)", (rt[:, 4] - rt[:, 2])[dbg["pnp_iterations"] > 0])
line("frame period rt[3][f] - rt[3][f - 1]", np.diff(rt[:, 3])[np.arange(1, N) % B != 0])
print("frames not decided within the awaited samples: %d of %d" % (int(((rt[:, 5] == 0) & (dbg["pnp_iterations"] > 0)).sum()), N))
print("samples: gather, to EPnP start, EPnP, consensus | frame part: gather+wait+rule, LM, record | edges, LM iterations   (k cycles)")
for r in rows:
    print("  %5.1f %5.1f %5.1f %5.1f | %5.1f %5.1f %5.1f | %d %d" % r)
print("  %5.1f %5.1f %5.1f %5.1f | %5.1f %5.1f %5.1f |   (mean)" % tuple(np.mean([r[:7] for r in rows], axis=0)))
s.close()
