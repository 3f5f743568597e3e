"""GPU suite of the dynamic-keypoint loop inside the device-resident tracker (svo_track_dynamic / svo_track_dynamic_out).

Every expectation is the loop of tests/dyn_ref.py driven by the EXISTING single-call entries - track_frame (+ debug_track_matches)
for the keypoints' map points, stereo_frame for the keypoints, lk_track / lk_track_bgr for the tracker - on six synthetic
1241 x 376 frames with the box schedule of tests/test_gating.py.  Lists are compared as uint32 views, counts and dropped exactly."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import dyn_ref  # noqa: E402
import lk_bgr_cases  # noqa: E402
import lk_cases  # noqa: E402
from test_gating import boxes_for  # noqa: E402

N, W, H = 6, 1241, 376
PITCH, BPITCH = 1280, 3840
GOLD = os.path.join(os.path.dirname(__file__), "golden")


class Fixture:
    """The frames (gray, and coloured the way tests/test_lk_bgr_gpu.py colours them), per image source the keypoints and their map
    points from the single-frame entry, and the restated loops, each computed once."""

    def __init__(self, pkg):
        import torch
        self.pkg, self.torch = pkg, torch
        synth = importlib.import_module("stereo_semantic_vo_amd.synth")
        L, R, _ = synth.render_sequence(N)
        self.L, self.R = L.numpy(), R.numpy()
        assert self.L.shape == (N, H, W)
        tint = np.rint((lk_cases.smooth_canvas(70, W, H, margin=0) - 127.5) * (40.0 / 255.0)).astype(np.int32)

        def colour(g):
            c = lk_bgr_cases.replicate(g)
            c[:, :, 0] = np.clip(g.astype(np.int32) + tint, 0, 255)
            return c
        self.cL = np.stack([colour(g) for g in self.L]); self.cR = np.stack([colour(g) for g in self.R])
        self.cam = pkg.Camera(**pkg.KITTI_00_02)
        self.fe = pkg.Svo(W, H, max_batch=1)
        self._src, self._ref, self._dev = {}, {}, {}

    def close(self):
        self.fe.close()

    def source(self, kind, boxes_of=boxes_for, tag="sched", depth_source=0):
        """kind "gray": the gray frames; "bgr": the colour frames (their gray is bgr_to_gray's)."""
        key = (kind, tag, depth_source)
        if key not in self._src:
            pkg = self.pkg
            gL = self.L if kind == "gray" else np.stack([self.fe.bgr_to_gray(c) for c in self.cL])
            gR = self.R if kind == "gray" else np.stack([self.fe.bgr_to_gray(c) for c in self.cR])
            trk = pkg.Svo(W, H, max_batch=1)
            trk.set_option("depth_source", depth_source)
            trk.track_reset(self.cam)
            xy, has_mp, rec = [], [], []
            for k in range(N):
                kp = self.fe.stereo_frame(gL[k], gR[k], self.cam)["kpL"]
                res = trk.track_frame(self.L[k], self.R[k], boxes=boxes_of(k)) if kind == "gray" else \
                    trk.track_frame_bgr(self.cL[k], self.cR[k], boxes=boxes_of(k))
                assert res["n_kp"] == len(kp)
                xy.append(np.stack([kp["x"], kp["y"]], 1).astype(np.float32))
                has_mp.append(trk.debug_track_matches()[:len(kp)] >= 0)
                rec.append(res.copy())
            trk.close()
            self._src[key] = dict(gL=gL, xy=xy, has_mp=has_mp, rec=b"".join(r.tobytes() for r in rec))
        return self._src[key]

    def ref(self, kind="gray", colour=0, seed_frames=2, max_pts=512, boxes_of=boxes_for, tag="sched", depth_source=0):
        key = (kind, colour, seed_frames, max_pts, tag, depth_source)
        if key not in self._ref:
            s = self.source(kind, boxes_of, tag, depth_source)
            if colour:
                track = lambda k, p: self.fe.lk_track_bgr(self.cL[k - 1], self.cL[k], p)[:2]
            else:
                track = lambda k, p: self.fe.lk_track(s["gL"][k - 1], s["gL"][k], p)[:2]
            self._ref[key] = dyn_ref.loop(N, lambda k: s["xy"][k], lambda k: s["has_mp"][k], boxes_of, track, seed_frames, max_pts)
        return self._ref[key]

    def dev(self, kind):
        """the frames in HBM: gray rows PITCH apart, colour rows BPITCH apart"""
        if kind not in self._dev:
            torch = self.torch
            if kind == "gray":
                dL = torch.zeros((N, H, PITCH), dtype=torch.uint8, device="cuda"); dR = torch.zeros_like(dL)
                dL[:, :, :W] = torch.from_numpy(self.L).cuda(); dR[:, :, :W] = torch.from_numpy(self.R).cuda()
            else:
                dL = torch.zeros((N, H, BPITCH), dtype=torch.uint8, device="cuda"); dR = torch.zeros_like(dL)
                dL[:, :, :3 * W] = torch.from_numpy(self.cL.reshape(N, H, 3 * W)).cuda()
                dR[:, :, :3 * W] = torch.from_numpy(self.cR.reshape(N, H, 3 * W)).cuda()
            torch.cuda.synchronize()
            self._dev[kind] = (dL, dR)
        return self._dev[kind]

    def boxes_dev(self, boxes_of=boxes_for, stride=4):
        torch = self.torch
        b = np.zeros((N, stride, 4), np.int32); n = np.zeros(N, np.int32)
        for k in range(N):
            bk = boxes_of(k)
            b[k, :len(bk)] = bk; n[k] = len(bk)
        return torch.from_numpy(b).cuda(), torch.from_numpy(n).cuda(), b, n


@pytest.fixture(scope="module")
def fx(pkg):
    f = Fixture(pkg)
    yield f
    f.close()


def params(pkg, enable=1, colour=0, seed_frames=2, max_pts=512):
    p = pkg.dyn_default_params()
    p.enable, p.colour, p.seed_frames, p.max_pts = enable, colour, seed_frames, max_pts
    return p


def run_dev(fx, ctx, splits=(N,), kind="gray", max_pts=512, attach=None, dyn=True):
    """The sequence through svo_track_batch[_bgr]_dev in calls of `splits` frames, no synchronisation in between; attach[c] False:
    call c gets no svo_track_dynamic_out.  -> lists, counts, dropped (numpy; frames of unattached calls stay 0), records (bytes)"""
    torch, pkg = fx.torch, fx.pkg
    dL, dR = fx.dev(kind)
    tb, tn, _, _ = fx.boxes_dev()
    pitch = PITCH if kind == "gray" else BPITCH
    rec = pkg.TRACK_DTYPE.itemsize
    res = torch.zeros((N, rec), dtype=torch.uint8, device="cuda")
    lists = torch.zeros((N, max_pts, 2), dtype=torch.float32, device="cuda")
    counts = torch.zeros(N, dtype=torch.int32, device="cuda"); dropped = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    f0 = 0
    for c, b in enumerate(splits):
        if dyn and (attach is None or attach[c]):
            ctx.track_dynamic_out(lists.data_ptr() + f0 * max_pts * 8, counts.data_ptr() + 4 * f0, dropped.data_ptr() + 4 * f0)
        bx = pkg.boxes_dev(tb.data_ptr() + f0 * 4 * 16, tn.data_ptr() + 4 * f0, 4)
        entry = ctx.track_batch_dev if kind == "gray" else ctx.track_batch_bgr_dev
        entry(dL.data_ptr() + f0 * H * pitch, dR.data_ptr() + f0 * H * pitch, pitch, b, res.data_ptr() + f0 * rec, boxes=bx)
        f0 += b
    assert f0 == N
    ctx.sync()
    torch.cuda.synchronize()
    return lists.cpu().numpy(), counts.cpu().numpy(), dropped.cpu().numpy(), res.cpu().numpy().tobytes()


def same(got, want, frames=range(N)):
    """lists as uint32 views over the frames' used entries, counts and dropped exactly"""
    gl, gc, gd = got[:3]
    wl, wc, wd = want
    for k in frames:
        assert gc[k] == wc[k] and gd[k] == wd[k], (k, gc[k], wc[k], gd[k], wd[k])
        assert np.array_equal(gl[k, :wc[k]].view(np.uint32), wl[k, :wc[k]].view(np.uint32)), k


def new_ctx(fx, p, max_batch=N, flags=None):
    ctx = fx.pkg.Svo(W, H, max_batch=max_batch, flags=flags)
    if p is not None:
        ctx.track_dynamic(p)
    ctx.track_reset(fx.cam)
    return ctx


@pytest.mark.gpu
def test_batch_dev_equals_the_restated_loop(pkg, fx):
    """svo_track_batch_dev, gray, max_pts 512, B = 6: lists, counts and dropped (all 0) are the restated loop's, the last list is
    not empty, an inside keypoint of frame 1 is excluded for having a map point, and the records are byte-identical to the same
    call with the feature off (and to the single-frame entry's)."""
    want = fx.ref()
    src = fx.source("gray")
    inside1 = dyn_ref.strictly_inside(src["xy"][1], boxes_for(1))
    assert int((inside1 & src["has_mp"][1]).sum()) >= 1
    assert want[1][0] == 2 * int(dyn_ref.strictly_inside(src["xy"][0], boxes_for(0)).sum()) and want[1][0] > 0
    ctx = new_ctx(fx, params(pkg))
    got = run_dev(fx, ctx)
    ctx.close()
    same(got, want)
    assert not got[2].any() and got[1][N - 1] > 0
    off = new_ctx(fx, None)
    rec_off = run_dev(fx, off, dyn=False)[3]
    off.close()
    assert got[3] == rec_off and rec_off == src["rec"]


@pytest.mark.gpu
def test_split_calls_and_the_frame_entry(pkg, fx):
    """The sequence as calls of 1 + 2 + 3 frames without a sync between them (a one-frame call, the seed boundary id < 2 inside
    a call that starts at frame 1, the carried image), the same with the middle call unattached (the chain still advances), and
    frame by frame through svo_track_frame with host arrays: all the bytes of the single call."""
    want = fx.ref()
    ctx = new_ctx(fx, params(pkg))
    got = run_dev(fx, ctx, splits=(1, 2, 3))
    same(got, want)
    assert got[3] == fx.source("gray")["rec"]
    ctx.track_reset(fx.cam)
    got = run_dev(fx, ctx, splits=(1, 2, 3), attach=(True, False, True))
    same(got, want, frames=(0, 3, 4, 5))
    assert not got[1][1:3].any() and not got[0][1:3].any()
    ctx.track_reset(fx.cam)
    got = run_dev(fx, ctx, splits=(2, 4))
    same(got, want)
    ctx.close()
    one = new_ctx(fx, params(pkg), max_batch=1)
    rec = []
    for k in range(N):
        lists = np.zeros((512, 2), np.float32); cnt = np.zeros(1, np.int32); drp = np.full(1, -7, np.int32)
        if k != 2:   # (frame 2 without an attach: the chain goes on)
            one.track_dynamic_out(lists, cnt, drp)
        rec.append(one.track_frame(fx.L[k], fx.R[k], boxes=boxes_for(k)).tobytes())
        if k != 2:
            same((lists[None], cnt, drp), tuple(a[k:k + 1] for a in want), frames=(0,))
    one.close()
    assert b"".join(rec) == fx.source("gray")["rec"]


@pytest.mark.gpu
@pytest.mark.parametrize("max_pts,seed_frames", [(100, 2), (200, 2), (512, 0), (512, 1), (300, -1)])
def test_capacity_and_seed_frames(pkg, fx, max_pts, seed_frames):
    want = fx.ref(max_pts=max_pts, seed_frames=seed_frames)
    wl, wc, wd = want
    if (max_pts, seed_frames) == (100, 2):
        assert wc[0] == 100 and wd[0] == 140
    if (max_pts, seed_frames) == (200, 2):
        assert wd[0] == 40 and wd[1] > 0
    if seed_frames == 0:
        assert not wc.any() and not wd.any()
    if seed_frames == 1:
        assert wc[0] == 240 and (wc[1:] <= wc[:-1]).all()
    if seed_frames == -1:
        assert wd.sum() > 0 and wd[2:].sum() > 0
    ctx = new_ctx(fx, params(pkg, max_pts=max_pts, seed_frames=seed_frames))
    got = run_dev(fx, ctx, max_pts=max_pts)
    ctx.close()
    same(got, want)
    assert got[3] == fx.source("gray")["rec"]


@pytest.mark.gpu
@pytest.mark.parametrize("colour", [1, 0])
def test_colour_entries(pkg, fx, colour):
    """svo_track_batch_bgr_dev: colour = 1 against the loop on lk_track_bgr, colour = 0 against the gray loop on bgr_to_gray's
    frames; in two calls, so that the carried colour image is used."""
    want = fx.ref(kind="bgr", colour=colour)
    assert want[1][N - 1] > 0
    ctx = new_ctx(fx, params(pkg, colour=colour))
    got = run_dev(fx, ctx, kind="bgr", splits=(4, 2))
    ctx.close()
    same(got, want)
    assert got[3] == fx.source("bgr")["rec"]
    if colour:
        assert not np.array_equal(want[0], fx.ref(kind="bgr", colour=0)[0]), "the tint must make colour LK differ from gray LK"


def _host_run(fx, ctx, kind, pinned, splits):
    torch, pkg = fx.torch, fx.pkg
    if kind == "gray":
        srcL, srcR, stride, entry = fx.L, fx.R, W, ctx.track_batch_host
    else:
        srcL, srcR, stride, entry = fx.cL.reshape(N, H, 3 * W), fx.cR.reshape(N, H, 3 * W), 3 * W, ctx.track_batch_bgr_host
    keep = []
    if pinned:
        tL, tR = torch.from_numpy(srcL.copy()).pin_memory(), torch.from_numpy(srcR.copy()).pin_memory()
        keep = [tL, tR]
        aL, aR = tL.numpy(), tR.numpy()
    else:
        aL, aR = np.ascontiguousarray(srcL), np.ascontiguousarray(srcR)
    _, _, hb, hn = fx.boxes_dev()
    res = np.zeros(N, pkg.TRACK_DTYPE)
    lists = np.zeros((N, 512, 2), np.float32); counts = np.zeros(N, np.int32); dropped = np.full(N, -7, np.int32)
    f0 = 0
    for b in splits:
        ctx.track_dynamic_out(lists[f0:], counts[f0:], dropped[f0:])
        entry(aL[f0:].ctypes.data, aR[f0:].ctypes.data, stride, b, res[f0:], boxes=pkg.boxes_host(hb[f0:f0 + b], hn[f0:f0 + b]))
        f0 += b
    ctx.sync()
    del keep
    return lists, counts, dropped, res.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,pinned", [("gray", False), ("gray", True), ("bgr", False)])
def test_host_fed(pkg, fx, kind, pinned):
    """svo_track_batch_host from pageable and from pinned memory, two calls back to back, lists delivered to host arrays; one
    svo_track_batch_bgr_host case (LK on the colour frames)."""
    colour = 1 if kind == "bgr" else 0
    want = fx.ref(kind=kind, colour=colour)
    ctx = new_ctx(fx, params(pkg, colour=colour))
    got = _host_run(fx, ctx, kind, pinned, (3, 3))
    ctx.close()
    same(got, want)
    assert got[3] == fx.source(kind)["rec"]


@pytest.mark.gpu
def test_detector_fed(pkg, fx, tmp_path):
    """svo_det_batch_dev (on the colour left frames) with the tracker as consumer, then svo_track_batch_dev on the gray frames, no
    host synchronisation in between: the lists are the restated loop's for the boxes read back afterwards."""
    import darknet_ref as ref
    torch = fx.torch
    cfg = os.path.join(GOLD, "tiny_yolo3_small.cfg")
    net = ref.parse_cfg(cfg)
    w = str(tmp_path / "y.weights")
    ref.write_weights(w, ref.seeded_params(net, 5, obj_bias=2.5, cls_bias=2.5))
    det = pkg.Detector(cfg, w, max_batch=N)
    dL, dR = fx.dev("gray")
    drec = torch.zeros(N * 64 * 6, dtype=torch.float32, device="cuda"); dn = torch.zeros(N, dtype=torch.int32, device="cuda")
    bx = torch.zeros((N, 64, 4), dtype=torch.int32, device="cuda"); bn = torch.zeros(N, dtype=torch.int32, device="cuda")
    rec = pkg.TRACK_DTYPE.itemsize
    res = torch.zeros((N, rec), dtype=torch.uint8, device="cuda")
    lists = torch.zeros((N, 512, 2), dtype=torch.float32, device="cuda")
    counts = torch.zeros(N, dtype=torch.int32, device="cuda"); dropped = torch.zeros(N, dtype=torch.int32, device="cuda")
    ctx = new_ctx(fx, params(pkg))
    torch.cuda.synchronize()
    boxes = pkg.boxes_dev(bx.data_ptr(), bn.data_ptr(), 64)
    det.batch_dev(fx.dev("bgr")[0].data_ptr(), W, H, 3, BPITCH, N, 0.8, drec.data_ptr(), 64, dn.data_ptr(), boxes=boxes, consumer=ctx)
    ctx.track_dynamic_out(lists.data_ptr(), counts.data_ptr(), dropped.data_ptr())
    ctx.track_batch_dev(dL.data_ptr(), dR.data_ptr(), PITCH, N, res.data_ptr(), boxes=boxes)
    ctx.sync()
    torch.cuda.synchronize()
    hb, hn = bx.cpu().numpy(), bn.cpu().numpy()
    ctx.close(); det.close()
    boxes_of = lambda k: hb[k, :hn[k]]
    want = fx.ref(boxes_of=boxes_of, tag="detector")
    src = fx.source("gray", boxes_of, "detector")
    assert any(dyn_ref.strictly_inside(src["xy"][k], boxes_of(k)).any() for k in range(2)), "no box holds a keypoint: the case shows nothing"
    assert want[1][0] > 0
    same((lists.cpu().numpy(), counts.cpu().numpy(), dropped.cpu().numpy()), want)
    assert res.cpu().numpy().tobytes() == src["rec"]


@pytest.mark.gpu
def test_argument_checks(pkg, fx):
    lib = pkg.load_library()
    torch = fx.torch
    ctx = pkg.Svo(W, H, max_batch=N)
    ctx.track_reset(fx.cam)
    call = lambda p: lib.svo_track_dynamic(ctx.h, C.byref(p))
    bad = []
    for field, v in (("winSize", 15), ("maxLevel", 4), ("maxLevel", -1), ("maxCount", 20), ("epsilon", 0.02), ("minEigThreshold", 1e-3)):
        p = params(pkg); setattr(p.lk, field, v); bad.append(p)
    for field, v in (("enable", 2), ("enable", -1), ("colour", 2), ("colour", -1), ("seed_frames", -2), ("max_pts", 0), ("max_pts", -1)):
        p = params(pkg); setattr(p, field, v); bad.append(p)
    for p in bad:
        assert call(p) == -1
    p = params(pkg, max_pts=4097)
    assert call(p) == -5
    p.lk.winSize = 15
    assert call(p) == -1                       # (lk_check's order: the parameters before the count)
    assert call(params(pkg, max_pts=4096, enable=0)) == 0
    assert lib.svo_track_dynamic(ctx.h, None) == -1
    # nothing is in force before the next reset: no attach possible, the batch call runs as before
    lists = torch.zeros((N, 512, 2), dtype=torch.float32, device="cuda"); counts = torch.zeros(N, dtype=torch.int32, device="cuda")
    ctx.track_dynamic(params(pkg))
    assert lib.svo_track_dynamic_out(ctx.h, C.c_void_p(lists.data_ptr()), C.c_void_p(counts.data_ptr()), None) == -1
    assert b"not enabled" in lib.svo_last_error(ctx.h)
    assert run_dev(fx, ctx, dyn=False)[3] == fx.source("gray")["rec"]
    ctx.track_reset(fx.cam)
    assert lib.svo_track_dynamic_out(ctx.h, None, C.c_void_p(counts.data_ptr()), None) == -1
    assert lib.svo_track_dynamic_out(ctx.h, C.c_void_p(lists.data_ptr()), None, None) == -1
    # the entries without the loop refuse while it is enabled, enqueue nothing, and the context goes on
    dL, dR = fx.dev("gray")
    res = torch.zeros((N, pkg.TRACK_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    with pytest.raises(pkg.SvoError, match="svo_track_tail_dev"):
        ctx.track_tail_dev(res.data_ptr(), res.data_ptr(), res.data_ptr(), res.data_ptr(), 500, 1, res.data_ptr())
    with pytest.raises(pkg.SvoError, match="svo_track_multi_step_dev"):
        ctx.track_multi_step_dev(dL.data_ptr(), dR.data_ptr(), PITCH, 1, res.data_ptr())
    with pytest.raises(pkg.SvoError, match="svo_track_sharded_dev"):
        pkg.Svo.track_sharded_dev([ctx], [dL.data_ptr()], [dR.data_ptr()], PITCH, N, res.data_ptr())
    same(run_dev(fx, ctx), fx.ref())
    # colour = 1 through a gray entry: refused at that call
    ctx.track_dynamic(params(pkg, colour=1))
    ctx.track_reset(fx.cam)
    with pytest.raises(pkg.SvoError, match="colour"):
        ctx.track_batch_dev(dL.data_ptr(), dR.data_ptr(), PITCH, N, res.data_ptr())
    with pytest.raises(pkg.SvoError, match="colour"):
        ctx.track_frame(fx.L[0], fx.R[0])
    # switched off again: as before
    ctx.track_dynamic(params(pkg, enable=0))
    ctx.track_reset(fx.cam)
    assert lib.svo_track_dynamic_out(ctx.h, C.c_void_p(lists.data_ptr()), C.c_void_p(counts.data_ptr()), None) == -1
    assert run_dev(fx, ctx, dyn=False)[3] == fx.source("gray")["rec"]
    ctx.close()


@pytest.mark.gpu
def test_pooled_stream_mode(pkg, fx):
    """the single-call case in the pooled stream mode (no dedicated hardware queues)"""
    ctx = new_ctx(fx, params(pkg), flags=pkg.CREATE_POOLED_STREAMS)
    assert ctx.stream_mode() & 1 == 0
    got = run_dev(fx, ctx)
    ctx.close()
    same(got, fx.ref())
    assert got[3] == fx.source("gray")["rec"]


@pytest.mark.gpu
@pytest.mark.parametrize("depth_source", [1, 3])
def test_dense_depth_sources(pkg, fx, depth_source):
    """The loop beside the dense stage (ELAS maps, SGBM maps): there a call's tail is enqueued chunk by chunk, and other keypoints
    have map points than with the sparse matcher.  Two calls; seeds at every frame, so that every frame's matching counts."""
    want = fx.ref(depth_source=depth_source, seed_frames=-1, max_pts=700)
    assert want[1][N - 1] > 0
    ctx = pkg.Svo(W, H, max_batch=N)
    ctx.set_option("depth_source", depth_source)
    ctx.track_dynamic(params(pkg, seed_frames=-1, max_pts=700))
    ctx.track_reset(fx.cam)
    got = run_dev(fx, ctx, splits=(4, 2), max_pts=700)
    ctx.close()
    same(got, want)
    assert got[3] == fx.source("gray", depth_source=depth_source)["rec"]


def _write_pgm(path, img):
    with open(str(path), "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, np.uint8).tobytes())


@pytest.mark.gpu
@pytest.mark.parametrize("colour", [False, True])
def test_stereo_kitti_dynamic_dev(pkg, fx, tmp_path, colour):
    """stereo_kitti --pipelined --dynamic-dev[-bgr] --write-dynamic (calls of 3 + 1 frames) against the frame-by-frame
    --dynamic-lk[-bgr]: the point files byte for byte; the trajectory files against the pipelined run without the flag."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "stereo-semantic-vo_amd", "host", "stereo_kitti")
    n = 4
    seq = tmp_path / "seq"
    dl, dr = ("image_2", "image_3") if colour else ("image_0", "image_1")
    (seq / dl).mkdir(parents=True); (seq / dr).mkdir(); (seq / "boxes").mkdir()
    for k in range(n):
        if colour:
            lk_bgr_cases.write_png(seq / dl / ("%06d.png" % k), fx.cL[k]); lk_bgr_cases.write_png(seq / dr / ("%06d.png" % k), fx.cR[k])
        else:
            _write_pgm(seq / dl / ("%06d.pgm" % k), fx.L[k]); _write_pgm(seq / dr / ("%06d.pgm" % k), fx.R[k])
        (seq / "boxes" / ("%d.txt" % (k + 1))).write_text("".join("%d %d %d %d\n" % tuple(b) for b in boxes_for(k)))
    (seq / "times.txt").write_text("".join("%e\n" % (0.1 * k) for k in range(n)))
    y = tmp_path / "s.yaml"
    y.write_text("%YAML:1.0\nCamera.fx: 718.856\nCamera.fy: 718.856\nCamera.cx: 607.1928\nCamera.cy: 185.2157\n"
                 "Camera.width: 1241\nCamera.height: 376\nCamera.bf: 386.1448\n")
    pre = ["--colour"] if colour else []
    bgr = "-bgr" if colour else ""
    runs = {"dev": pre + ["--dynamic-dev" + bgr, "--write-dynamic", "DYN", "--pipelined", "voc", str(y), str(seq), "3"],
            "plain": pre + ["--pipelined", "voc", str(y), str(seq), "3"],
            "lk": pre + ["--dynamic-lk" + bgr, "--write-dynamic", "DYN", "voc", str(y), str(seq)]}
    for name, args in runs.items():
        (tmp_path / name / "dyn").mkdir(parents=True)
        args = [str(tmp_path / name / "dyn") if a == "DYN" else a for a in args]
        p = subprocess.run([exe] + args, capture_output=True, text=True, cwd=str(tmp_path / name), timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
    some = 0
    for k in range(n):
        a = (tmp_path / "dev" / "dyn" / ("%06d.txt" % k)).read_bytes()
        assert a == (tmp_path / "lk" / "dyn" / ("%06d.txt" % k)).read_bytes(), k
        some += len(a)
    assert some > 0 and os.listdir(str(tmp_path / "plain" / "dyn")) == []
    for f in ("cameratrajectory_kitti.txt", "cameratrajectory_tum.txt"):
        a = (tmp_path / "dev" / f).read_bytes()
        assert len(a) > 0 and a == (tmp_path / "plain" / f).read_bytes(), f
    # the flags' rules: the device loop is the pipelined mode's, the host loop the frame-by-frame mode's
    tail = ["voc", str(y), str(seq)]
    p = subprocess.run([exe] + pre + ["--dynamic-dev" + bgr] + tail, capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert p.returncode != 0 and "--pipelined" in p.stderr
    p = subprocess.run([exe] + pre + ["--dynamic-lk" + bgr, "--pipelined"] + tail, capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert p.returncode != 0 and "--pipelined" in p.stderr and "--dynamic-dev" in p.stderr
    if not colour:
        p = subprocess.run([exe, "--dynamic-dev-bgr", "--pipelined"] + tail, capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
        assert p.returncode != 0 and "--colour" in p.stderr
