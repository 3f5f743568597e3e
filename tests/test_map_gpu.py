"""GPU suite of svo_track_map_out: each tracked frame's map points and observations, delivered by the tracker entries.

Six synthetic 1241 x 376 frames with the box schedule of tests/test_gating.py (as tests/test_dynamic_dev_gpu.py).  Every expectation
comes from existing, separately pinned entries: svo_debug_track_frames (identities), svo_frontend_batch_dev / svo_debug_track_depths
(u, v, depth) and the result records' poses through tests/map_ref.py (positions; its unproject is pinned to orc_unproject by
tests/test_map_cpu.py).  Records are compared as raw bytes."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import lk_bgr_cases  # noqa: E402
import map_ref  # noqa: E402
from test_gating import boxes_for  # noqa: E402

N, W, H, K = 6, 1241, 376, 500
PITCH, BPITCH = 1280, 3840
GUARD = 0xA5


class Fixture:
    def __init__(self, pkg):
        import torch
        self.pkg, self.torch = pkg, torch
        synth = importlib.import_module("stereo_semantic_vo_amd.synth")
        L, R, _ = synth.render_sequence(N)
        self.L, self.R = L.numpy(), R.numpy()
        assert self.L.shape == (N, H, W)
        self.cam = pkg.Camera(**pkg.KITTI_00_02)
        c = pkg.KITTI_00_02
        self.cam4 = (c["fx"], c["fy"], c["cx"], c["cy"])
        self.rec = pkg.TRACK_DTYPE.itemsize
        dL = torch.zeros((N, H, PITCH), dtype=torch.uint8, device="cuda"); dR = torch.zeros_like(dL)
        dL[:, :, :W] = torch.from_numpy(self.L).cuda(); dR[:, :, :W] = torch.from_numpy(self.R).cuda()
        self.dL, self.dR = dL, dR
        b = np.zeros((N, 4, 4), np.int32); n = np.zeros(N, np.int32)
        for k in range(N):
            bk = boxes_for(k)
            b[k, :len(bk)] = bk; n[k] = len(bk)
        self.hb, self.hn = b, n
        self.tb, self.tn = torch.from_numpy(b).cuda(), torch.from_numpy(n).cuda()
        # the stateless front end's arrays of the six pairs, in HBM (what svo_track_tail_dev is fed) and on the host
        fe = pkg.Svo(W, H, max_batch=N)
        self.fe_kp = torch.zeros((N, K, pkg.KP_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        self.fe_desc = torch.zeros((N, K, 32), dtype=torch.uint8, device="cuda")
        self.fe_n = torch.zeros(N, dtype=torch.int32, device="cuda")
        self.fe_uR = torch.zeros((N, K), dtype=torch.float32, device="cuda")
        self.fe_depth = torch.zeros((N, K), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        fe.frontend_batch_dev(dL.data_ptr(), dR.data_ptr(), PITCH, N, self.cam, self.fe_kp.data_ptr(), self.fe_desc.data_ptr(),
                              self.fe_n.data_ptr(), self.fe_uR.data_ptr(), self.fe_depth.data_ptr())
        fe.sync()
        fe.close()
        self.kp = self.fe_kp.cpu().numpy().reshape(N, -1).view(pkg.KP_DTYPE).reshape(N, K)
        self.nkp = self.fe_n.cpu().numpy()
        self.depth = self.fe_depth.cpu().numpy()
        self._want = {}

    def boxes(self, f0):
        return self.pkg.boxes_dev(self.tb.data_ptr() + f0 * 4 * 16, self.tn.data_ptr() + 4 * f0, 4)

    def new_ctx(self, max_batch=N, depth_source=0, dyn=None):
        ctx = self.pkg.Svo(W, H, max_batch=max_batch)
        if depth_source:
            ctx.set_option("depth_source", depth_source)
        if dyn is not None:
            ctx.track_dynamic(dyn)
        ctx.track_reset(self.cam)
        return ctx

    def want(self, depth_source=0):
        """-> (per-frame expected record arrays, result records as bytes, per-frame debug records) of a run WITHOUT the attachment"""
        if depth_source not in self._want:
            pkg, torch = self.pkg, self.torch
            if depth_source == 0:
                ctx = self.new_ctx()
                res = torch.zeros((N, self.rec), dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                ctx.track_batch_dev(self.dL.data_ptr(), self.dR.data_ptr(), PITCH, N, res.data_ptr(), boxes=self.boxes(0))
                ctx.sync()
                dbg = ctx.debug_track_frames(0, N)
                rec = res.cpu().numpy().reshape(-1).view(pkg.TRACK_DTYPE)
                xy = [np.stack([self.kp[k]["x"], self.kp[k]["y"]], 1)[:self.nkp[k]] for k in range(N)]
                z = [self.depth[k, :self.nkp[k]] for k in range(N)]
                ctx.close()
            else:   # (a dense call's tail runs in chunks: frame by frame, where every probe answers for the frame just tracked)
                ctx = self.new_ctx(max_batch=1, depth_source=depth_source)
                rec = np.zeros(N, pkg.TRACK_DTYPE); dbg = np.zeros(N, pkg.TRACK_DEBUG_DTYPE); xy, z = [], []
                for k in range(N):
                    rec[k] = ctx.track_frame(self.L[k], self.R[k], boxes=boxes_for(k))
                    dbg[k] = ctx.debug_track_frames(0, 1)[0]
                    kp, d = ctx.debug_track_depths(0)
                    xy.append(np.stack([kp["x"], kp["y"]], 1).astype(np.float32)); z.append(d.copy())
                ctx.close()
            pos, lists = {}, []
            for k in range(N):
                assert rec[k]["n_kp"] == len(xy[k]) and dbg[k]["frame_id"] == k
                lists.append(map_ref.expected(k, dbg[k]["match_gid"], dbg[k]["new_gid"], xy[k], z[k], self.cam4, rec[k]["Tcw"], pos))
            self._want[depth_source] = (lists, rec.tobytes(), dbg, z)
        return self._want[depth_source]


@pytest.fixture(scope="module")
def fx(pkg):
    return Fixture(pkg)


def guarded(fx, frames, k=K, extra=64):
    """obs for `frames` frames of k records + `extra` bytes behind them, counts - all filled with the guard byte (HBM)"""
    torch = fx.torch
    obs = torch.full((frames * k * 32 + extra,), GUARD, dtype=torch.uint8, device="cuda")
    counts = torch.full((frames + 4,), -1, dtype=torch.int32, device="cuda")
    return obs, counts


def check(obs, counts, want, frames, k=K, armed=None, extra=64):
    """obs (bytes, numpy), counts (int32, numpy): frame f's records are want[frames[f]] byte for byte, kp strictly ascending, and
    every byte behind a frame's records and behind the last frame still holds the guard.  armed[f] False: nothing written at all."""
    obs = np.asarray(obs).view(np.uint8).reshape(-1)
    for f, k_abs in enumerate(frames):
        row = obs[f * k * 32:(f + 1) * k * 32]
        if armed is not None and not armed[f]:
            assert (row == GUARD).all() and counts[f] == -1, f
            continue
        w = want[k_abs]
        assert counts[f] == len(w), (f, counts[f], len(w))
        got = row[:len(w) * 32].view(map_ref.OBS)
        assert (np.diff(got["kp"].astype(np.int32)) > 0).all(), f
        assert got.tobytes() == w.tobytes(), (f, np.flatnonzero(got.view(np.uint32) != w.view(np.uint32))[:8])
        assert (row[len(w) * 32:] == GUARD).all(), f
    if extra:
        assert (obs[len(frames) * k * 32:] == GUARD).all()
    assert (np.asarray(counts)[len(frames):] == -1).all()


def run_dev(fx, ctx, splits=(N,), arm=None, bgr=False, dyn_out=None):
    """the sequence through svo_track_batch[_bgr]_dev in calls of `splits` frames, no synchronisation in between; arm[c] False:
    call c is made without svo_track_map_out -> obs bytes, counts, records (bytes)"""
    torch = fx.torch
    obs, counts = guarded(fx, N)
    res = torch.zeros((N, fx.rec), dtype=torch.uint8, device="cuda")
    if bgr:
        cL = torch.from_numpy(np.stack([lk_bgr_cases.replicate(g) for g in fx.L]).reshape(N, H, 3 * W)).cuda()
        cR = torch.from_numpy(np.stack([lk_bgr_cases.replicate(g) for g in fx.R]).reshape(N, H, 3 * W)).cuda()
        dL = torch.zeros((N, H, BPITCH), dtype=torch.uint8, device="cuda"); dR = torch.zeros_like(dL)
        dL[:, :, :3 * W] = cL; dR[:, :, :3 * W] = cR
        pitch, entry = BPITCH, ctx.track_batch_bgr_dev
    else:
        dL, dR, pitch, entry = fx.dL, fx.dR, PITCH, ctx.track_batch_dev
    torch.cuda.synchronize()
    f0 = 0
    for c, b in enumerate(splits):
        if arm is None or arm[c]:
            ctx.track_map_out(obs.data_ptr() + f0 * K * 32, counts.data_ptr() + 4 * f0)
        if dyn_out is not None:
            lists, cnt, drp = dyn_out
            ctx.track_dynamic_out(lists.data_ptr() + f0 * 512 * 8, cnt.data_ptr() + 4 * f0, drp.data_ptr() + 4 * f0)
        entry(dL.data_ptr() + f0 * H * pitch, dR.data_ptr() + f0 * H * pitch, pitch, b, res.data_ptr() + f0 * fx.rec, boxes=fx.boxes(f0))
        f0 += b
    assert f0 == N
    ctx.sync()
    torch.cuda.synchronize()
    return obs.cpu().numpy(), counts.cpu().numpy(), res.cpu().numpy().tobytes()


@pytest.mark.gpu
def test_batch_dev_one_call(pkg, fx):
    """svo_track_batch_dev, one call of 6: every frame's records are the restated list byte for byte; counts = matched + created;
    new points lie where orc_unproject puts them under that frame's SetPose (identity at frame 0) - map_ref.expected computes
    exactly that -; every gid is new exactly once, in the first frame it appears in; a matched record carries the bits exported
    when its gid was new; and the result records are those of the run without the attachment."""
    want, rec_off, dbg, _ = fx.want()
    # the schedule must make epipolar vetoes and gated creation occur, or the case shows nothing
    one = fx.new_ctx(max_batch=1)
    vetoes = 0
    for k in range(N):
        one.track_frame(fx.L[k], fx.R[k], boxes=boxes_for(k))
        if k > 0:
            vetoes += one.debug_track_gate()[1]
    one.close()
    assert vetoes > 0, "no epipolar veto in the schedule: the case shows nothing"
    gated = 0
    for k in range(N):
        n = fx.nkp[k]
        free = (dbg[k]["match_gid"][:n] < 0) & (dbg[k]["new_gid"][:n] < 0) & (fx.depth[k, :n] > 0)
        gated += int(free.sum())
    assert gated > 0, "no keypoint with depth was kept from becoming a map point: the case shows nothing"
    ctx = fx.new_ctx()
    obs, counts, rec = run_dev(fx, ctx)
    ctx.close()
    check(obs, counts, want, range(N))
    assert rec == rec_off
    first, exported = {}, {}
    for k in range(N):
        n = fx.nkp[k]
        assert counts[k] == int((dbg[k]["match_gid"][:n] >= 0).sum() + (dbg[k]["new_gid"][:n] >= 0).sum())
        got = obs[k * K * 32:][:counts[k] * 32].view(map_ref.OBS)
        assert len(got) > 0 and (got["depth"][got["flags"] == 1] > 0).all()
        for r in got:
            g, xyz = int(r["gid"]), (r["X"].tobytes(), r["Y"].tobytes(), r["Z"].tobytes())
            if g not in first:
                assert r["flags"] == pkg.MAP_NEW, (k, g)
                first[g] = k; exported[g] = xyz
            else:
                assert r["flags"] == 0 and first[g] < k and exported[g] == xyz, (k, g)
    # matched and created records both occur (five correspondences are what PnP needs to run at all), or the checks above are idle
    assert any((w["flags"] == 0).sum() >= 5 for w in want[1:]) and all((w["flags"] == 1).sum() > 0 for w in want)


@pytest.mark.gpu
@pytest.mark.parametrize("splits,arm", [((3, 3), None), ((1, 5), None), ((2, 2, 2), (True, False, True))])
def test_split_calls(pkg, fx, splits, arm):
    """consecutive calls alternate the halves of the work records and the front-end output sets; a call made without arming
    between two armed ones writes nothing and leaves the later call's records unchanged"""
    want, rec_off, _, _ = fx.want()
    ctx = fx.new_ctx()
    obs, counts, rec = run_dev(fx, ctx, splits=splits, arm=arm)
    ctx.close()
    armed = None if arm is None else [arm[c] for c, b in enumerate(splits) for _ in range(b)]
    check(obs, counts, want, range(N), armed=armed)
    assert rec == rec_off


@pytest.mark.gpu
def test_bgr_entries_on_replicated_gray(pkg, fx):
    want, rec_off, _, _ = fx.want()
    ctx = fx.new_ctx()
    obs, counts, rec = run_dev(fx, ctx, splits=(4, 2), bgr=True)
    ctx.close()
    check(obs, counts, want, range(N))
    assert rec == rec_off
    one = fx.new_ctx(max_batch=1)
    for k in range(N):
        o = np.full(K * 32 + 64, GUARD, np.uint8); c = np.full(5, -1, np.int32)
        o = o[(-o.ctypes.data) % 16:][:K * 32 + 32]
        one.track_map_out(o, c)
        one.track_frame_bgr(lk_bgr_cases.replicate(fx.L[k]), lk_bgr_cases.replicate(fx.R[k]), boxes=boxes_for(k))
        check(o, c, want, [k], extra=32)
    one.close()


@pytest.mark.gpu
def test_frame_entry_and_host_fed(pkg, fx):
    """svo_track_frame with host arrays (complete on return; frame 2 not armed), svo_track_batch_host in two calls with host
    arrays read after svo_sync"""
    want, rec_off, _, _ = fx.want()
    one = fx.new_ctx(max_batch=1)
    recs = []
    for k in range(N):
        o = np.full(K * 32 + 64, GUARD, np.uint8); c = np.full(5, -1, np.int32)
        o = o[(-o.ctypes.data) % 16:][:K * 32 + 32]
        if k != 2:
            one.track_map_out(o, c)
        recs.append(one.track_frame(fx.L[k], fx.R[k], boxes=boxes_for(k)).tobytes())
        check(o, c, want, [k], armed=[k != 2], extra=32)
    one.close()
    assert b"".join(recs) == rec_off
    ctx = fx.new_ctx()
    raw = np.full(N * K * 32 + 80, GUARD, np.uint8)
    obs = raw[(-raw.ctypes.data) % 16:][:N * K * 32 + 64]
    counts = np.full(N + 4, -1, np.int32)
    res = np.zeros(N, pkg.TRACK_DTYPE)
    aL, aR = np.ascontiguousarray(fx.L), np.ascontiguousarray(fx.R)
    f0 = 0
    for b in (3, 3):
        ctx.track_map_out(obs[f0 * K * 32:], counts[f0:])
        ctx.track_batch_host(aL[f0:].ctypes.data, aR[f0:].ctypes.data, W, b, res[f0:], boxes=pkg.boxes_host(fx.hb[f0:f0 + b], fx.hn[f0:f0 + b]))
        f0 += b
    ctx.sync()
    ctx.close()
    check(obs, counts, want, range(N))
    assert res.tobytes() == rec_off


def dyn_params(pkg):
    p = pkg.dyn_default_params()
    p.enable, p.max_pts = 1, 512
    return p


def dyn_want(fx):
    """the loop's lists, counts and dropped counts of the six frames (numpy), from the _dev entry without the map attachment - the
    run test_with_the_dynamic_loop takes them from; made once"""
    if "dyn" not in fx._want:
        torch = fx.torch
        d = (torch.zeros((N, 512, 2), dtype=torch.float32, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda"),
             torch.full((N,), -7, dtype=torch.int32, device="cuda"))
        ctx = fx.new_ctx(dyn=dyn_params(fx.pkg))
        run_dev(fx, ctx, splits=(2, 4), arm=(False, False), dyn_out=d)
        ctx.close()
        fx._want["dyn"] = tuple(a.cpu().numpy() for a in d)
        assert fx._want["dyn"][1][N - 1] > 0
    return fx._want["dyn"]


def host_fed_three_calls(pkg, fx, armed_calls):
    """svo_track_batch_host in calls of 2, 2 and 2 frames on a context with the dynamic-keypoint loop (max_pts 512); both
    svo_track_map_out and svo_track_dynamic_out armed with host arrays on the calls of `armed_calls`.  Checked when the third call
    has returned and BEFORE any svo_sync - the first call's two frames are with the caller (include/svo.h: "once the second
    following host-fed call has returned"), complete and byte for byte, and nothing was written for a call that was not armed -
    and again after svo_sync, all six frames and the result records."""
    want, rec_off, _, _ = fx.want()
    wl, wc, wd = dyn_want(fx)
    ctx = fx.new_ctx(dyn=dyn_params(pkg))
    raw = np.full(N * K * 32 + 80, GUARD, np.uint8)
    obs = raw[(-raw.ctypes.data) % 16:][:N * K * 32 + 64]
    counts = np.full(N + 4, -1, np.int32)
    lists = np.full(N * 512 * 8 + 64, GUARD, np.uint8)
    cnt = np.full(N + 4, -1, np.int32); drp = np.full(N + 4, -7, np.int32)
    res = np.zeros(N, pkg.TRACK_DTYPE)
    aL, aR = np.ascontiguousarray(fx.L), np.ascontiguousarray(fx.R)
    armed = [c in armed_calls for c in range(3) for _ in range(2)]

    def check_frames(frames):
        """frames 0 .. frames - 1 as delivered (or, not armed, untouched); every frame behind them untouched if its call was not armed"""
        check(obs[:frames * K * 32], counts[:frames], want, range(frames), armed=armed[:frames], extra=0)
        for k in range(N):
            mine = lists[k * 512 * 8:(k + 1) * 512 * 8]
            if not armed[k]:
                assert (obs[k * K * 32:(k + 1) * K * 32] == GUARD).all() and counts[k] == -1, k
                assert (mine == GUARD).all() and cnt[k] == -1 and drp[k] == -7, k
            elif k < frames:
                assert cnt[k] == wc[k] and drp[k] == wd[k], (k, cnt[k], wc[k], drp[k], wd[k])
                assert mine[:cnt[k] * 8].tobytes() == wl[k, :wc[k]].tobytes(), k
        assert (obs[N * K * 32:] == GUARD).all() and (lists[N * 512 * 8:] == GUARD).all()
        assert (counts[N:] == -1).all() and (cnt[N:] == -1).all() and (drp[N:] == -7).all()

    for c in range(3):
        f0 = 2 * c
        if c in armed_calls:
            ctx.track_map_out(obs[f0 * K * 32:], counts[f0:])
            ctx.track_dynamic_out(lists[f0 * 512 * 8:], cnt[f0:], drp[f0:])
        ctx.track_batch_host(aL[f0:].ctypes.data, aR[f0:].ctypes.data, W, 2, res[f0:], boxes=pkg.boxes_host(fx.hb[f0:f0 + 2], fx.hn[f0:f0 + 2]))
    check_frames(2)     # (no svo_sync yet)
    ctx.sync()
    ctx.close()
    check_frames(N)
    assert res.tobytes() == rec_off


@pytest.mark.gpu
def test_host_fed_set_reuse(pkg, fx):
    """both attachments armed on each of three host-fed calls: the third call stages in the pinned set of the first, whose two
    frames reach the caller's arrays first - before any svo_sync"""
    host_fed_three_calls(pkg, fx, armed_calls=(0, 1, 2))


@pytest.mark.gpu
def test_host_fed_armed_once(pkg, fx):
    """both attachments armed on the first of three host-fed calls only: its two frames are with the caller when the third call
    has returned, before any svo_sync, though no later armed call reuses the pinned set; the other calls' arrays stay untouched"""
    host_fed_three_calls(pkg, fx, armed_calls=(0,))


def tail_call(fx, ctx, f0, b, obs, counts, res, arm=True):
    if arm:
        ctx.track_map_out(obs.data_ptr() + f0 * K * 32, counts.data_ptr() + 4 * f0)
    ctx.track_tail_dev(fx.fe_kp.data_ptr() + f0 * K * 28, fx.fe_desc.data_ptr() + f0 * K * 32, fx.fe_n.data_ptr() + 4 * f0,
                       fx.fe_depth.data_ptr() + f0 * K * 4, K, b, res.data_ptr() + f0 * fx.rec, boxes=fx.boxes(f0))


@pytest.mark.gpu
def test_tail_entry_fed_the_front_end_arrays(pkg, fx):
    torch = fx.torch
    want, rec_off, _, _ = fx.want()
    ctx = fx.new_ctx()
    obs, counts = guarded(fx, N)
    res = torch.zeros((N, fx.rec), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    tail_call(fx, ctx, 0, 2, obs, counts, res)
    tail_call(fx, ctx, 2, 4, obs, counts, res)
    ctx.sync()
    torch.cuda.synchronize()
    ctx.close()
    check(obs.cpu().numpy(), counts.cpu().numpy(), want, range(N))
    assert res.cpu().numpy().tobytes() == rec_off


@pytest.mark.gpu
def test_hand_made_edges_through_the_tail_entry(pkg, fx):
    """max_kp 96 (one and a half waves), kp_stride 128 > max_kp, calls of B = 1 and B = 3 over hand-made front-end arrays:
    frame 0 has max_kp keypoints, all with depth (max_kp records, all new); frame 1 the same keypoints, depths all <= 0 (matched
    records only); frame 2 no keypoint (count 0, nothing written); frame 3 four known descriptors and twelve fresh ones (fewer than
    5 correspondences: PnP fails; the fresh ones become points).  Guard bytes around every list."""
    torch = fx.torch
    MK, KS, F = 96, 128, 4
    rng = np.random.default_rng(5)
    kp = np.zeros((F, KS), pkg.KP_DTYPE); desc = np.zeros((F, KS, 32), np.uint8); depth = np.full((F, KS), -1, np.float32)
    n = np.array([MK, MK, 0, 16], np.int32)
    kp["x"][0, :MK] = rng.uniform(40, 600, MK).astype(np.float32); kp["y"][0, :MK] = rng.uniform(40, 200, MK).astype(np.float32)
    kp["size"] = 31
    desc[0, :MK] = rng.integers(0, 256, (MK, 32), dtype=np.uint8); depth[0, :MK] = rng.uniform(5, 40, MK).astype(np.float32)
    kp[1] = kp[0]; desc[1] = desc[0]; depth[1, :MK] = np.where(np.arange(MK) % 2 == 0, 0.0, -1.0)
    kp[3, :4] = kp[0, 10:14]; desc[3, :4] = desc[0, 10:14]; depth[3, :4] = depth[0, 10:14]
    kp["x"][3, 4:16] = rng.uniform(40, 600, 12).astype(np.float32); kp["y"][3, 4:16] = rng.uniform(40, 200, 12).astype(np.float32)
    desc[3, 4:16] = rng.integers(0, 256, (12, 32), dtype=np.uint8); depth[3, 4:16] = rng.uniform(5, 40, 12).astype(np.float32)
    d_kp = torch.from_numpy(kp.view(np.uint8).reshape(F, KS, 28)).cuda(); d_desc = torch.from_numpy(desc).cuda()
    d_n = torch.from_numpy(n).cuda(); d_depth = torch.from_numpy(depth).cuda()

    def run(arm):
        ctx = pkg.Svo(640, 240, max_kp=MK, max_batch=4)
        ctx.track_reset(fx.cam)
        obs, counts = guarded(fx, F, k=MK)
        res = torch.zeros((F, fx.rec), dtype=torch.uint8, device="cuda")
        dbg = np.zeros(F, pkg.TRACK_DEBUG_DTYPE)
        torch.cuda.synchronize()
        for f0, b in ((0, 1), (1, 3)):
            if arm:
                ctx.track_map_out(obs.data_ptr() + f0 * MK * 32, counts.data_ptr() + 4 * f0)
            ctx.track_tail_dev(d_kp.data_ptr() + f0 * KS * 28, d_desc.data_ptr() + f0 * KS * 32, d_n.data_ptr() + 4 * f0,
                               d_depth.data_ptr() + f0 * KS * 4, KS, b, res.data_ptr() + f0 * fx.rec)
            if not arm:
                dbg[f0:f0 + b] = ctx.debug_track_frames(0, b)
        ctx.sync()
        torch.cuda.synchronize()
        ctx.close()
        return obs.cpu().numpy(), counts.cpu().numpy(), res.cpu().numpy().reshape(-1).view(pkg.TRACK_DTYPE), dbg

    _, _, rec, dbg = run(False)
    pos, want = {}, []
    for k in range(F):
        xy = np.stack([kp["x"][k], kp["y"][k]], 1)[:n[k]]
        want.append(map_ref.expected(k, dbg[k]["match_gid"], dbg[k]["new_gid"], xy, depth[k, :n[k]], fx.cam4, rec[k]["Tcw"], pos))
    assert len(want[0]) == MK and (want[0]["flags"] == 1).all()
    assert len(want[1]) >= 5 and (want[1]["flags"] == 0).all(), "frame 1 must have matched records and nothing else"
    assert len(want[2]) == 0
    assert 0 < (want[3]["flags"] == 0).sum() < 5 and (want[3]["flags"] == 1).sum() == 12 and rec[3]["n_lm_edges"] < 5
    obs, counts, rec_on, _ = run(True)
    check(obs, counts, want, range(F), k=MK)
    assert rec_on.tobytes() == rec.tobytes()


@pytest.mark.gpu
def test_sgbm_depth_source(pkg, fx):
    """depth_source 3: a call's tail is enqueued chunk by chunk, other keypoints have depth; two calls"""
    want, rec_off, _, z = fx.want(depth_source=3)
    assert any(not np.array_equal(z[k], fx.depth[k, :len(z[k])]) for k in range(N)), "the dense depths must differ from the sparse ones"
    ctx = fx.new_ctx(depth_source=3)
    obs, counts, rec = run_dev(fx, ctx, splits=(4, 2))
    ctx.close()
    check(obs, counts, want, range(N))
    assert rec == rec_off


@pytest.mark.gpu
def test_with_the_dynamic_loop(pkg, fx):
    """the dynamic-keypoint loop on, both attachments armed for every call: the map records are those of the loop switched off,
    the dynamic lists those of a run without the map attachment"""
    torch = fx.torch
    want, rec_off, _, _ = fx.want()
    p = pkg.dyn_default_params()
    p.enable, p.max_pts = 1, 512

    def dyn_arrays():
        return (torch.zeros((N, 512, 2), dtype=torch.float32, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda"),
                torch.full((N,), -7, dtype=torch.int32, device="cuda"))
    lists = []
    for arm in ((True, True), (False, False)):
        d = dyn_arrays()
        ctx = fx.new_ctx(dyn=p)
        obs, counts, rec = run_dev(fx, ctx, splits=(2, 4), arm=arm, dyn_out=d)
        ctx.close()
        assert rec == rec_off
        if arm[0]:
            check(obs, counts, want, range(N))
        lists.append(tuple(a.cpu().numpy() for a in d))
    # (a list's used entries, as tests/test_dynamic_dev_gpu.py compares them: what lies behind counts[k] is never defined)
    (la, ca, da), (lb, cb, db) = lists
    assert np.array_equal(ca, cb) and np.array_equal(da, db) and ca[N - 1] > 0
    for k in range(N):
        assert la[k, :ca[k]].tobytes() == lb[k, :ca[k]].tobytes(), k


@pytest.mark.gpu
def test_refusals_and_one_shot(pkg, fx):
    torch = fx.torch
    lib = pkg.load_library()
    want, rec_off, _, _ = fx.want()
    obs, counts = guarded(fx, N)
    res = torch.zeros((N, fx.rec), dtype=torch.uint8, device="cuda")
    po, pc = C.c_void_p(obs.data_ptr()), C.c_void_p(counts.data_ptr())
    ctx = pkg.Svo(W, H, max_batch=N)
    assert lib.svo_track_map_out(ctx.h, po, pc) == -1 and b"svo_track_reset" in lib.svo_last_error(ctx.h)   # before any reset
    ctx.track_reset(fx.cam)
    assert lib.svo_track_map_out(None, po, pc) == -1
    assert lib.svo_track_map_out(ctx.h, None, pc) == -1
    assert lib.svo_track_map_out(ctx.h, po, None) == -1
    assert lib.svo_track_map_out(ctx.h, C.c_void_p(obs.data_ptr() + 4), pc) == -1      # (two 16-byte stores per record)
    # armed: the entries that do not deliver it refuse by name, enqueue nothing, leave the context usable and the attachment armed
    ctx.track_map_out(obs.data_ptr(), counts.data_ptr())
    with pytest.raises(pkg.SvoError, match="svo_track_multi_step_dev"):
        ctx.track_multi_step_dev(fx.dL.data_ptr(), fx.dR.data_ptr(), PITCH, 1, res.data_ptr())
    with pytest.raises(pkg.SvoError, match="svo_track_sharded_dev"):
        pkg.Svo.track_sharded_dev([ctx], [fx.dL.data_ptr()], [fx.dR.data_ptr()], PITCH, N, res.data_ptr())
    with pytest.raises(pkg.SvoError, match="svo_track_sharded_host"):
        pkg.Svo.track_sharded_host([ctx], np.ascontiguousarray(fx.L), np.ascontiguousarray(fx.R), W, N, np.zeros(N, pkg.TRACK_DTYPE))
    ctx.sync()
    torch.cuda.synchronize()
    assert (obs.cpu().numpy() == GUARD).all()
    ctx.track_batch_dev(fx.dL.data_ptr(), fx.dR.data_ptr(), PITCH, 3, res.data_ptr(), boxes=fx.boxes(0))     # still armed: delivers
    # one-shot: the next call writes nothing
    ctx.track_batch_dev(fx.dL.data_ptr() + 3 * H * PITCH, fx.dR.data_ptr() + 3 * H * PITCH, PITCH, 3, res.data_ptr() + 3 * fx.rec,
                        boxes=fx.boxes(3))
    ctx.sync()
    torch.cuda.synchronize()
    check(obs.cpu().numpy(), counts.cpu().numpy(), want, range(N), armed=[True] * 3 + [False] * 3)
    assert res.cpu().numpy().tobytes() == rec_off
    # a reset disarms
    ctx.track_map_out(obs.data_ptr() + 3 * K * 32, counts.data_ptr() + 12)
    ctx.track_reset(fx.cam)
    ctx.track_batch_dev(fx.dL.data_ptr(), fx.dR.data_ptr(), PITCH, 1, res.data_ptr(), boxes=fx.boxes(0))
    ctx.sync()
    torch.cuda.synchronize()
    assert (obs.cpu().numpy()[3 * K * 32:] == GUARD).all()
    ctx.close()
