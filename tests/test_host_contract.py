"""What include/svo.h promises the HOST, beyond the records themselves:

- host-fed calls (svo_track_batch_host, svo_track_batch_bgr_host, svo_frontend_batch_host): the outputs of call c are complete,
  and its pinned source images may be reused, once the second following host-fed call on the context has returned - without
  an svo_sync, whatever kind the calls in between are;
- a bounded wait inside the pose chain that runs out (test switch "debug_lose_sample") is reported by svo_sync as
  SVO_E_TIMEOUT once per svo_track_reset, for one sequence and for many, and the sticky flag says 4 until the next reset.

Every record is compared with svo_track_batch_dev's (or svo_frontend_batch_dev's) on the same resident frames, byte for byte."""
import importlib
import re

import numpy as np
import pytest

from test_hostfeed import PITCH, boxes_of, pin, reference

N = 64
CALL = 16          # frames per host-fed call: ~1.7 ms of pose chain, longer than a call takes to enqueue


@pytest.fixture(scope="module")
def seq(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    dev = torch.device("cuda", 0)
    L, R, _ = synth.render_sequence(N, device=dev)
    H, W = int(L.shape[1]), int(L.shape[2])
    dL = torch.zeros((N, H, PITCH), dtype=torch.uint8, device=dev); dR = torch.zeros_like(dL)
    dL[:, :, :W] = L; dR[:, :, :W] = R
    cam = pkg.Camera(**pkg.KITTI_00_02)
    return dict(dL=dL, dR=dR, W=W, H=H, cam=cam, dev=dev,
                hL=dL.cpu().numpy(), hR=dR.cpu().numpy(),                       # pitch 1280 (= the library's staging pitch)
                pL=np.ascontiguousarray(L.cpu().numpy()), pR=np.ascontiguousarray(R.cpu().numpy()))   # packed, stride = W


def pinned_records(pkg, n):
    """n records' worth of pinned host memory, every byte 0xFF"""
    import torch
    t = torch.full((n * pkg.TRACK_DTYPE.itemsize,), 0xFF, dtype=torch.uint8).pin_memory()
    assert t.is_pinned()
    return t


def frontend_reference(pkg, s, k0, B):
    """svo_frontend_batch_dev on resident frames k0 .. k0 + B - 1: (kp, desc, n, uR, depth) on the host"""
    import torch
    K, dev = 500, s["dev"]
    ref = pkg.Svo(s["W"], s["H"], max_batch=B)
    kp = torch.zeros((B, K, pkg.KP_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    desc = torch.zeros((B, K, 32), dtype=torch.uint8, device=dev)
    n = torch.zeros(B, dtype=torch.int32, device=dev)
    uR = torch.zeros((B, K), dtype=torch.float32, device=dev)
    depth = torch.zeros((B, K), dtype=torch.float32, device=dev)
    fb = s["H"] * PITCH
    ref.frontend_batch_dev(s["dL"].data_ptr() + k0 * fb, s["dR"].data_ptr() + k0 * fb, PITCH, B, s["cam"], d_kpL=kp.data_ptr(),
                           d_descL=desc.data_ptr(), d_nL=n.data_ptr(), d_uR=uR.data_ptr(), d_depth=depth.data_ptr())
    ref.sync(); ref.close()
    return (kp.cpu().numpy().view(pkg.KP_DTYPE).reshape(B, K), desc.cpu().numpy(), n.cpu().numpy(), uR.cpu().numpy(), depth.cpu().numpy())


def frontend_outputs(pkg, B):
    K = 500
    return (np.zeros((B, K), pkg.KP_DTYPE), np.zeros((B, K, 32), np.uint8), np.full(B, -1, np.int32),
            np.zeros((B, K), np.float32), np.zeros((B, K), np.float32))


def assert_frontend_equal(got, want):
    gk, gd, gn, gu, gz = got
    wk, wd, wn, wu, wz = want
    assert np.array_equal(gn, wn) and wn.min() > 100
    for f in range(len(wn)):
        m = int(wn[f])
        assert gk[f, :m].tobytes() == wk[f, :m].tobytes(), f
        assert np.array_equal(gd[f, :m], wd[f, :m]), f
        assert np.array_equal(gu[f, :m].view(np.uint32), wu[f, :m].view(np.uint32)), f
        assert np.array_equal(gz[f, :m].view(np.uint32), wz[f, :m].view(np.uint32)), f


def camera_centre(r):
    T = r["Tcw"].reshape(4, 4).astype(np.float64)
    return -T[:3, :3].T @ T[:3, 3]


def assert_tracks_on(got, want, k):
    """a frame after a lost sample: tracked (PnP consensus found), a pose within a few centimetres of the undisturbed run's"""
    assert got["n_pnp_inliers"] > 4 and got["frame_id"] == want["frame_id"], k
    assert np.linalg.norm(camera_centre(got) - camera_centre(want)) < 0.1, k


# ---- host-fed calls: the "second following call" -------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["gray", "gray_boxes", "bgr"])
def test_pinned_records_are_complete_when_the_second_following_call_returns(pkg, seq, kind):
    """Records written straight into pinned memory (pre-filled with 0xFF), four calls of 16 frames from pinned sources: call c's
    records are read as soon as call c + 2 has returned, BEFORE any svo_sync, and must already be the resident tracker's.  Without
    boxes nothing else in a call waits for the set's previous use; bgr: B = G = R copies of the gray frames (the same records)."""
    s = seq
    sizes = [CALL] * 4
    n = sum(sizes)
    rec = pkg.TRACK_DTYPE.itemsize
    want = reference(pkg, s, sizes, boxes=kind == "gray_boxes")
    if kind == "bgr":
        aL, aR = (np.ascontiguousarray(np.repeat(a[:n, :, :, None], 3, axis=3)) for a in (s["pL"], s["pR"]))
        stride = 3 * s["W"]
    else:
        aL, aR, stride = s["hL"][:n], s["hR"][:n], PITCH
    tL, tR = pin(aL), pin(aR)
    res = pinned_records(pkg, n)
    ctx = pkg.Svo(s["W"], s["H"], max_batch=CALL)
    ctx.track_reset(s["cam"])
    call = ctx.track_batch_bgr_host if kind == "bgr" else ctx.track_batch_host
    fb = s["H"] * stride
    offs = [sum(sizes[:c]) for c in range(len(sizes))]
    early, keep = {}, []
    for c, B in enumerate(sizes):
        k0 = offs[c]
        bx = None
        if kind == "gray_boxes":
            bx = pkg.boxes_host(np.array([boxes_of(k) for k in range(k0, k0 + B)], np.int32), np.full(B, 2, np.int32))
            keep.append(bx)
        call(tL.data_ptr() + k0 * fb, tR.data_ptr() + k0 * fb, stride, B, res.data_ptr() + k0 * rec, boxes=bx)
        if c >= 2:
            a, b = offs[c - 2], offs[c - 2] + sizes[c - 2]
            early[c - 2] = res.numpy()[a * rec:b * rec].tobytes()   # (no svo_sync yet)
    ctx.sync()
    assert ctx.track_overflowed() == 0
    ctx.close()
    assert res.numpy().tobytes() == want
    for c, got in early.items():
        a, b = offs[c], offs[c] + sizes[c]
        assert got == want[a * rec:b * rec], ("call", c, "read after call", c + 2, "returned")


@pytest.mark.gpu
def test_pinned_track_sources_may_be_overwritten_after_the_second_following_call(pkg, seq):
    """Pinned sources and pinned records: as soon as call c + 2 has returned, call c's source frames are overwritten in place with
    noise.  The records (read after svo_sync) must be the resident tracker's on the original frames."""
    s = seq
    sizes = [CALL] * 4
    n = sum(sizes)
    rec = pkg.TRACK_DTYPE.itemsize
    want = reference(pkg, s, sizes)
    tL, tR = pin(np.array(s["hL"][:n])), pin(np.array(s["hR"][:n]))
    noise = np.random.default_rng(5).integers(0, 256, (CALL,) + s["hL"].shape[1:], dtype=np.uint8)
    res = pinned_records(pkg, n)
    ctx = pkg.Svo(s["W"], s["H"], max_batch=CALL)
    ctx.track_reset(s["cam"])
    fb = s["H"] * PITCH
    offs = [sum(sizes[:c]) for c in range(len(sizes))]
    for c, B in enumerate(sizes):
        k0 = offs[c]
        ctx.track_batch_host(tL.data_ptr() + k0 * fb, tR.data_ptr() + k0 * fb, PITCH, B, res.data_ptr() + k0 * rec)
        if c >= 2:
            a, b = offs[c - 2], offs[c - 2] + sizes[c - 2]
            tL.numpy()[a:b] = noise[:b - a]
            tR.numpy()[a:b] = noise[:b - a]
    ctx.sync()
    assert ctx.track_overflowed() == 0
    ctx.close()
    assert res.numpy().tobytes() == want


@pytest.mark.gpu
def test_pinned_front_end_sources_may_be_overwritten_after_the_second_following_call(pkg, seq):
    """svo_frontend_batch_host from pinned sources: call c's frames overwritten with noise once call c + 2 has returned; the
    outputs (after svo_sync) must be svo_frontend_batch_dev's on the original frames."""
    s = seq
    sizes = [CALL] * 4
    n = sum(sizes)
    want = [frontend_reference(pkg, s, c * CALL, CALL) for c in range(len(sizes))]
    tL, tR = pin(np.array(s["hL"][:n])), pin(np.array(s["hR"][:n]))
    noise = np.random.default_rng(6).integers(0, 256, (CALL,) + s["hL"].shape[1:], dtype=np.uint8)
    got = [frontend_outputs(pkg, CALL) for _ in sizes]
    ctx = pkg.Svo(s["W"], s["H"], max_batch=CALL)
    fb = s["H"] * PITCH
    for c, B in enumerate(sizes):
        k0 = c * CALL
        kp, desc, nn, uR, depth = got[c]
        ctx.frontend_batch_host(tL.data_ptr() + k0 * fb, tR.data_ptr() + k0 * fb, PITCH, B, s["cam"], kpL=kp, descL=desc, nL=nn,
                                uR=uR, depth=depth)
        if c >= 2:
            a = (c - 2) * CALL
            tL.numpy()[a:a + CALL] = noise
            tR.numpy()[a:a + CALL] = noise
    ctx.sync()
    ctx.close()
    for c in range(len(sizes)):
        assert_frontend_equal(got[c], want[c])


@pytest.mark.gpu
def test_host_fed_calls_of_different_kinds_share_the_parity(pkg, seq):
    """A pinned svo_track_batch_host call, an svo_frontend_batch_host call, a second svo_track_batch_host call on one context: the
    first call's records (pinned, 0xFF before) are complete when the third call returns; after svo_sync the tracker's records and
    the front end's outputs are the resident entries'."""
    s = seq
    rec = pkg.TRACK_DTYPE.itemsize
    want = reference(pkg, s, [CALL, CALL])
    want_fe = frontend_reference(pkg, s, 2 * CALL, CALL)
    tL, tR = pin(s["hL"][:3 * CALL]), pin(s["hR"][:3 * CALL])
    res = pinned_records(pkg, 2 * CALL)
    fe = frontend_outputs(pkg, CALL)
    ctx = pkg.Svo(s["W"], s["H"], max_batch=CALL)
    ctx.track_reset(s["cam"])
    fb = s["H"] * PITCH
    ctx.track_batch_host(tL.data_ptr(), tR.data_ptr(), PITCH, CALL, res.data_ptr())
    kp, desc, nn, uR, depth = fe
    ctx.frontend_batch_host(tL.data_ptr() + 2 * CALL * fb, tR.data_ptr() + 2 * CALL * fb, PITCH, CALL, s["cam"], kpL=kp, descL=desc,
                            nL=nn, uR=uR, depth=depth)
    ctx.track_batch_host(tL.data_ptr() + CALL * fb, tR.data_ptr() + CALL * fb, PITCH, CALL, res.data_ptr() + CALL * rec)
    first = res.numpy()[:CALL * rec].tobytes()   # (no svo_sync yet)
    ctx.sync()
    assert ctx.track_overflowed() == 0
    ctx.close()
    assert res.numpy().tobytes() == want
    assert first == want[:CALL * rec]
    assert_frontend_equal(fe, want_fe)


# ---- timeouts: reported once per reset, for any number of sequences ------------------------------------------------------

def _resident_run(pkg, s, ctx, n, cuts, lose_call=None):
    """track_batch_dev over frames 0 .. n - 1 in calls of `cuts`, svo_sync after each; call `lose_call` runs with
    "debug_lose_sample" = 3 and its svo_sync must report SVO_E_TIMEOUT (once).  Returns the records."""
    import torch
    rec = pkg.TRACK_DTYPE.itemsize
    fb = s["H"] * PITCH
    out = torch.zeros((n, rec), dtype=torch.uint8, device=s["dev"])
    k0 = 0
    for c, B in enumerate(cuts):
        if c == lose_call:
            ctx.set_option("debug_lose_sample", 3)      # sample 2 of every fused pose launch of this call never reports
        ctx.track_batch_dev(s["dL"].data_ptr() + k0 * fb, s["dR"].data_ptr() + k0 * fb, PITCH, B, out.data_ptr() + k0 * rec)
        if c == lose_call:
            ctx.set_option("debug_lose_sample", 0)
            with pytest.raises(pkg.SvoError, match="timed out"):
                ctx.sync()
            assert ctx.track_overflowed() == 4
            ctx.sync()                                      # (reported once)
        else:
            ctx.sync()
        k0 += B
    return out.cpu().numpy().view(pkg.TRACK_DTYPE).reshape(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("depth_source", [0, 1])
def test_timeout_is_reported_again_after_a_reset(pkg, seq, depth_source):
    """One sequence (depth_source 0: samples and frame part in one launch; 1: beside the dense stage, the first 8 samples in a
    launch of their own - "tail_semi").  A lost sample is reported by svo_sync; after svo_track_reset and "tail_fused" = 1 again a
    second lost sample must be reported again.  The sticky flag is 0 right after each reset and 4 after each event; the lost
    frame is a PnP failure, the frames before it are the undisturbed run's, the frames after it are tracked."""
    s = seq
    n, cuts = 7, [3, 1, 3]
    ref = pkg.Svo(s["W"], s["H"], max_batch=3)
    ref.set_option("depth_source", depth_source)
    ref.track_reset(s["cam"])
    want = _resident_run(pkg, s, ref, n, cuts)
    assert ref.track_overflowed() == 0
    ref.close()
    ctx = pkg.Svo(s["W"], s["H"], max_batch=3)
    ctx.set_option("depth_source", depth_source)
    for rep in range(2):
        ctx.track_reset(s["cam"])
        assert ctx.track_overflowed() == 0, rep
        if rep:
            ctx.set_option("tail_fused", 1)                 # (the first report switched the fused launch off)
        got = _resident_run(pkg, s, ctx, n, cuts, lose_call=1)
        for k in range(3):
            assert got[k].tobytes() == want[k].tobytes(), (rep, k)
        assert got[3]["n_pnp_inliers"] == -1 and got[3]["frame_id"] == 3, rep
        for k in range(4, n):
            assert_tracks_on(got[k], want[k], (rep, k))
    ctx.close()


@pytest.mark.gpu
def test_timeout_in_the_many_sequence_pose_chain_is_reported(pkg, seq):
    """Eight sequences, "tail_semi" = 2 (each step's pose chains: the first 8 samples of every sequence, then the other samples and
    the frame parts in one launch), one step with a lost sample.  svo_sync reports SVO_E_TIMEOUT once and names the sequences
    concerned: those that ran RANSAC in that step.  Two sequences get a blank pair in that step (no keypoints, nothing to wait
    for): all their records equal the undisturbed run's.  The others: records before the step equal, a PnP failure in it, tracked
    after it."""
    import torch
    s = seq
    S, STEPS, LOST, BLANK = 8, 5, 2, (6, 7)
    H, W, dev = s["H"], s["W"], s["dev"]
    rec = pkg.TRACK_DTYPE.itemsize
    idx = torch.tensor([[(q % 3) + t for q in range(S)] for t in range(STEPS)], device=dev)
    mL = s["dL"][idx.reshape(-1)].reshape(STEPS, S, H, PITCH).contiguous()
    mR = s["dR"][idx.reshape(-1)].reshape(STEPS, S, H, PITCH).contiguous()
    for q in BLANK:
        mL[LOST, q] = 0; mR[LOST, q] = 0
    torch.cuda.synchronize()

    def run(lose):
        m = pkg.Svo(W, H, max_batch=S)
        m.set_option("tail_semi", 2)
        m.track_multi_reset(S, s["cam"])
        assert m.track_overflowed() == 0
        out = torch.zeros((STEPS, S, rec), dtype=torch.uint8, device=dev)
        err = None
        for t in range(STEPS):
            if lose and t == LOST:
                m.set_option("debug_lose_sample", 3)
            m.track_multi_step_dev(mL[t].data_ptr(), mR[t].data_ptr(), PITCH, S, out[t].data_ptr())
            if lose and t == LOST:
                m.set_option("debug_lose_sample", 0)
                with pytest.raises(pkg.SvoError, match="timed out") as ei:
                    m.sync()
                err = str(ei.value)
                assert m.track_overflowed() == 4
                m.sync()                                    # (reported once)
        m.sync()
        if not lose:
            assert m.track_overflowed() == 0
        m.close()
        return out.cpu().numpy().view(pkg.TRACK_DTYPE).reshape(STEPS, S), err

    want, _ = run(False)
    got, err = run(True)
    ran = [q for q in range(S) if q not in BLANK]
    for q in ran:
        assert want[LOST, q]["n_pnp_inliers"] > 4, q         # (the undisturbed run found a consensus in that step)
    affected = sorted(q for q in range(S) if got[LOST, q]["n_pnp_inliers"] == -1)
    assert affected == ran, affected
    named = re.search(r"sequence\(s\) ([0-9, ]+) of %d" % S, err)
    assert named, err
    assert sorted(int(v) for v in named.group(1).replace(",", " ").split()) == affected, err
    for q in BLANK:
        for t in range(STEPS):
            assert got[t, q].tobytes() == want[t, q].tobytes(), (q, t)
    for q in ran:
        for t in range(LOST):
            assert got[t, q].tobytes() == want[t, q].tobytes(), (q, t)
        for t in range(LOST + 1, STEPS):
            assert_tracks_on(got[t, q], want[t, q], (q, t))
