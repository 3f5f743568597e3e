"""The hand-over from the RANSAC samples to the LM in the fused pose launch (k_tp_tail_ord), and the LM with its first chunk of
edges held in registers: nothing of it may change a bit of any result."""
import importlib

import numpy as np
import pytest

import util

LM_SIZES = [1, 5, 63, 64, 65, 127, 128, 129, 300, 512]   # one lane, one wave, two edges per lane, the chunk boundary (128), more chunks
KITTI_K = (718.856, 718.856, 607.1928, 185.2157)


def lm_problem(n):
    """n points 5..60 m in front of a known pose, observed with 0.5 px noise, every tenth edge 8 px off (Huber's linear branch:
    delta^2 = 5.991); the start pose is the true one moved by 2 cm and turned by 0.5 degrees."""
    rng = np.random.default_rng(1000 + n)
    fx, fy, cx, cy = KITTI_K
    u = rng.uniform(40, 1200, n); v = rng.uniform(40, 340, n); z = rng.uniform(5, 60, n)
    Xc = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)

    def rot(axis, ang):
        k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
    R = rot([0.3, -1.0, 0.2], 0.02)
    t = np.array([0.05, -0.02, -0.8])
    Xw = (R.T @ (Xc - t).T).T
    obs = np.stack([u, v], 1) + rng.normal(0, 0.5, (n, 2))
    out = np.arange(n) % 10 == 9
    ang = rng.uniform(0, 2 * np.pi, n)
    obs[out] += 8.0 * np.stack([np.cos(ang), np.sin(ang)], 1)[out]
    T0 = np.eye(4)
    T0[:3, :3] = rot([1.0, 1.0, -1.0], np.deg2rad(0.5)) @ R
    d = np.array([1.0, -2.0, 2.0]); d *= 0.02 / np.linalg.norm(d)
    T0[:3, 3] = t + d
    Xw = Xw.astype(np.float32).astype(np.float64)   # world points and keypoints are CV_32F in the reference
    obs = obs.astype(np.float32).astype(np.float64)
    return Xw, obs, np.array(KITTI_K, np.float64), T0


def lm_bits(T, st):
    return (np.ascontiguousarray(T, np.float64).tobytes(), st.n_edges, st.iterations, st.trials_total, st.terminated,
            np.float64(st.chi2_initial).tobytes(), np.float64(st.chi2_final).tobytes(), np.float64(st.lambda_final).tobytes())


@pytest.fixture(scope="module")
def lm_oracle(orc):
    """the oracle's pose optimisation of every case, computed once"""
    out = {}
    for n in LM_SIZES:
        Xw, obs, K, T0 = lm_problem(n)
        Tr, sr, _ = orc.pose_opt(Xw, obs, K, T0)
        out[n] = (Xw, obs, K, T0, Tr, sr)
    return out


@pytest.mark.parametrize("n", LM_SIZES)
def test_lm_cases_converge_on_the_oracle(lm_oracle, n):
    """(CPU) every case of the register-resident-edge test does something: a finite pose after at least 2 LM iterations, and from
    n = 10 on at least one edge beyond Huber's delta at the solution."""
    Xw, obs, K, T0, Tr, sr = lm_oracle[n]
    assert sr.n_edges == n and sr.iterations >= 2, (n, sr.iterations)
    assert np.isfinite(Tr).all() and np.isfinite(sr.chi2_final)
    assert not np.array_equal(Tr, T0)
    if n >= 10:
        pc = (Tr[:3, :3] @ Xw.T).T + Tr[:3, 3]
        e = obs - np.stack([pc[:, 0] / pc[:, 2] * K[0] + K[2], pc[:, 1] / pc[:, 2] * K[1] + K[3]], 1)
        assert ((e * e).sum(1) > 5.991).any()


@pytest.mark.gpu
@pytest.mark.parametrize("n", LM_SIZES)
def test_lm_with_register_resident_edges_equals_the_one_lane_loop_and_the_oracle(pkg, lm_oracle, n):
    """svo_pose_opt with the first chunk's correspondences in registers ("pose_mfma" = 1 and 2) against the one-lane checker (0),
    which reads every edge from memory, and against the oracle: pose and svo_lm_stats byte for byte."""
    Xw, obs, K, T0, Tr, sr = lm_oracle[n]
    svo = pkg.Svo(640, 240)
    got = {}
    for mode in (0, 1, 2):
        svo.set_option("pose_mfma", mode)
        T, st = svo.pose_opt(Xw, obs, K, T0)
        got[mode] = lm_bits(T, st)
    svo.close()
    assert got[1] == got[0] and got[2] == got[0], n
    assert got[0] == lm_bits(Tr, sr), n


# ---- the fused launch against the two-launch chain ------------------------------------------------------------------
# 192 frames: the synthetic drive's first frame that the eight awaited samples do not decide is frame 146 (9 samples visited; 149 and
# 150 follow with 14 and 11) - its first 64 and 128 frames hold none, and the coverage test below needs one
N_FRAMES = 192
CHUNKS = (64, 16, 1)
DBG_FIELDS = ("pnp_best", "pnp_iterations", "pnp_inliers", "pnp_ok", "T_pnp")


@pytest.fixture(scope="module")
def handover_runs(pkg):
    """N_FRAMES full-size frames rendered on the device, tracked with the fused pose launch ("tail_fused" = 1, the default) and
    with the two-launch chain (0), in calls of 64, 16 and 1 frames: records and svo_debug_track_frames of every frame."""
    import torch
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    dev = torch.device("cuda", 0)
    N = N_FRAMES
    L, R, _ = synth.render_sequence(N, device=dev)
    H, W = int(L.shape[1]), int(L.shape[2])
    pitch = 1280
    dL = torch.zeros((N, H, pitch), dtype=torch.uint8, device=dev); dR = torch.zeros_like(dL)
    dL[:, :, :W] = L.to(dev); dR[:, :, :W] = R.to(dev)
    cam = pkg.Camera(**pkg.KITTI_00_02)
    rec = pkg.TRACK_DTYPE.itemsize
    fb = H * pitch
    runs = {}
    for chunk in CHUNKS:
        for fused in (1, 0):
            s = pkg.Svo(W, H, max_batch=chunk)
            s.set_option("tail_fused", fused)
            s.track_reset(cam)
            res = torch.zeros((N, rec), dtype=torch.uint8, device=dev)
            dbg = []
            for off in range(0, N, chunk):
                s.track_batch_dev(dL.data_ptr() + off * fb, dR.data_ptr() + off * fb, pitch, chunk, res.data_ptr() + off * rec)
                dbg.append(s.debug_track_frames(0, chunk).copy())
            s.sync()
            assert s.track_overflowed() == 0, (chunk, fused)
            runs[(chunk, fused)] = (res.cpu().numpy().tobytes(), np.concatenate(dbg))
            s.close()
    return runs


@pytest.mark.gpu
def test_the_sequence_reaches_every_path_of_the_handover(pkg, handover_runs):
    """(on the two-launch run) the frames exercise what the fused hand-over distinguishes: a frame the awaited samples do not decide
    (more than 8 samples visited), winners at three different samples among the frames they do decide, and frame 0 (no RANSAC)."""
    rec_bytes, dbg = handover_runs[(64, 0)]
    r = np.frombuffer(rec_bytes, pkg.TRACK_DTYPE)
    it, best = dbg["pnp_iterations"], dbg["pnp_best"]
    print("pnp_iterations:", it.tolist())
    print("pnp_best:", best.tolist())
    assert r[0]["frame_id"] == 0 and dbg[0]["frame_id"] == 0 and it[0] == 0
    assert (it > 8).any(), it
    early = (it >= 1) & (it <= 8)
    assert len(set(best[early].tolist())) >= 3, best[early]


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", CHUNKS)
def test_fused_handover_equals_the_two_launch_chain(handover_runs, chunk):
    """records byte for byte; winner, samples visited, consensus, outcome and the PnP pose of every frame"""
    rf, df = handover_runs[(chunk, 1)]
    r0, d0 = handover_runs[(chunk, 0)]
    assert rf == r0
    assert rf == handover_runs[(64, 0)][0]
    for k in DBG_FIELDS:
        assert df[k].tobytes() == d0[k].tobytes(), k
    assert np.array_equal(df["frame_id"], np.arange(N_FRAMES))


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", CHUNKS)
def test_handover_stamp_is_sane(handover_runs, chunk):
    """rt[5] (10 ns ticks): latest announcement of an awaited sample -> the LM's first build.  Positive and below 20 us on every
    frame the awaited samples decided, 0 elsewhere (frame 0: no RANSAC); the frame part ends after it starts."""
    _, d = handover_runs[(chunk, 1)]
    rt, it = d["rt"].astype(np.int64), d["pnp_iterations"]
    early = (it >= 1) & (it <= 8)
    print("rt[5] of the frames decided early:", rt[early, 5].tolist())
    assert early.sum() > N_FRAMES // 2
    assert ((rt[early, 5] > 0) & (rt[early, 5] < 2000)).all(), rt[early, 5]
    assert it[0] == 0 and rt[0, 5] == 0
    assert (rt[~early, 5] == 0).all()
    assert (rt[:, 4] < rt[:, 3]).all()
