"""The three-row Jacobi block with the rows in registers (EO_JACOBI_ASM_3R of csrc/svo_epnp_ord_asm.h, tools/gen_jacobi_asm.py) on the
device: five-point samples chosen on the CPU (tools/make_epnp_small_cases.py) so that each of a solve's five 3 x 3 decompositions is
left after several sweep counts and the three side-by-side ABt problems stop in different sweeps, through the entry
tests/test_epnp_ord.py uses, bit for bit against the CPU restatement's recorded results; and a short tracked sequence with the pose
chain as one launch and as two."""
import importlib
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = np.array([718.856, 718.856, 607.1928, 185.2157])


@pytest.fixture(scope="module")
def cases():
    return np.load(os.path.join(ROOT, "tests", "golden", "epnp5_small_cases.npy"))


def test_fixture_covers_the_exits_of_the_three_row_loop(cases):
    """(Needs no GPU.)  tools/make_epnp_small_cases.py drew 200,000 seeded samples - ordinary point sets, three kilometres from the origin,
    duplicated correspondences.  Per problem (control points, cvInvert(CC), ABt of candidates 1 to 3) the fixture holds at least three
    different sweep counts; in at least 20 cases the three ABt problems, which share the loop, do not stop in the same sweep (in the
    200,000 tries three pairwise different counts came up four times: those four are in); one sample is exactly coplanar (a zero
    singular value) and one has two equal singular values of PW0^T PW0 - both take the sequential finish, not the block's result."""
    assert len(cases) <= 400
    ordinary = cases[cases["kind"] == 0]
    for p in range(5):
        counts = set(ordinary["sweeps"][:, p].tolist())
        assert len(counts) >= 3 and min(counts) >= 1 and max(counts) < 25, (p, counts)
    abt = ordinary["sweeps"][:, 2:]
    assert int((abt.min(axis=1) != abt.max(axis=1)).sum()) >= 20
    assert sum(1 for r in abt if len(set(r.tolist())) == 3) >= 1
    assert (cases["kind"] == 1).sum() == 1 and (cases["kind"] == 2).sum() == 1
    sym = cases[cases["kind"] == 2][0]["X"]
    d = sym - sym.mean(axis=0)
    ptp = d.T @ d                                  # exact: small integers
    assert np.array_equal(ptp, np.diag([8.0, 8.0, 20.0]))
    flat = cases[cases["kind"] == 1][0]["X"]
    assert np.ptp(flat[:, 2]) == 0.0


@pytest.mark.gpu
def test_fixture_samples_are_bit_identical_to_the_recorded_oracle_results(pkg, cases):
    svo = pkg.Svo(640, 240, max_batch=1)
    svo.set_option("epnp_exact", 2)
    for i, c in enumerate(cases):
        Rg, tg, rg = svo.debug_epnp5(c["X"], c["u"], K)
        R, t, ro = c["R"], c["t"], c["rep"]
        key = (i, int(c["kind"]), c["sweeps"].tolist())
        if np.isfinite(R).all() and np.isfinite(t).all():
            assert np.array_equal(R.view(np.uint64), Rg.view(np.uint64)), key
            assert np.array_equal(t.view(np.uint64), tg.view(np.uint64)), key
        else:
            assert c["kind"] != 0, key
        both_nan = np.isnan(ro) & np.isnan(rg)
        assert np.array_equal(ro.view(np.uint64)[~both_nan], rg.view(np.uint64)[~both_nan]), key
    svo.close()


@pytest.mark.gpu
def test_eight_tracked_frames_fused_and_split_equal_the_oracle_tracker(pkg, orc):
    """8 frames of 1241 x 376: the records of the pose chain as ONE launch per frame ("tail_fused" 1, k_tp_tail_ord) and as two
    (k_tp_hyp_ord, then the frame part) are byte-identical to each other, and their counters, RANSAC consensus, LM iterations and
    pose are the free-running oracle tracker's."""
    import torch
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    N = 8
    dev = torch.device("cuda", 0)
    L, R, _ = synth.render_sequence(N, device=dev)
    H, W = int(L.shape[1]), int(L.shape[2])
    assert (W, H) == (1241, 376)
    pitch = 1280
    dL = torch.zeros((N, H, pitch), dtype=torch.uint8, device=dev); dR = torch.zeros_like(dL)
    dL[:, :, :W] = L.to(dev); dR[:, :, :W] = R.to(dev)
    cam = pkg.Camera(**pkg.KITTI_00_02)
    res = torch.zeros((N, pkg.TRACK_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    outs = {}
    for fused in (1, 0):
        s = pkg.Svo(W, H, max_batch=N)
        s.set_option("tail_fused", fused)
        s.track_reset(cam)
        s.track_batch_dev(dL.data_ptr(), dR.data_ptr(), pitch, N, res.data_ptr())
        s.sync()
        assert s.track_overflowed() == 0
        outs[fused] = res.cpu().numpy().view(pkg.TRACK_DTYPE).reshape(-1).copy()
        s.close()
    assert outs[1].tobytes() == outs[0].tobytes()
    Lh, Rh = L.cpu().numpy(), R.cpu().numpy()
    trk = orc.Tracker(W, H, pkg.KITTI_00_02)
    for k in range(N):
        ref, _ = trk.track(Lh[k], Rh[k])
        got = outs[1][k]
        for f in ("frame_id", "n_kp", "n_stereo", "n_match_pass1", "n_match_pass2", "n_lm_edges", "n_new_mappoints", "n_local_map",
                  "n_pnp_inliers", "lm_iterations"):
            assert got[f] == ref[f], (k, f, got[f], ref[f])
        assert got["Tcw"].tobytes() == ref["Tcw"].tobytes(), k
    trk.close()
