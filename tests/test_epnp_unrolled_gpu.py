"""The unrolled 12 x 12 step loop (csrc/svo_epnp_ord_asm.h, tools/gen_jacobi_asm.py) on the device: five-point samples chosen on the
CPU so that the loop is left after every sweep count the search met, through the entry tests/test_epnp_ord.py uses, bit for bit
against the CPU restatement's recorded results; and a short tracked sequence with the pose chain as one launch and as two."""
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = np.array([718.856, 718.856, 607.1928, 185.2157])


@pytest.fixture(scope="module")
def cases():
    return np.load(os.path.join(ROOT, "tests", "golden", "epnp5_unrolled_cases.npy"))


def test_fixture_covers_the_exits_of_the_unrolled_loop(cases):
    """(Needs no GPU work, kept beside the test it qualifies.)  tools/make_epnp_unrolled_cases.py drew 100,000 seeded samples -
    ordinary point sets, three kilometres from the origin, duplicated correspondences - and met 5 to 10 sweeps; NONE of them left
    the range of the loop's unscaled divisions (a singular value outside [2^-100, 2^100], or 25 sweeps): that branch stays with the
    `epnp_force_seq` switch of tests/test_epnp_ord.py and its degenerate samples.  The unrolled program has ONE closing copy, the
    period's last: a solve of s sweeps leaves it there after PRO + s PER steps, so every sweep count is the same exit, reached after
    another number of turns."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_jacobi_asm
    u = gen_jacobi_asm.Unrolled()
    closing = [t for t in u.copies() if u.closes(t) is not None]
    assert closing == [u.pro + u.per - 1]
    ordinary = cases[cases["kind"] == 0]
    assert len(set(ordinary["sweeps"].tolist())) >= 3 and ordinary["sweeps"].min() >= 2 and ordinary["sweeps"].max() < 25
    assert (cases["kind"] == 1).sum() >= 1                       # exactly coplanar: the degenerate path, no assembly loop
    assert 200 <= len(cases) <= 400


def test_fixture_samples_are_bit_identical_to_the_recorded_oracle_results(pkg, cases):
    svo = pkg.Svo(640, 240, max_batch=1)
    svo.set_option("epnp_exact", 2)
    for i, c in enumerate(cases):
        Rg, tg, rg = svo.debug_epnp5(c["X"], c["u"], K)
        R, t, ro = c["R"], c["t"], c["rep"]
        key = (i, int(c["kind"]), int(c["sweeps"]))
        if np.isfinite(R).all() and np.isfinite(t).all():
            assert np.array_equal(R.view(np.uint64), Rg.view(np.uint64)), key
            assert np.array_equal(t.view(np.uint64), tg.view(np.uint64)), key
        else:
            assert c["kind"] != 0, key
        both_nan = np.isnan(ro) & np.isnan(rg)
        assert np.array_equal(ro.view(np.uint64)[~both_nan], rg.view(np.uint64)[~both_nan]), key
    svo.close()


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
