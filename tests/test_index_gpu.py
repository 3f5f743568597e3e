"""The tracker's matching passes on the device (k_ti_lists, k_ti_resolve / ti_resolve_pass of csrc/svo_track.hip) on the
hand-made descriptor frames of index_cases.py, through svo_track_tail_dev: map-point identities per keypoint, counters, pool
rows and active-row counts must equal the C oracle's tail and the plain restatement (index_ref.py) exactly, and the records
must be byte-identical between one call of all frames, one frame per call, and every track_lcap x track_nblk setting.
Every number is an integer compared for equality.  `rounds` is evidence of reach, not a contract: >= 1 where a pass had rows."""
import numpy as np
import pytest

import index_cases
import index_ref

pytestmark = pytest.mark.gpu

COUNTERS = ("n_kp", "n_stereo", "n_match_pass1", "n_match_pass2", "n_lm_edges", "n_new_mappoints", "n_local_map",
            "n_pnp_inliers", "lm_iterations")
MODES = [(lcap, nblk) for lcap in (8, 2, 1) for nblk in (3, 1, 0)]
STRIDE = 500


@pytest.fixture(scope="module")
def ctx(pkg):
    s = pkg.Svo(index_cases.W, index_cases.H, max_batch=8)
    yield s
    s.close()


def _pack(pkg, frames, dev):
    import torch
    N = len(frames)
    kp = np.zeros((N, STRIDE), pkg.KP_DTYPE); desc = np.zeros((N, STRIDE, 32), np.uint8)
    n = np.zeros(N, np.int32); depth = np.zeros((N, STRIDE), np.float32)
    bx = np.zeros((N, 64, 4), np.int32); nb = np.zeros(N, np.int32)
    for k, (a, d, z, b) in enumerate(frames):
        n[k] = len(a); kp[k, :len(a)] = a; desc[k, :len(a)] = d; depth[k, :len(a)] = z
        nb[k] = len(b); bx[k, :len(b)] = b
    t = dict(kp=torch.from_numpy(kp.view(np.uint8).reshape(N, STRIDE, -1)).to(dev), desc=torch.from_numpy(desc).to(dev),
             n=torch.from_numpy(n).to(dev), depth=torch.from_numpy(depth).to(dev), bx=torch.from_numpy(bx).to(dev),
             nb=torch.from_numpy(nb).to(dev))
    torch.cuda.synchronize()
    return t


def _tail(pkg, s, t, first, count, res):
    rec = pkg.TRACK_DTYPE.itemsize
    bx = pkg.boxes_dev(t["bx"][first:].data_ptr(), t["nb"][first:].data_ptr(), 64)
    s.track_tail_dev(t["kp"][first:].data_ptr(), t["desc"][first:].data_ptr(), t["n"][first:].data_ptr(),
                     t["depth"][first:].data_ptr(), STRIDE, count, res.data_ptr() + first * rec, boxes=bx)
    s.sync()


def _check_frame(name, f, n, dbg, rows, r, ora):
    """One frame's device outputs against the restatement `r` and the oracle's `ora`."""
    res, cur, mg, ng, F, nv = ora
    want_m, want_n = index_ref.as_reported(r, f)
    assert np.array_equal(dbg["match_gid"][:n], want_m) and np.array_equal(dbg["match_gid"], mg), (name, f)
    assert np.array_equal(dbg["new_gid"][:n], want_n) and np.array_equal(dbg["new_gid"], ng), (name, f)
    assert dbg["frame_id"] == f
    assert list(dbg["active_rows"]) == r["active"], (name, f, list(dbg["active_rows"]), r["active"])
    for p in (0, 1):
        assert (dbg["rounds"][p] >= 1) == (r["active"][p] > 0), (name, f, p, list(dbg["rounds"]))
    if rows is not None:
        assert np.array_equal(rows[:n], r["rows"]) and np.array_equal(rows[:n], cur[:n]) and (rows[n:] == -1).all(), (name, f)


@pytest.mark.parametrize("name", index_cases.SMALL_FIRST)
def test_matching_passes_on_hand_made_frames(orc, pkg, ctx, name):
    import torch
    cam_d = dict(pkg.KITTI_00_02)
    case = index_cases.build(name, cam_d)
    frames, ref = case["frames"], case["ref"]
    ora = index_cases.oracle_tail(orc, cam_d, name)
    dev = torch.device("cuda", 0)
    cam = pkg.Camera(**pkg.KITTI_00_02)
    N = len(frames)
    rec = pkg.TRACK_DTYPE.itemsize
    t = _pack(pkg, frames, dev)
    s = ctx
    try:
        single = None
        for lcap, nblk in (MODES[0], MODES[-1]):               # one frame per call, at the defaults and with both turned down
            s.set_option("track_lcap", lcap); s.set_option("track_nblk", nblk)
            s.track_reset(cam)
            res = torch.zeros((N, rec), dtype=torch.uint8, device=dev)
            for f in range(N):
                _tail(pkg, s, t, f, 1, res)
                got = res[f].cpu().numpy().view(pkg.TRACK_DTYPE)[0]
                for c in COUNTERS:
                    assert got[c] == ora[f][0][c], (name, f, c, got[c], ora[f][0][c])
                for c in ("n_match_pass1", "n_match_pass2", "n_new_mappoints", "n_local_map"):
                    assert got[c] == ref[f][c], (name, f, c)
                dbg = s.debug_track_frames(0, 1)[0]
                _check_frame(name, f, len(frames[f][0]), dbg, s.debug_track_matches(), ref[f], ora[f])
                if len(frames[f][3]) and f > 0:
                    assert s.debug_track_gate()[1] == ora[f][5] == len(ref[f]["vetoed"]), (name, f)
                if single is None:
                    print("REACH", name, "frame", f, "active", list(dbg["active_rows"]), "rounds", list(dbg["rounds"]))
            assert s.track_overflowed() == 0
            if single is None:
                single = res.cpu().numpy().tobytes()
            else:
                assert res.cpu().numpy().tobytes() == single, (name, lcap, nblk)
        for lcap, nblk in MODES:                               # one call of all frames, every list capacity x blocker count
            s.set_option("track_lcap", lcap); s.set_option("track_nblk", nblk)
            s.track_reset(cam)
            out = torch.zeros((N, rec), dtype=torch.uint8, device=dev)
            _tail(pkg, s, t, 0, N, out)
            assert out.cpu().numpy().tobytes() == single, (name, lcap, nblk)
            dbg = s.debug_track_frames(0, N)
            rows = s.debug_track_matches()
            for f in range(N):
                _check_frame(name, f, len(frames[f][0]), dbg[f], rows if f == N - 1 else None, ref[f], ora[f])
            print("ROUNDS", name, "lcap", lcap, "nblk", nblk, [list(d["rounds"]) for d in dbg])
            assert s.track_overflowed() == 0
    finally:
        s.set_option("track_lcap", 8); s.set_option("track_nblk", 3)
