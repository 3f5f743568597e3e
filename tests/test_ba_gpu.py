"""GPU suite of the windowed bundle adjustment (svo_ba_*; csrc/svo_ba.hip) against the numpy twin (tests/ba_ref.py) on the hand-made
windows of tests/ba_cases.py.

Per case: the discrete results equal the twin's (status, counts, the point list's gids and n_obs, iterations, trials); poses,
points and the two chi2 stay within 10 x the case's recorded scatter between the twin's summation orders
(tests/golden/ba_restatement_pins.json), with a floor of 1e-12 relative - the margin this project gives a float64 path whose
summation order it does not pin; chi2_final <= chi2_initial; the same call twice gives the same bytes."""
import importlib
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import ba_cases  # noqa: E402
import ba_ref  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 0xA5
PINS = json.load(open(os.path.join(ba_ref.GOLDEN, "ba_restatement_pins.json")))
_twin = {}


def twin(name):
    if name not in _twin:
        c = ba_cases.case(name)
        _twin[name] = (c, ba_ref.run(c["obs"], c["counts"], c["Tcw"], c["cam"], c["params"]))
    return _twin[name]


def margin(scatter):
    return max(10 * scatter, 1e-12)


def compare(T, pts, st, ref, scatter, what):
    """device outputs of one window against a twin result under the scatter dict(pose, points, chi2)"""
    d = ba_ref.discrete(ref)
    got = dict(status=int(st["status"]), n_points=int(st["n_points"]), n_edges=int(st["n_edges"]),
               n_edges_stereo=int(st["n_edges_stereo"]), iterations=int(st["iterations"]))
    assert got == {k: d[k] for k in got}, what
    assert int(st["trials_total"]) == sum(d["trials"]), what
    assert np.array_equal(pts["gid"], ref["gid"]) and np.array_equal(pts["n_obs"], ref["n_obs"]), what
    X = np.stack([pts["X"], pts["Y"], pts["Z"]], 1).reshape(-1, 3)
    dT, dX = ba_cases._rel(ref["Tcw"].reshape(-1), np.asarray(T).reshape(-1)), ba_cases._rel(ref["X"], X)
    s = ref["stats"]
    dchi = max(abs(float(st[k]) - s[k]) / max(abs(s[k]), 1e-300) if float(st[k]) != s[k] else 0.0 for k in ("chi2_initial", "chi2_final"))
    print("%s: pose %.2e (margin %.2e)  points %.2e (%.2e)  chi2 %.2e (%.2e)" %
          (what, dT, margin(scatter["pose"]), dX, margin(scatter["points"]), dchi, margin(scatter["chi2"])))
    assert dT <= margin(scatter["pose"]), what
    assert dX <= margin(scatter["points"]), what
    assert dchi <= margin(scatter["chi2"]), what
    assert float(st["chi2_final"]) <= float(st["chi2_initial"]), what


@pytest.mark.parametrize("name", list(ba_cases.CASES))
def test_case_against_the_twin(pkg, name):
    c, ref = twin(name)
    ba = pkg.BundleAdjuster(c["max_kp"], 1)
    cam = pkg.Camera(*c["cam"])
    par = pkg.BaParams.default(**c["params"])
    T, pts, st = ba.window(cam, par, c["obs"], c["counts"], c["Tcw"])
    T2, pts2, st2 = ba.window(cam, par, c["obs"], c["counts"], c["Tcw"])
    ba.close()
    assert PINS[name]["discrete"] == ba_ref.discrete(ref)
    compare(T, pts, st, ref, PINS[name]["scatter"], name)
    assert T.tobytes() == T2.tobytes() and pts.tobytes() == pts2.tobytes() and st.tobytes() == st2.tobytes(), "not deterministic"
    if name == "empty":
        assert int(st["status"]) == pkg.BA_EMPTY and np.array_equal(T, c["Tcw"].astype(np.float64))
    for f in range(c["params"]["n_fixed"]):
        assert np.array_equal(T[f], c["Tcw"][f].astype(np.float64)), "a fixed frame moved"


class Dev:
    """Device copies of a frame sequence and guarded outputs for n_windows windows."""

    def __init__(self, pkg, obs, counts, Tcw, max_kp, window, n_windows, pose_stride=64, points=True):
        import torch
        self.torch = torch
        F, stride = obs.shape
        self.obs = torch.from_numpy(np.ascontiguousarray(obs).view(np.uint8).reshape(-1)).cuda()
        self.counts = torch.from_numpy(np.ascontiguousarray(counts, np.int32)).cuda()
        poses = np.full((F, pose_stride), GUARD, np.uint8)
        poses[:, :64] = np.ascontiguousarray(Tcw, np.float32).reshape(F, 16).view(np.uint8)
        self.Tcw = torch.from_numpy(poses.reshape(-1)).cuda()
        self.pad = 256
        self.nT = n_windows * window * 16 * 8
        self.pstride = window * max_kp // 2
        self.nP = n_windows * self.pstride * 32
        self.nS = n_windows * 48
        self.window, self.n_windows, self.stride, self.pose_stride = window, n_windows, stride, pose_stride
        self.oT = torch.full((self.nT + 2 * self.pad,), GUARD, dtype=torch.uint8, device="cuda")
        self.oP = torch.full((self.nP + 2 * self.pad,), GUARD, dtype=torch.uint8, device="cuda") if points else None
        self.oS = torch.full((self.nS + 2 * self.pad,), GUARD, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def run(self, ba, cam, par, first, step, producer=None):
        ba.windows_dev(cam, par, self.obs.data_ptr(), self.counts.data_ptr(), self.stride, self.Tcw.data_ptr(), self.pose_stride,
                       first, self.n_windows, step, self.oT.data_ptr() + self.pad,
                       None if self.oP is None else self.oP.data_ptr() + self.pad, self.oS.data_ptr() + self.pad, producer=producer)

    def fetch(self, pkg):
        """-> per window (T bytes, points bytes (the n_points written), stats bytes); checks the guards"""
        out = []
        oT, oS = self.oT.cpu().numpy(), self.oS.cpu().numpy()
        oP = None if self.oP is None else self.oP.cpu().numpy()
        for a, n in ((oT, self.nT), (oS, self.nS)) + (() if oP is None else ((oP, self.nP),)):
            assert (a[:self.pad] == GUARD).all() and (a[self.pad + n:] == GUARD).all(), "guard bytes written"
        for w in range(self.n_windows):
            st = oS[self.pad + 48 * w:self.pad + 48 * (w + 1)].copy().view(pkg.BA_STATS_DTYPE)[0]
            T = oT[self.pad + w * self.window * 128:self.pad + (w + 1) * self.window * 128].copy()
            P = b""
            if oP is not None:
                slot = oP[self.pad + w * self.pstride * 32:self.pad + (w + 1) * self.pstride * 32]
                n = int(st["n_points"])
                assert (slot[32 * n:] == GUARD).all(), "points beyond n_points written"
                P = slot[:32 * n].copy()
            out.append((T, P, st))
        return out


@pytest.fixture(scope="module")
def long_case():
    # 16 frames of one scene, windows of 4
    c = ba_cases.make(seed=71, window=16, n_fixed=1, n_points=260, max_kp=256)
    c["params"].update(window=4, n_fixed=1)
    return c


def test_windows_are_independent(pkg, long_case):
    """A window solved alone == the same window as number 0, 2 and 4 of a five-window call, at step 1 and 3, byte for byte; guard
    bytes around the three outputs (and the point slots beyond n_points) untouched; d_points may be NULL."""
    c = long_case
    cam = pkg.Camera(*c["cam"])
    par = pkg.BaParams.default(**c["params"])
    ba = pkg.BundleAdjuster(c["max_kp"], 5)
    for step in (1, 3):
        first = 1 if step == 1 else 0
        five = Dev(pkg, c["obs"], c["counts"], c["Tcw"], c["max_kp"], 4, 5)
        five.run(ba, cam, par, first, step)
        ba.sync()
        got = five.fetch(pkg)
        nop = Dev(pkg, c["obs"], c["counts"], c["Tcw"], c["max_kp"], 4, 5, points=False)
        nop.run(ba, cam, par, first, step)
        ba.sync()
        for (T, P, st), (T2, _, st2) in zip(got, nop.fetch(pkg)):
            assert T.tobytes() == T2.tobytes() and st.tobytes() == st2.tobytes()
        for w in (0, 2, 4):
            f0 = first + w * step
            one = Dev(pkg, c["obs"][f0:f0 + 4], c["counts"][f0:f0 + 4], c["Tcw"][f0:f0 + 4], c["max_kp"], 4, 1)
            one.run(ba, cam, par, 0, 1)
            ba.sync()
            T, P, st = one.fetch(pkg)[0]
            assert int(st["status"]) == 0 and int(st["n_points"]) > 20
            assert T.tobytes() == got[w][0].tobytes() and P.tobytes() == got[w][1].tobytes() and st.tobytes() == got[w][2].tobytes(), (step, w)
    ba.close()


def test_pose_strides_and_the_host_entry_agree(pkg):
    """pose_stride_bytes of a bare 64-byte pose and of svo_track_result, through svo_ba_windows_dev == svo_ba_window."""
    c, ref = twin("stride_small")
    cam = pkg.Camera(*c["cam"])
    par = pkg.BaParams.default(**c["params"])
    ba = pkg.BundleAdjuster(c["max_kp"], 1)
    T, pts, st = ba.window(cam, par, c["obs"], c["counts"], c["Tcw"])
    for ps in (64, pkg.TRACK_DTYPE.itemsize):
        d = Dev(pkg, c["obs"], c["counts"], c["Tcw"], c["max_kp"], c["params"]["window"], 1, pose_stride=ps)
        d.run(ba, cam, par, 0, 1)
        ba.sync()
        T2, P2, st2 = d.fetch(pkg)[0]
        assert T2.tobytes() == T.tobytes() and P2.tobytes() == pts.tobytes() and st2.tobytes() == st.tobytes(), ps
    ba.close()


N, W, H, K, PITCH = 12, 1241, 376, 500, 1280


def test_hand_over_from_the_tracker(pkg):
    """svo_track_batch_dev with svo_track_map_out, followed at once by svo_ba_windows_dev(producer = ctx) with no svo_sync in
    between == a second run that synchronises first and adjusts copies of the records; the tracker's result records of both ==
    those of a run without any adjustment; the windows agree with the twin on the same records."""
    import torch
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    L, R, _ = synth.render_sequence(N)
    dL = torch.zeros((N, H, PITCH), dtype=torch.uint8, device="cuda")
    dR = torch.zeros_like(dL)
    dL[:, :, :W] = L.cuda()
    dR[:, :, :W] = R.cuda()
    cam = pkg.Camera(**pkg.KITTI_00_02)
    par = pkg.BaParams.default()
    rec = pkg.TRACK_DTYPE.itemsize
    torch.cuda.synchronize()

    def track(adjust):
        """adjust: None, 'behind' (producer hand-over, no sync) or 'copies' (sync, then adjust copies)"""
        ctx = pkg.Svo(W, H, max_batch=N)
        ctx.track_reset(cam)
        res = torch.zeros((N, rec), dtype=torch.uint8, device="cuda")
        obs = torch.zeros((N * K * 32,), dtype=torch.uint8, device="cuda")
        counts = torch.zeros((N,), dtype=torch.int32, device="cuda")
        ba = pkg.BundleAdjuster(K, 2)
        ba.stream        # (the adjuster's device side exists before the tracker call: nothing but the two calls in between)
        oT = torch.zeros((2 * 8 * 16,), dtype=torch.float64, device="cuda")
        oP = torch.zeros((2 * 4 * K * 32,), dtype=torch.uint8, device="cuda")
        oS = torch.zeros((2 * 48,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        if adjust:
            ctx.track_map_out(obs.data_ptr(), counts.data_ptr())
        ctx.track_batch_dev(dL.data_ptr(), dR.data_ptr(), PITCH, N, res.data_ptr())
        if adjust == "behind":
            ba.windows_dev(cam, par, obs, counts, K, res, rec, 0, 2, 4, oT, oP, oS, producer=ctx)
        elif adjust == "copies":
            ctx.sync()
            obs2, counts2, res2 = obs.clone(), counts.clone(), res.clone()
            torch.cuda.synchronize()
            ba.windows_dev(cam, par, obs2, counts2, K, res2, rec, 0, 2, 4, oT, oP, oS)
        ba.sync()
        ctx.sync()
        out = (res.cpu().numpy().tobytes(), oT.cpu().numpy(), oP.cpu().numpy(), oS.cpu().numpy().view(pkg.BA_STATS_DTYPE),
               obs.cpu().numpy().view(pkg.MAP_OBS_DTYPE).reshape(N, K), counts.cpu().numpy())
        ba.close()
        ctx.close()
        return out

    plain = track(None)
    behind = track("behind")
    copies = track("copies")
    assert behind[0] == plain[0] == copies[0], "the tracker's records changed"
    assert behind[1].tobytes() == copies[1].tobytes() and behind[3].tobytes() == copies[3].tobytes()
    res = np.frombuffer(behind[0], pkg.TRACK_DTYPE)
    for w in range(2):
        st = behind[3][w]
        n = int(st["n_points"])
        assert int(st["status"]) == 0 and n > 50
        sl = slice(w * 4 * K * 32, w * 4 * K * 32 + 32 * n)
        assert behind[2][sl].tobytes() == copies[2][sl].tobytes()
        f0 = 4 * w
        p = ba_ref.default_params()
        args = (behind[4][f0:f0 + 8], behind[5][f0:f0 + 8], res["Tcw"][f0:f0 + 8].reshape(8, 4, 4), ba_cases.KITTI, p)
        rs = [ba_ref.run(*args, order=o) for o in ba_ref.ORDERS]
        d = [ba_ref.discrete(r) for r in rs]
        assert d[0] == d[1] == d[2], "the twin's own orders disagree on these records: no margin to hold the device to"
        pts = behind[2][sl].copy().view(pkg.BA_POINT_DTYPE)
        compare(behind[1][w * 128:(w + 1) * 128].reshape(8, 4, 4), pts, st, rs[0], ba_cases.scatter(rs), "tracked window %d" % w)
