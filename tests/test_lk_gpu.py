"""GPU suite of the pyramidal Lucas-Kanade tracker (svo_lk_*): the device against the numpy restatement tests/lk_ref.py, bit for
bit - every pyramid and derivative level through svo_lk_debug_level, then next points, status and err; the batch entry and
the chain entry against single calls; the argument checks; independence from the tracker; the host class seams
frame::LKTrack (host/lk_check) and Tracking::dynamic_lk (host/stereo_kitti --dynamic-lk)."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import lk_cases
import lk_ref
import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stage_case(name):
    kind, size = name.split("_")
    W, H = (int(v) for v in size.split("x"))
    if kind == "noise":
        return lk_cases.noise(W + H, W, H), lk_cases.noise(W + H + 1, W, H)
    return util.urban_pair(W, H, 30, 60)


STAGE_CASES = ("noise_185x177", "noise_120x50", "noise_1241x48", "noise_83x37",
               "urban_185x177", "urban_120x50", "urban_1241x48", "urban_83x37")
STAGE_TOP = {"185x177": 3, "120x50": 1, "1241x48": 1, "83x37": 0}


def _result_case(name):
    """(prev, next, points)"""
    if name == "exits185x177":        # the planted-shift pair with every exit, integer and tie coordinates: 300 points
        return lk_cases.exits_pair() + (lk_cases.exits_points(300),)
    if name == "planted120x50":       # top level 1
        return lk_cases.planted_pair(13, 120, 50, (-3.2, 1.7)) + (lk_cases.edge_points(120, 50),)
    if name == "rows1241x48":         # full-width rows, points in the first and last 21 columns
        return lk_cases.planted_pair(12, 1241, 48, (1.5, 0.5)) + (lk_cases.edge_points(1241, 48),)
    if name == "lowcontrast120x100":  # the oscillation rule at level 0
        pts = np.concatenate([[lk_cases.OSCILLATION_POINT], lk_cases.inner_grid(120, 100, 25, 9)]).astype(np.float32)
        return lk_cases.low_contrast_pair() + (pts,)
    if name == "wander40x40":         # one level, all 30 iterations
        pts = np.concatenate([[lk_cases.MAX_COUNT_POINT], lk_cases.inner_grid(40, 40, 8, 5)]).astype(np.float32)
        return lk_cases.wander_pair() + (pts,)
    raise KeyError(name)


RESULT_CASES = ("exits185x177", "planted120x50", "rows1241x48", "lowcontrast120x100", "wander40x40")
_refs = {}


def _ref(name):
    """The restatement of a result case, computed once per session and never modified."""
    if name not in _refs:
        prev, nxt, pts = _result_case(name)
        _refs[name] = (prev, nxt, pts, lk_ref.track(prev, nxt, pts))
    return _refs[name]


@pytest.fixture(scope="module")
def svo(pkg):
    s = pkg.Svo(640, 240, max_batch=1)     # (LK takes any pair size: its arena is its own)
    yield s
    s.close()


def _same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", STAGE_CASES)
def test_every_level_equals_the_restatement(svo, name):
    prev, nxt = _stage_case(name)
    H, W = prev.shape
    levels_p, derivs_p = lk_ref.build_pyramid(prev)
    levels_n, derivs_n = lk_ref.build_pyramid(nxt)
    top = len(levels_p) - 1
    assert top == STAGE_TOP[name.split("_")[1]]
    svo.lk_track(prev, nxt, np.float32([[W / 2, H / 2]]))
    for frame, (levels, derivs) in enumerate(((levels_p, derivs_p), (levels_n, derivs_n))):
        for level in range(top + 1):
            img, t = svo.lk_debug_level(0, frame, level)
            assert t == top
            bad = np.argwhere(img != levels[level])
            assert img.shape == levels[level].shape and len(bad) == 0, (name, frame, level, len(bad), bad[:4].tolist())
            der, _ = svo.lk_debug_level(1, frame, level)
            bad = np.argwhere(der != derivs[level])
            assert der.shape == derivs[level].shape and len(bad) == 0, (name, frame, level, len(bad), bad[:4].tolist())
    with pytest.raises(Exception, match="level above"):
        svo.lk_debug_level(0, 0, top + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", RESULT_CASES)
def test_points_status_and_err_equal_the_restatement(svo, name):
    prev, nxt, pts, ref = _ref(name)
    ex = ref["exits"]
    if name == "exits185x177":
        assert len(pts) == 300
        assert ex[0, 0] == lk_ref.EXIT_RANGE_PREV and ex[1, 0] == lk_ref.EXIT_MIN_EIG and ex[2, 0] == lk_ref.EXIT_RANGE_NEXT
        assert ref["iterations"][2, 0] > 0 and not ref["status"][:3].any()
        for code in (lk_ref.EXIT_EPSILON, lk_ref.EXIT_OSCILLATION, lk_ref.EXIT_MAX_COUNT):
            assert (ex == code).any(), code
        assert (pts == np.floor(pts)).all(axis=1).sum() >= 40 and ((pts % 1) == 0.5).any(axis=1).sum() >= 40
    if name == "lowcontrast120x100":
        assert ex[0, 0] == lk_ref.EXIT_OSCILLATION
    if name == "wander40x40":
        assert ex[0, 0] == lk_ref.EXIT_MAX_COUNT and ref["iterations"][0, 0] == 30 and ref["top"] == 0
    if name == "rows1241x48":
        assert (pts[:, 0] < 21).sum() >= 12 and (pts[:, 0] >= 1241 - 21).sum() >= 12
    nxt_pts, st, err = svo.lk_track(prev, nxt, pts)
    assert np.array_equal(st, ref["status"]), np.flatnonzero(st != ref["status"])[:8]
    bad = np.flatnonzero((nxt_pts.view(np.uint32) != ref["next_pts"].view(np.uint32)).any(axis=1))
    assert len(bad) == 0, (len(bad), bad[:8].tolist(), nxt_pts[bad[:3]].tolist(), ref["next_pts"][bad[:3]].tolist())
    assert _same_bits(err, ref["err"]), np.flatnonzero(err != ref["err"])[:8]
    assert 0 < st.sum() and np.all(err[st == 0] == 0)


@pytest.mark.gpu
def test_max_level_is_honoured(pkg, svo):
    prev, nxt, pts, _ = _ref("planted120x50")
    p = pkg.lk_default_params()
    p.maxLevel = 0
    ref = lk_ref.track(prev, nxt, pts[:16], max_level=0)
    got, st, err = svo.lk_track(prev, nxt, pts[:16], p)
    assert svo.lk_debug_level(0, 0, 0)[1] == 0
    assert _same_bits(got, ref["next_pts"]) and np.array_equal(st, ref["status"]) and _same_bits(err, ref["err"])


# ---- svo_lk_batch_dev -----------------------------------------------------------------------------------------------------------
def _frames(B, W=200, H=180, seed=40):
    """B frames of one texture moving by (1.5 b, -0.75 b)."""
    c = lk_cases.smooth_canvas(seed, W, H)
    return [lk_cases.resample(c, W, H, 1.5 * b, -0.75 * b) for b in range(B)]


def _to_dev(frames, pitch):
    import torch
    dev = torch.device("cuda", 0)
    B, (H, W) = len(frames), frames[0].shape
    d = torch.zeros((B, H, pitch), dtype=torch.uint8, device=dev)
    d[:, :, :W] = torch.from_numpy(np.stack(frames)).to(dev)
    return d


@pytest.mark.gpu
def test_batch_equals_single_calls(pkg, svo):
    """Five frames (rows 256 bytes apart, not W), four pairs with 0 / 1 / 64 / 65 points ... and max_pts in a second call's
    last pair; frame 1, 2, 3 each serve two pairs."""
    import torch
    W, H, B, pitch, max_pts = 200, 180, 5, 256, 130
    frames = _frames(B)
    rng = np.random.default_rng(8)
    for counts in ((0, 1, 64, 65), (65, 0, 1, max_pts)):
        pts = rng.uniform((-5, -5), (W + 5, H + 5), (B - 1, max_pts, 2)).astype(np.float32)
        dev = torch.device("cuda", 0)
        d_f = _to_dev(frames, pitch)
        d_pts = torch.from_numpy(pts).to(dev); d_cnt = torch.tensor(counts, dtype=torch.int32, device=dev)
        d_next = torch.full((B - 1, max_pts, 2), -7.0, dtype=torch.float32, device=dev)
        d_st = torch.full((B - 1, max_pts), 9, dtype=torch.uint8, device=dev)
        d_err = torch.full((B - 1, max_pts), -7.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        svo.lk_batch_dev(d_f.data_ptr(), pitch, W, H, B, d_pts.data_ptr(), d_cnt.data_ptr(), max_pts, d_next.data_ptr(),
                         d_st.data_ptr(), d_err.data_ptr())
        g_next, g_st, g_err = d_next.cpu().numpy(), d_st.cpu().numpy(), d_err.cpu().numpy()
        for b, n in enumerate(counts):
            nx, st, err = svo.lk_track(frames[b], frames[b + 1], pts[b, :n])
            assert g_next[b, :n].tobytes() == nx.tobytes() and g_st[b, :n].tobytes() == st.tobytes(), b
            assert g_err[b, :n].tobytes() == err.tobytes(), b
            assert np.all(g_st[b, n:] == 9) and np.all(g_next[b, n:] == -7.0), "entries past a list's count are not written"
            if n:
                assert st.sum() > 0
    # a NULL err array is allowed
    svo.lk_batch_dev(d_f.data_ptr(), pitch, W, H, B, d_pts.data_ptr(), d_cnt.data_ptr(), max_pts, d_next.data_ptr(),
                     d_st.data_ptr(), None)


# ---- svo_lk_chain_dev -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_chain_equals_a_host_loop_of_single_calls(pkg, svo):
    """Six frames, seeds at frames 0, 1 and 3.  Frame 1's seeds overflow max_pts.  Frame 2 is constant below row 60: the points
    that sit there have a zero normal matrix when frame 2 is the previous image, so more than half of the list dies on the way
    to frame 3."""
    import torch
    W, H, B, pitch, max_seeds, max_pts = 200, 180, 6, 208, 80, 100
    frames = _frames(B, seed=41)
    frames[2] = frames[2].copy()
    frames[2][60:, :] = 128
    rng = np.random.default_rng(9)
    seeds = np.zeros((B, max_seeds, 2), np.float32)
    seed_counts = np.array([60, 50, 0, 80, 0, 0], np.int32)
    for f in range(B):
        seeds[f, :seed_counts[f]] = rng.uniform((5, 5), (W - 5, H - 5), (seed_counts[f], 2))
    # the host loop
    lists, counts, dropped, survivors = [], [], [], []
    cur = np.zeros((0, 2), np.float32)
    for f in range(B):
        if f:
            nx, st, _ = svo.lk_track(frames[f - 1], frames[f], cur)
            cur = nx[st != 0]
        survivors.append(len(cur))
        take = min(int(seed_counts[f]), max_pts - len(cur))
        dropped.append(int(seed_counts[f]) - take)
        cur = np.concatenate([cur, seeds[f, :take]]).astype(np.float32)
        lists.append(cur); counts.append(len(cur))
    assert dropped[1] > 0 and counts[1] == max_pts, "frame 1's seeds overflow the list"
    assert 0 < survivors[3] < 0.5 * counts[2], "more than half of frame 2's list dies on the way to frame 3"
    assert counts[5] > 0
    dev = torch.device("cuda", 0)
    d_f = _to_dev(frames, pitch)
    d_seeds = torch.from_numpy(seeds).to(dev); d_sc = torch.from_numpy(seed_counts).to(dev)
    d_lists = torch.full((B, max_pts, 2), -7.0, dtype=torch.float32, device=dev)
    d_lc = torch.full((B,), -1, dtype=torch.int32, device=dev); d_dr = torch.full((B,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    svo.lk_chain_dev(d_f.data_ptr(), pitch, W, H, B, d_seeds.data_ptr(), d_sc.data_ptr(), max_seeds, max_pts, d_lists.data_ptr(),
                     d_lc.data_ptr(), d_dr.data_ptr())
    g_lists, g_lc, g_dr = d_lists.cpu().numpy(), d_lc.cpu().numpy(), d_dr.cpu().numpy()
    assert g_lc.tolist() == counts and g_dr.tolist() == dropped
    for f in range(B):
        assert g_lists[f, :counts[f]].tobytes() == lists[f].tobytes(), f


# ---- errors ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_checks(pkg, svo):
    prev, nxt, pts, _ = _ref("planted120x50")
    p = pkg.lk_default_params()
    p.winSize = 15
    with pytest.raises(pkg.SvoError, match="invalid"):
        svo.lk_track(prev, nxt, pts, p)
    for change in (dict(maxLevel=4), dict(maxCount=20), dict(epsilon=0.03), dict(minEigThreshold=1e-3)):
        p = pkg.lk_default_params()
        for k, v in change.items():
            setattr(p, k, v)
        with pytest.raises(pkg.SvoError, match="invalid"):
            svo.lk_track(prev, nxt, pts, p)
    lib = pkg.load_library()
    p = pkg.lk_default_params()
    # sizes and counts are answered on the host, before the context is looked at
    assert lib.svo_lk_track(None, None, None, 120, 120, 50, C.byref(p), None, 4097, None, None, None) == -5
    assert lib.svo_lk_track(None, None, None, 4097, 4097, 50, C.byref(p), None, 10, None, None, None) == -5
    assert lib.svo_lk_track(None, None, None, 21, 21, 50, C.byref(p), None, 10, None, None, None) == -1
    nx, st, err = svo.lk_track(prev, nxt, np.zeros((0, 2), np.float32))      # n = 0: SVO_OK, nothing happens
    assert nx.shape == (0, 2) and st.shape == (0,) and err.shape == (0,)
    with pytest.raises(pkg.SvoError, match="4096"):
        svo.lk_track(prev, nxt, np.zeros((4097, 2), np.float32))


# ---- independence ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lk_between_tracker_frames_changes_nothing(pkg):
    import torch
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    L, R, _ = synth.render_sequence(3, device=torch.device("cuda", 0))
    L, R = L.cpu().numpy(), R.cpu().numpy()
    H, W = L.shape[1], L.shape[2]
    cam = pkg.Camera(**pkg.KITTI_00_02)
    runs = []
    for with_lk in (False, True):
        ctx = pkg.Svo(W, H, max_batch=1)
        ctx.track_reset(cam)
        rec = []
        for k in range(3):
            rec.append(ctx.track_frame(L[k], R[k]).tobytes() + ctx.debug_track_matches().tobytes())
            if with_lk and k < 2:
                _, st, _ = ctx.lk_track(L[k], L[k + 1], lk_cases.inner_grid(W, H, 60, 90))
                assert st.sum() > 0
        ctx.close()
        runs.append(b"".join(rec))
    assert runs[0] == runs[1]


# ---- the host class seam --------------------------------------------------------------------------------------------------------
def _write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, np.uint8).tobytes())


@pytest.mark.gpu
def test_host_class_lktrack_prints_the_restatements_points(tmp_path):
    """frame::LKTrack (host/lk_check) on a written pair: every point's coordinates (as float bit patterns), status and err."""
    exe = os.path.join(ROOT, "stereo-semantic-vo_amd", "host", "lk_check")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    prev, nxt, pts, ref = _ref("planted120x50")
    _write_pgm(tmp_path / "p.pgm", prev); _write_pgm(tmp_path / "n.pgm", nxt)
    with open(tmp_path / "pts.txt", "w") as f:
        for x, y in pts:
            f.write("%r %r\n" % (float(x), float(y)))
    r = subprocess.run([exe, str(tmp_path / "p.pgm"), str(tmp_path / "n.pgm"), str(tmp_path / "pts.txt")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l.split() for l in r.stdout.splitlines() if l.startswith("lk ")]
    assert len(lines) == len(pts)
    for i, tok in enumerate(lines):
        want = ref["next_pts"][i].view(np.uint32)
        assert (int(tok[1]), int(tok[2], 16), int(tok[3], 16), int(tok[4]), int(tok[5], 16)) == \
            (i, int(want[0]), int(want[1]), int(ref["status"][i]), int(ref["err"][i:i + 1].view(np.uint32)[0])), i
    kept = [l.split() for l in r.stdout.splitlines() if l.startswith("kept ")]
    assert int(kept[0][1]) == int(ref["status"].sum())


# ---- Tracking::dynamic_lk through host/stereo_kitti ------------------------------------------------------------------------------
N_DYN = 4
DYN_BOX = (500, 760, 200, 330)           # left right top bottom, the offline format


@pytest.fixture(scope="module")
def dynamic_runs(pkg, tmp_path_factory):
    """A four-frame synthetic sequence with one box per frame through stereo_kitti, three times: plain, --dynamic-lk with
    --write-dynamic, and plain again from a second copy of the trajectory directory."""
    import torch
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    L, R, _ = synth.render_sequence(N_DYN, device=torch.device("cuda", 0))
    L, R = L.cpu().numpy(), R.cpu().numpy()
    root = tmp_path_factory.mktemp("dyn")
    seq = root / "seq"
    (seq / "image_0").mkdir(parents=True); (seq / "image_1").mkdir(); (seq / "boxes").mkdir()
    for k in range(N_DYN):
        _write_pgm(seq / "image_0" / ("%06d.pgm" % k), L[k]); _write_pgm(seq / "image_1" / ("%06d.pgm" % k), R[k])
        (seq / "boxes" / ("%d.txt" % (k + 1))).write_text("%d %d %d %d\n" % DYN_BOX)
    (seq / "times.txt").write_text("".join("%e\n" % (0.1 * k) for k in range(N_DYN)))
    y = root / "s.yaml"
    y.write_text("%YAML:1.0\nCamera.fx: 718.856\nCamera.fy: 718.856\nCamera.cx: 607.1928\nCamera.cy: 185.2157\n"
                 "Camera.width: 1241\nCamera.height: 376\nCamera.bf: 386.1448\n")
    exe = os.path.join(ROOT, "stereo-semantic-vo_amd", "host", "stereo_kitti")
    out = {}
    for name, extra in (("off", []), ("on", ["--dynamic-lk", "--write-dynamic", str(root / "on" / "dyn")])):
        (root / name / "dyn").mkdir(parents=True)
        p = subprocess.run([exe] + extra + ["voc", str(y), str(seq)], capture_output=True, text=True, cwd=str(root / name),
                           timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        out[name] = root / name
    return L, R, out


def _strictly_inside(x, y, box):
    return (x > box[0]) & (x < box[1]) & (y > box[2]) & (y < box[3])


@pytest.mark.gpu
def test_tracking_dynamic_lk_equals_the_restated_loop(pkg, dynamic_runs):
    """Per frame, the list stereo_kitti --write-dynamic wrote (lastframe.DY_keypoints after the frame) against the commented
    loop of src/Tracking.cc:189-223 restated here and driven by Svo.lk_track: the previous list tracked and erased by status in
    order, then the seeds - at frame 0 every keypoint strictly inside the box (init), and at frames 0 and 1 every keypoint
    strictly inside the box that has no map point after matching (createmappoint, id <= 1)."""
    L, R, runs = dynamic_runs
    H, W = L.shape[1], L.shape[2]
    cam = pkg.Camera(**pkg.KITTI_00_02)
    fe = pkg.Svo(W, H, max_batch=1)
    trk = pkg.Svo(W, H, max_batch=1)
    trk.track_reset(cam)
    box = np.array([DYN_BOX], np.int32)
    cur = np.zeros((0, 2), np.float32)
    seeded = 0
    for k in range(N_DYN):
        if len(cur):
            nx, st, _ = fe.lk_track(L[k - 1], L[k], cur)
            cur = nx[st != 0]
        kp = fe.stereo_frame(L[k], R[k], cam)["kpL"]
        xy = np.stack([kp["x"], kp["y"]], 1).astype(np.float32)
        res = trk.track_frame(L[k], R[k], boxes=box)
        has_mp = trk.debug_track_matches()[:len(xy)] >= 0
        assert res["n_kp"] == len(xy)
        inside = _strictly_inside(xy[:, 0], xy[:, 1], DYN_BOX)
        if k == 0:
            cur = np.concatenate([cur, xy[inside]])
        if k <= 1:
            cur = np.concatenate([cur, xy[inside & ~has_mp]])
            seeded += int((inside & ~has_mp).sum())
        got = np.loadtxt(str(runs["on"] / "dyn" / ("%06d.txt" % k)), dtype=np.float64, ndmin=2).astype(np.float32).reshape(-1, 2)
        assert got.shape == cur.shape, (k, got.shape, cur.shape)
        assert np.array_equal(got.view(np.uint32), cur.astype(np.float32).view(np.uint32)), k
    fe.close(); trk.close()
    assert seeded > 0 and len(cur) > 0, "the box must hold keypoints, and some must survive to the last frame"
    # a point on the box's edge is no seed: the test is strict
    assert not _strictly_inside(np.float32(DYN_BOX[0]), np.float32(250), DYN_BOX)


@pytest.mark.gpu
def test_dynamic_lk_leaves_the_trajectory_files_alone(dynamic_runs):
    """The LK loop feeds nothing back into tracking: with the flag on, both trajectory files are byte-identical to the run
    without it, which writes no point files."""
    _, _, runs = dynamic_runs
    for f in ("cameratrajectory_kitti.txt", "cameratrajectory_tum.txt"):
        a, b = (runs["off"] / f).read_bytes(), (runs["on"] / f).read_bytes()
        assert len(a) > 0 and a == b, f
    assert os.listdir(str(runs["off"] / "dyn")) == [] and len(os.listdir(str(runs["on"] / "dyn"))) == N_DYN


@pytest.mark.gpu
def test_frame_count_is_capped_on_the_host(pkg):
    lib = pkg.load_library()
    p = pkg.lk_default_params()
    assert lib.svo_lk_batch_dev(None, None, 200, 200, 180, 4097, C.byref(p), None, None, 10, None, None, None) == -5
    assert lib.svo_lk_chain_dev(None, None, 200, 200, 180, 4097, C.byref(p), None, None, 10, 10, None, None, None) == -5
