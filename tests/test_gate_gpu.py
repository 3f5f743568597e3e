"""The semantic gate's kernels at their edges, on the device: svo_bf_match and svo_match_greedy_gated bit for bit against
the plain references of gate_ref.py, svo_fundamental_8point against the committed 50-digit fixture
(tests/golden/fmat_cases.npz, made by tests/golden/make_fmat_golden.py), and the tracker's own gate kernels (k_tg_bf,
k_tg_fmat and their grouped forms) on crafted front-end results against the oracle's tail and across device modes.

What is compared only up to scale and sign, and why: the 8-point contract fixes F[8] = 1 where |F[8]| > 1.19e-7 and returns
the de-normalised unit eigenvector otherwise, whose sign is the eigen-solver's business (pure translation: F is skew-symmetric,
F[8] = 0 up to rounding).  So F[8] == 1.0 is asserted exactly in the first branch, and entries are compared after Frobenius
normalisation and sign alignment in both; the gate's own quantity, the point-to-line distance, is invariant to both and is
compared directly.  Where the eigenvector itself is not unique (planar and collinear sets) only the residual and the rank are."""
import importlib
import os

import numpy as np
import pytest

import gate_cases
import gate_ref
import util

pytestmark = pytest.mark.gpu

FM = np.load(os.path.join(util.GOLDEN, "fmat_cases.npz"))
NAMES = [str(n) for n in FM["names"]]
TAGS = dict(zip(NAMES, (str(t) for t in FM["tags"])))
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def svo(pkg):
    s = pkg.Svo(640, 240, max_batch=1)
    yield s
    s.close()


# ---- a. svo_bf_match ---------------------------------------------------------------------------------------------------
def _bf_equal(svo, q, t):
    got, ref = svo.bf_match(q, t), gate_ref.bf_match_ref(q, t)
    for a, r in zip(got, ref):
        assert a.dtype == r.dtype and np.array_equal(a, r)
    return got


@pytest.mark.parametrize("M,N", gate_cases.BF_SHAPES)
def test_bf_match_shapes(svo, M, N):
    ti, d, keep = _bf_equal(svo, *gate_cases.bf_shape_case(M, N))
    if N == 0:
        assert list(ti) == [-1] * M and list(d) == [-1] * M and not keep.any()


def test_bf_match_capacity_ties_and_minima(svo, pkg):
    with pytest.raises(pkg.SvoError, match="capacity exceeded"):
        svo.bf_match(util.random_descriptors(1, 3), util.random_descriptors(2, 1025))
    for q, t in gate_cases.bf_tie_case():
        _bf_equal(svo, q, t)
    for gmin in (0, 16):
        q, t, thr = gate_cases.bf_minimum_case(gmin)
        ti, d, keep = _bf_equal(svo, q, t)
        assert list(d[:3]) == [gmin, thr, thr + 1] and list(keep) == [1, 1, 0, 0]


# ---- b. svo_match_greedy_gated ---------------------------------------------------------------------------------------------
def _gated(svo, c, **kw):
    return svo.match_greedy_gated(c["q"], c["t"], c["assigned"], c["max_dist"], c["ratio"], c["q_xy"], c["t_xy"],
                                  kw.pop("boxes", c["boxes"]), c["F"], q_skip=c["q_skip"], **kw)


def _gated_equal(svo, c, ref):
    got = _gated(svo, c)
    for k, (a, r) in enumerate(zip(got, ref[:6])):
        assert a.dtype == r.dtype and np.array_equal(a, r), (k, np.flatnonzero(a != r)[:8])
    return got


@pytest.mark.parametrize("M,N", gate_cases.GATED_SHAPES)
def test_greedy_gated_shapes(svo, M, N):
    """Every output array, `vetoed` included, on shapes around the lane count and the Npad 512 / 1024 switch, with skipped rows,
    pre-assigned columns and planted releases of a vetoed column."""
    c, ref = gate_cases.gated_case(M, N)
    got = _gated_equal(svo, c, ref)
    for i, j in c["release"]:
        assert got[5][i] == 1 and got[3][i + 1] == 1 and got[0][i + 1] == j


def test_greedy_gated_pass2_parameters_and_64_boxes(svo, pkg):
    _gated_equal(svo, *gate_cases.gated_case(64, 64, 30, 2.0))
    c, ref = gate_cases.gated_case(65, 65, many_boxes=True)
    _gated_equal(svo, c, ref)
    with pytest.raises(pkg.SvoError, match="invalid argument"):
        _gated(svo, c, boxes=np.concatenate([c["boxes"], c["boxes"][:1]]))


def test_greedy_gated_threshold_and_box_edges(svo):
    """0.1 px and the padded edges are strict: exact cases (the line is horizontal, the distance |cy - y0| has no rounding)."""
    c, ref, expect = gate_cases.threshold_case()
    assert np.array_equal(_gated_equal(svo, c, ref)[5], expect)
    c, ref, expect = gate_cases.box_edge_case()
    assert np.array_equal(_gated_equal(svo, c, ref)[5], expect)


def test_greedy_gated_zero_F_and_no_boxes(svo):
    c, ref = gate_cases.zero_F_case()
    got = _gated_equal(svo, c, ref)           # every distance NaN: no veto
    free = svo.match_greedy(c["q"], c["t"], c["assigned"], c["max_dist"], c["ratio"], q_skip=c["q_skip"])
    for a, r in zip(got[:5], free):
        assert np.array_equal(a, r)
    assert not got[5].any()
    dirty = np.full(len(c["q"]), 0xAA, np.uint8)
    out = _gated(svo, c, boxes=None, vetoed=dirty)
    assert out[5] is dirty and not dirty.any()
    for a, r in zip(out[:5], free):
        assert np.array_equal(a, r)


# ---- c. svo_fundamental_8point ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_8point_against_the_high_precision_fixture(svo, orc, name):
    p1, p2, F, lam, tag = FM[name + "/p1"], FM[name + "/p2"], FM[name + "/F"], FM[name + "/lam"], TAGS[name]
    Fd = svo.fundamental_8point(p1, p2)
    if tag == "zero":
        assert not Fd.any()
        return
    assert np.isfinite(Fd).all() and Fd.any()
    nrm = np.linalg.norm(Fd)
    assert abs(np.linalg.det(Fd)) <= 1e-12 * nrm ** 3                 # rank 2
    # the eigenvalue picked is a real one: a padding pick (or any other wrong column) leaves a residual of order
    # sqrt(lam9).  Floor: a backward-stable eigen-solver misses lam1 by at most 64 eps lam9.
    res_d, res_o = gate_ref.algebraic_residual(Fd, p1, p2), gate_ref.algebraic_residual(orc.fundamental_8point(p1, p2), p1, p2)
    print(name, "residual device", res_d, "oracle", res_o, "floor", np.sqrt(64 * EPS * lam[2]))
    assert res_d <= 1.0001 * res_o + np.sqrt(64 * EPS * lam[2])
    if tag == "ungapped":
        # planar / collinear sets: the null space of the normal matrix has more than one dimension, the "eigenvector of the
        # smallest eigenvalue" is whatever unit vector of it the sweep order lands on - entries are not comparable
        return
    if tag == "norm":
        assert Fd[2, 2] == 1.0
    else:                                                             # pure translation: the un-normalised branch
        assert abs(Fd[2, 2]) < 1.1920929e-07
    spread = float(np.linalg.norm(p1 - p1.mean(0), axis=1).mean())
    dev = np.array([gate_ref.entry_deviation(Fd, F), gate_ref.probe_deviation(Fd, F, FM[name + "/last"], FM[name + "/cur"], spread)])
    print(name, "device deviation", dev, "bound", FM[name + "/bound"], "oracle's", FM[name + "/dev"])
    assert (dev <= FM[name + "/bound"]).all(), (dev, FM[name + "/bound"])


# ---- d. the tracker's own gate kernels on crafted front-end results -------------------------------------------------------------
BIG = np.array([[200, 1000, 195, 370], [20, 120, 30, 90]], np.int32)          # the boxes of tests/test_gating.py
COUNTERS = ("n_kp", "n_stereo", "n_match_pass1", "n_match_pass2", "n_lm_edges", "n_new_mappoints", "n_local_map",
            "n_pnp_inliers", "lm_iterations")


@pytest.fixture(scope="module")
def frontend(orc, pkg):
    """The oracle's front-end results of the five synthetic frames of tests/test_gating.py: per frame (kp, desc, depth)."""
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    L, R, T = synth.render_sequence(5)
    L, R = L.numpy(), R.numpy()
    cam = pkg.KITTI_00_02
    fe = [orc.stereo_frame(L[k], R[k], cam["bf"], cam["fx"]) for k in range(5)]
    return L.shape[2], L.shape[1], [(f["kpL"], f["dL"], f["depth"]) for f in fe]


def _truncate(frames, counts):
    return [(kp[:n], d[:n], z[:n]) if n is not None else (kp, d, z) for (kp, d, z), n in zip(frames, counts)]


def _survivors(frames, k, boxes):
    """Current keypoints of frame k whose brute-force match is kept and which lie outside every padded box - what the
    8-point solve of frame k gets (by the plain references alone)."""
    ti, d, keep = gate_ref.bf_match_ref(frames[k][1], frames[k - 1][1])
    kp = frames[k][0]
    return [i for i in range(len(kp)) if keep[i] and not gate_ref.in_boxes_ref(kp["x"][i], kp["y"][i], boxes)]


def _box_leaving(frames, k, want):
    """One box over a half plane with an integer edge, chosen so that exactly `want` kept matches of frame k stay outside it."""
    ti, d, keep = gate_ref.bf_match_ref(frames[k][1], frames[k - 1][1])
    big = 100000
    for axis in ("x", "y"):
        v = frames[k][0][axis][keep != 0].astype(np.float64)
        for edge in range(int(v.min()) - 1, int(v.max()) + 2):
            # the box above the edge: outside iff v <= low - 10 = edge; the box below it: outside iff v >= high + 10 = edge
            for cnt, lo, hi in ((int((v <= edge).sum()), edge + 10, big), (int((v >= edge).sum()), -big, edge - 10)):
                if cnt == want:
                    box = np.array([[lo, hi, -big, big] if axis == "x" else [-big, big, lo, hi]], np.int32)
                    assert len(_survivors(frames, k, box)) == want
                    return box
    raise AssertionError("no integer edge leaves exactly %d matches" % want)


def _scenarios(W, H, frames):
    """name -> (frames, boxes per frame).  Frame 0 is never gated on the device side of F (no last frame); boxes from frame 1."""
    std = [np.zeros((0, 4), np.int32)] + [BIG] * 4
    out = {}
    n_full = [len(f[0]) for f in frames]
    assert min(n_full) > 400
    out["counts_500_65_500_7"] = (_truncate(frames, [None, 65, None, 7, None]), std)       # (500, 65), (65, 500), (500, 7)
    out["counts_64_500_63_64"] = (_truncate(frames, [64, None, 64, 63, 64]), std)          # (64, 500), (500, 64), (64, 63), (63, 64)
    everywhere = np.array([[-100, W + 100, -100, H + 100]], np.int32)
    out["boxes_cover_the_image"] = (frames, [std[0], BIG, everywhere, BIG, BIG])
    out["seven_survive"] = (frames, [std[0], BIG, _box_leaving(frames, 2, 7), BIG, BIG])
    out["eight_survive"] = (frames, [std[0], BIG, _box_leaving(frames, 2, 8), BIG, BIG])
    dup = [(kp, d.copy(), z) for kp, d, z in frames]
    for group in ([3, 67, 131, 200], [10, 74], [63, 64]):          # ties across trips of one lane and across lanes
        for j in group[1:]:
            dup[1][1][j] = dup[1][1][group[0]]
    out["duplicated_descriptors"] = (dup, std)
    far = np.array([[5000 + 10 * k, 5005 + 10 * k, 5000, 5005] for k in range(62)], np.int32)
    out["64_boxes_deciding_last"] = (frames, [std[0]] + [np.concatenate([far, BIG])] * 4)
    return out


SCENARIOS = ["counts_500_65_500_7", "counts_64_500_63_64", "boxes_cover_the_image", "seven_survive", "eight_survive",
             "duplicated_descriptors", "64_boxes_deciding_last"]


def _oracle_tail(orc, pkg, W, H, frames, boxes):
    trk = orc.Tracker(W, H, pkg.KITTI_00_02)
    out = []
    for (kp, d, z), b in zip(frames, boxes):
        res, cur, pnp, Tp = trk.track_tail(kp, d, z, boxes=b)
        out.append((res.copy(), cur.copy(), trk.F.copy(), trk.vetoes))
    trk.close()
    return out


def _pack(pkg, frames, boxes, dev):
    import torch
    N = len(frames)
    kp = np.zeros((N, 500), pkg.KP_DTYPE); desc = np.zeros((N, 500, 32), np.uint8)
    n = np.zeros(N, np.int32); depth = np.zeros((N, 500), np.float32)
    bx = np.zeros((N, 64, 4), np.int32); nb = np.zeros(N, np.int32)
    for k, ((a, d, z), b) in enumerate(zip(frames, boxes)):
        n[k] = len(a); kp[k, :len(a)] = a; desc[k, :len(a)] = d; depth[k, :len(a)] = z
        nb[k] = len(b); bx[k, :len(b)] = b
    t = dict(kp=torch.from_numpy(kp.view(np.uint8).reshape(N, 500, -1)).to(dev), desc=torch.from_numpy(desc).to(dev),
             n=torch.from_numpy(n).to(dev), depth=torch.from_numpy(depth).to(dev), bx=torch.from_numpy(bx).to(dev),
             nb=torch.from_numpy(nb).to(dev))
    torch.cuda.synchronize()
    return t


def _tail(pkg, s, t, first, count, res):
    rec = pkg.TRACK_DTYPE.itemsize
    bx = pkg.boxes_dev(t["bx"][first:].data_ptr(), t["nb"][first:].data_ptr(), 64)
    s.track_tail_dev(t["kp"][first:].data_ptr(), t["desc"][first:].data_ptr(), t["n"][first:].data_ptr(),
                     t["depth"][first:].data_ptr(), 500, count, res.data_ptr() + first * rec, boxes=bx)
    s.sync()


@pytest.fixture(scope="module")
def tracker_ctx(pkg, frontend):
    W, H, _ = frontend
    s = pkg.Svo(W, H, max_batch=5)
    yield s
    s.close()


@pytest.mark.parametrize("name", SCENARIOS)
def test_tracker_gate_on_crafted_frontend_results(orc, pkg, frontend, tracker_ctx, name):
    """k_tg_bf / k_tg_fmat (frame by frame, and gate_group 0) and k_tg_bf_group / k_tg_fmat_group (the batch) on keypoint
    counts around the lane count, no / seven / eight surviving matches, tied descriptors and 64 boxes: counters, matches, veto
    count and F against the oracle's tail on the same arrays, and records byte-identical across the device's modes."""
    import torch
    W, H, base = frontend
    frames, boxes = _scenarios(W, H, base)[name]
    ref = _oracle_tail(orc, pkg, W, H, frames, boxes)
    if name == "boxes_cover_the_image":
        assert not ref[2][2].any() and ref[2][3] == 0
    if name == "seven_survive":
        assert not ref[2][2].any()
    if name == "eight_survive":
        assert ref[2][2].any()
    dev = torch.device("cuda", 0)
    cam = pkg.Camera(**pkg.KITTI_00_02)
    N = len(frames)
    rec = pkg.TRACK_DTYPE.itemsize
    t = _pack(pkg, frames, boxes, dev)
    s = tracker_ctx
    s.set_option("gate_group", 1)
    s.track_reset(cam)
    res = torch.zeros((N, rec), dtype=torch.uint8, device=dev)
    for k in range(N):                                     # frame by frame
        _tail(pkg, s, t, k, 1, res)
        r = res[k].cpu().numpy().view(pkg.TRACK_DTYPE)[0]
        want, want_cur, want_F, want_vetoes = ref[k]
        for f in COUNTERS:
            assert r[f] == want[f], (name, k, f, r[f], want[f])
        cur = s.debug_track_matches()
        assert np.array_equal(cur[:want["n_kp"]], want_cur[:want["n_kp"]]), (name, k)
        if k > 0:
            F, nv = s.debug_track_gate()
            print(name, k, "vetoes", nv, want_vetoes, "F deviation", np.abs(F.reshape(9) - want_F).max())
            if not want_F.any():
                assert not F.any(), (name, k)
            assert np.allclose(F.reshape(9), want_F, rtol=1e-6, atol=1e-9), (name, k)
            assert nv == want_vetoes, (name, k, nv, want_vetoes)
    single = res.cpu().numpy().tobytes()
    F1, nv1 = s.debug_track_gate()
    for group in (1, 0):                                   # the batch, grouped gate kernels and per-frame ones
        s.set_option("gate_group", group)
        s.track_reset(cam)
        out = torch.zeros((N, rec), dtype=torch.uint8, device=dev)
        _tail(pkg, s, t, 0, N, out)
        assert out.cpu().numpy().tobytes() == single, (name, group)
        F2, nv2 = s.debug_track_gate()
        assert nv2 == nv1 and np.array_equal(F1, F2), (name, group)
    s.set_option("gate_group", 1)
    assert s.track_overflowed() == 0
