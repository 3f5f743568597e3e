"""GPU suite of the bag of words (svo_bow_*; csrc/svo_bow.hip) against the numpy twin (tests/bow_ref.py) on the cases of
tests/bow_cases.py.  Everything is compared bit for bit, no tolerance: words, nodes, counts and the bytes of every double; outputs
stand between guard bytes, and what lies behind a frame's length stays untouched."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import bow_cases as Cs  # noqa: E402
import bow_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0xA5
PAD = 256


def lib_voc(pkg, v, **kw):
    return pkg.Vocabulary.from_arrays(v.k, v.L, v.weighting, v.parent, v.desc, v.weight, **kw)


def guarded(torch, nbytes):
    return torch.full((nbytes + 2 * PAD,), GUARD, dtype=torch.uint8, device="cuda")


def inner(t, nbytes):
    a = t.cpu().numpy()
    assert (a[:PAD] == GUARD).all() and (a[PAD + nbytes:] == GUARD).all(), "guard bytes written"
    return a[PAD:PAD + nbytes].copy()


def run_transform(pkg, voc, frames, stride, levelsup=0, counts=None, outputs=("words", "vec", "vec_n", "fv", "fv_n"), producer=None):
    """frames: a list of (n_i, 32) arrays -> dict of the raw outputs (B, stride, ..) / (B,) that were asked for"""
    import torch
    B = len(frames)
    desc = np.full((B, stride, 32), 0x5A, np.uint8)
    n = np.zeros(B, np.int32)
    for f, d in enumerate(frames):
        m = min(len(d), stride)
        desc[f, :m] = d[:m]
        n[f] = len(d)
    if counts is not None:
        n[:] = counts
    d_desc, d_n = torch.from_numpy(desc).cuda(), torch.from_numpy(n).cuda()
    size = dict(words=B * stride * 4, vec=B * stride * 16, vec_n=B * 4, fv=B * stride * 8, fv_n=B * 4)
    out = {k: guarded(torch, size[k]) for k in outputs}
    torch.cuda.synchronize()
    ptr = {k: (out[k].data_ptr() + PAD if k in out else None) for k in size}
    voc.transform_dev(d_desc, d_n, stride, B, levelsup, ptr["words"], ptr["vec"], ptr["vec_n"], ptr["fv"], ptr["fv_n"], producer=producer)
    voc.sync()
    raw = {k: inner(out[k], size[k]) for k in outputs}
    dt = dict(words=np.int32, vec=pkg.BOW_ENTRY_DTYPE, vec_n=np.int32, fv=pkg.BOW_FEATURE_DTYPE, fv_n=np.int32)
    return {k: raw[k].view(dt[k]).reshape((B, stride) if k in ("words", "vec", "fv") else (B,)) for k in outputs}


def check_frames(got, v, frames, stride, levelsup=0, what=""):
    """every output that is there against the twin, frame by frame"""
    guard16 = np.full(16, GUARD, np.uint8).tobytes()
    for f, d in enumerate(frames):
        d = d[:stride]
        w, vec, fv = R.transform(v, d, levelsup)
        tag = "%s frame %d (n = %d)" % (what, f, len(d))
        if "words" in got:
            assert np.array_equal(got["words"][f, :len(d)], w), tag
            assert (got["words"][f, len(d):] == -1).all(), tag
        if "vec_n" in got:
            assert got["vec_n"][f] == len(vec), tag
        if "fv_n" in got:
            assert got["fv_n"][f] == len(fv), tag
        if "vec" in got:
            assert got["vec"][f, :len(vec)].tobytes() == vec.tobytes(), tag
            assert got["vec"][f, len(vec):].tobytes() == guard16 * (stride - len(vec)), tag + ": written behind the vector"
        if "fv" in got:
            assert got["fv"][f, :len(fv)].tobytes() == fv.tobytes(), tag
            assert got["fv"][f, len(fv):].tobytes() == guard16[:8] * (stride - len(fv)), tag + ": written behind the FeatureVector"


# ---- walk ------------------------------------------------------------------------------------------------------------------------------
WALKS = [(2, 1, 0), (2, 3, 0), (2, 6, 0), (3, 1, 0), (3, 3, 0), (3, 6, 0), (10, 1, 0), (10, 3, 0), (10, 6, 0.6), (16, 1, 0), (16, 3, 0),
         (16, 6, 0.75), (17, 1, 0), (17, 3, 0), (17, 6, 0.75), (20, 1, 0), (20, 3, 0), (20, 6, 0.75)]


@pytest.mark.parametrize("k,L,ragged", WALKS, ids=["k%d-L%d" % (k, L) for k, L, _ in WALKS])
def test_walk(pkg, k, L, ragged):
    """groups narrower than, equal to and wider than 16 lanes; 1, 3 and 6 dependent levels; distance 0 and 256"""
    c = Cs.walk_random(k, L, ragged)
    c["prove"]()
    voc = lib_voc(pkg, c["voc"], max_kp=128)
    for ls in (0, 1):
        check_frames(run_transform(pkg, voc, [c["descs"]], 128, ls), c["voc"], [c["descs"]], 128, ls, "levelsup %d" % ls)
    voc.close()


@pytest.mark.parametrize("which", ["first", "last", "all"])
def test_walk_ties(pkg, which):
    c = Cs.walk_ties(which)
    c["prove"]()
    voc = lib_voc(pkg, c["voc"], max_kp=16)
    got = run_transform(pkg, voc, [c["descs"]], 16)
    check_frames(got, c["voc"], [c["descs"]], 16)
    assert (got["words"][0, :len(c["descs"])] == {"first": 0, "last": 3, "all": 0}[which]).all()
    voc.close()


@pytest.mark.parametrize("shuffle", [False, True], ids=["ids-in-order", "ids-interleaved"])
def test_walk_ragged_and_levelsup(pkg, tmp_path, shuffle):
    """a leaf at level 1 beside leaves at level L, stop words; levelsup 0, 2, L and L + 1; the interleaved ids come through the file"""
    c = Cs.walk_ragged(shuffle)
    c["prove"]()
    v = c["voc"]
    p = tmp_path / "voc.txt"
    p.write_text(R.format_text(v))
    voc = pkg.Vocabulary.from_text(str(p), max_kp=128)
    assert voc.describe() == v.describe()
    for ls in (0, 2, v.L, v.L + 1):
        got = run_transform(pkg, voc, [c["descs"]], 128, ls)
        check_frames(got, v, [c["descs"]], 128, ls, "levelsup %d" % ls)
        if ls >= v.L:
            assert (got["fv"][0, :got["fv_n"][0]]["node"] == 0).all()
    voc.close()


def test_tiny_vocabulary_by_hand(pkg):
    """the hand-computed examples of tests/test_bow_cpu.py, on the device"""
    voc = pkg.Vocabulary.from_text(Cs.TINY, max_kp=8)
    descs = np.stack([Cs.flat(b) for b in (0x30, 0x07, 0x03, 0x07, 0x01, 0x07, 0x11)])
    words, vec, fv = voc.transform(descs, levelsup=1)
    assert words.tolist() == [10, 1, -1, 1, 0, 1, 0]
    assert vec["word"].tolist() == [0, 1, 10] and vec["value"].tolist() == [1.0 / 4.875, 3.75 / 4.875, 0.125 / 4.875]
    assert [tuple(x) for x in fv.tolist()] == [(3, 4), (3, 6), (4, 1), (4, 3), (4, 5), (13, 0)]
    assert [tuple(x) for x in voc.transform(descs[:1], levelsup=0)[2].tolist()] == [(15, 0)]
    assert [tuple(x) for x in voc.transform(descs[1:2], levelsup=0)[2].tolist()] == [(4, 0)]      # a leaf above level 3: the leaf
    assert [tuple(x) for x in voc.transform(descs[:2], levelsup=3)[2].tolist()] == [(0, 0), (0, 1)]
    w, vec, fv = voc.transform(descs[:0])
    assert len(w) == 0 and len(vec) == 0 and len(fv) == 0
    voc.close()


@pytest.mark.parametrize("k", [1, 2, 20])
def test_assign(pkg, k):
    import torch
    voc = pkg.Vocabulary.from_text(Cs.TINY)
    rng = np.random.default_rng(k)
    centres = Cs.rand_desc(40 + k, k)
    if k == 20:
        centres[7] = centres[3]
        centres[19] = centres[18]
    for n in (1, 63, 64, 65):
        descs = Cs.near(n, centres, n, flips=int(rng.integers(0, 90)))
        descs[0] = centres[-1]
        if n > 1:
            descs[1] = ~centres[0]
        idx, dist = guarded(torch, 4 * n), guarded(torch, 4 * n)
        d_desc, d_c = torch.from_numpy(descs).cuda(), torch.from_numpy(centres).cuda()
        torch.cuda.synchronize()
        voc.assign_dev(d_desc, n, d_c, k, idx.data_ptr() + PAD, dist.data_ptr() + PAD)
        voc.sync()
        ri, rd = R.assign(descs, centres)
        assert np.array_equal(inner(idx, 4 * n).view(np.int32), ri), (k, n)
        assert np.array_equal(inner(dist, 4 * n).view(np.int32), rd), (k, n)
        if k == 20:
            assert ri[0] == 18 and rd[0] == 0
    voc.close()


# ---- vectors ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vec_case():
    v = Cs.vec_voc()
    return v, Cs.vec_frames(v, [0, 1, 2, 63, 64, 65, 500])


def test_vector_lengths(pkg, vec_case):
    """n = 0, 1, 2, 63, 64, 65 and 500 in one call of 7 frames, and each alone (B = 1)"""
    v, frames = vec_case
    voc = lib_voc(pkg, v, max_kp=512, max_frames=8)
    check_frames(run_transform(pkg, voc, frames, 512), v, frames, 512, what="B = 7")
    for f in frames:
        check_frames(run_transform(pkg, voc, [f], 500), v, [f], 500, what="B = 1")
    voc.close()


def test_vector_count_is_clamped(pkg, vec_case):
    """kp_stride 512 with a count of 600, a negative count"""
    v, _ = vec_case
    frames = Cs.vec_frames(v, [512, 512], seed=33)
    voc = lib_voc(pkg, v, max_kp=512, max_frames=2)
    got = run_transform(pkg, voc, frames, 512, counts=[600, -3])
    check_frames(got, v, [frames[0], frames[1][:0]], 512)
    voc.close()


@pytest.mark.parametrize("B", [2, 37])
def test_vector_batches(pkg, vec_case, B):
    v, _ = vec_case
    rng = np.random.default_rng(B)
    frames = Cs.vec_frames(v, [int(x) for x in rng.integers(0, 130, B)], seed=200 + B)
    voc = lib_voc(pkg, v, max_kp=160, max_frames=40)
    check_frames(run_transform(pkg, voc, frames, 130), v, frames, 130)
    voc.close()


@pytest.mark.parametrize("name", ["vec_repeat500", "vec_all_different", "vec_all_stopped", "vec_stop_mixed", "vec_norm_order"])
def test_vector_cases(pkg, name):
    c = getattr(Cs, name)()
    c["prove"]()
    voc = lib_voc(pkg, c["voc"], max_kp=512)
    got = run_transform(pkg, voc, [c["descs"]], 512)
    check_frames(got, c["voc"], [c["descs"]], 512, what=name)
    if name == "vec_all_stopped":
        assert got["vec_n"][0] == 0 and got["fv_n"][0] == 0 and (got["words"] == -1).all()
    w, vec, fv = voc.transform(c["descs"])
    rw, rvec, rfv = R.transform(c["voc"], c["descs"])
    assert np.array_equal(w, rw) and vec.tobytes() == rvec.tobytes() and fv.tobytes() == rfv.tobytes(), "the host entry"
    voc.close()


@pytest.mark.parametrize("weighting", [R.TF_IDF, R.TF, R.IDF, R.BINARY])
def test_weightings(pkg, weighting):
    v = Cs.vec_voc(weighting, stop=0.1)
    frames = Cs.vec_frames(v, [150, 40], seed=91, dup=0.5)
    voc = lib_voc(pkg, v, max_kp=160, max_frames=2)
    assert voc.describe()["weighting"] == weighting
    check_frames(run_transform(pkg, voc, frames, 160), v, frames, 160)
    voc.close()


def test_every_output_alone(pkg, vec_case):
    v, frames = vec_case
    frames = frames[2:6]
    voc = lib_voc(pkg, v, max_kp=80, max_frames=4)
    for k in ("words", "vec", "vec_n", "fv", "fv_n"):
        check_frames(run_transform(pkg, voc, frames, 80, outputs=(k,)), v, frames, 80, what=k + " alone")
    voc.close()


# ---- scores and queries ------------------------------------------------------------------------------------------------------------------
def upload_vecs(vecs, stride):
    import torch
    arr, n = Cs.pack(vecs, stride)
    return torch.from_numpy(arr.view(np.uint8).reshape(-1)).cuda(), torch.from_numpy(n).cuda()


def dense_scores(voc, dA, nA, QA, dB, nB, NB, stride):
    import torch
    out = guarded(torch, QA * NB * 8)
    torch.cuda.synchronize()
    voc.score_dev(dA, nA, QA, dB, nB, NB, stride, out.data_ptr() + PAD)
    voc.sync()
    return inner(out, QA * NB * 8).view(np.float64).reshape(QA, NB)


def test_scores(pkg):
    """1 against 500, 63 / 64 / 65 against each other, 0 against anything, disjoint vectors (-0.0), a common word only at the first /
    only at the last entry, every vector against itself: the bytes of the twin's doubles"""
    c = Cs.score_sets()
    c["prove"]()
    voc = pkg.Vocabulary.from_text(Cs.TINY, max_kp=512)
    dA, nA = upload_vecs(c["A"], 500)
    dB, nB = upload_vecs(c["B"], 500)
    got = dense_scores(voc, dA, nA, len(c["A"]), dB, nB, len(c["B"]), 500)
    want = R.scores(c["A"], c["B"])
    assert got.tobytes() == want.tobytes()
    assert np.signbit(got[6, 7]) and got[6, 7] == 0.0 and got[0].tobytes() == np.full(len(c["B"]), -0.0).tobytes()
    both = c["A"] + c["B"]
    dC, nC = upload_vecs(both, 500)
    self_scores = dense_scores(voc, dC, nC, len(both), dC, nC, len(both), 500)
    assert self_scores.tobytes() == R.scores(both, both).tobytes()
    voc.close()


def run_query(pkg, voc, dV, nV, stride, N, q0, Q, gap, min_score, top_k):
    import torch
    cand, cnt = guarded(torch, Q * top_k * 16), guarded(torch, Q * 4)
    torch.cuda.synchronize()
    voc.query_dev(dV, nV, stride, N, q0, Q, gap, min_score, top_k, cand.data_ptr() + PAD, cnt.data_ptr() + PAD)
    voc.sync()
    return inner(cand, Q * top_k * 16).view(pkg.BOW_CAND_DTYPE).reshape(Q, top_k), inner(cnt, Q * 4).view(np.int32)


@pytest.fixture(scope="module")
def qdb():
    c = Cs.query_db()
    c["prove"]()
    n = len(c["vecs"])
    c["scores"] = R.scores(c["vecs"], c["vecs"])
    return c, n


def test_query(pkg, qdb):
    """gaps that leave a query no frame, one frame, exactly top_k frames; planted equal scores; top_k 1 and 16; min_score equal to
    a score; query_dev == the twin's query == score_dev followed by the twin's selection"""
    c, N = qdb
    vecs, S = c["vecs"], c["scores"]
    voc = pkg.Vocabulary.from_text(Cs.TINY, max_kp=128)
    dV, nV = upload_vecs(vecs, 96)
    dense = dense_scores(voc, dV, nV, N, dV, nV, N, 96)
    assert dense.tobytes() == S.tobytes()
    eq = float(S[N - 1, 2])                      # the score of the planted duplicates 2, 9, 17, 25 against the last frame
    for q0, Q, gap, ms, k in ((N - 4, 4, 0, -1.0, 16), (N - 4, 4, 3, -1.0, 1), (0, N, 0, 0.0, 4), (0, N, 5, 0.05, 3), (N - 1, 1, 0, eq, 16),
                              (N - 1, 1, N - 1, -1.0, 4), (N - 1, 1, N - 2, -1.0, 4), (N - 1, 1, N - 5, -1.0, 4), (N - 1, 1, N + 7, -1.0, 4),
                              (7, 9, 2, 0.1, 2)):
        cand, cnt = run_query(pkg, voc, dV, nV, 96, N, q0, Q, gap, ms, k)
        rc, rn = R.query(vecs, q0, Q, gap, ms, k)
        what = (q0, Q, gap, ms, k)
        assert np.array_equal(cnt, rn), what
        assert cand.tobytes() == rc.tobytes(), what
        for i in range(Q):                       # and from the device's own dense scores
            sc, sn = R.select(dense[q0 + i], q0 + i, gap, ms, k)
            assert sn == cnt[i] and sc.tobytes() == cand[i].tobytes(), what
    cand, cnt = run_query(pkg, voc, dV, nV, 96, N, N - 1, 1, 0, -1.0, 16)
    dup = [int(f) for f in cand["frame"][0] if f in (2, 9, 17, 25)]
    assert dup == [2, 9, 17, 25], "equal scores by ascending frame"
    assert (S[N - 1, cand["frame"][0, :cnt[0]]] == cand["score"][0, :cnt[0]]).all()
    cand, cnt = run_query(pkg, voc, dV, nV, 96, N, N - 1, 1, 0, eq, 16)
    assert (cand["score"][0, :cnt[0]] > eq).all() and not set(cand["frame"][0].tolist()) & {2, 9, 17, 25}, "min_score is a strict bound"
    assert run_query(pkg, voc, dV, nV, 96, N, N - 1, 1, N - 1, -1.0, 4)[1][0] == 0
    assert run_query(pkg, voc, dV, nV, 96, N, N - 1, 1, N - 2, -1.0, 4)[1][0] == 1
    assert run_query(pkg, voc, dV, nV, 96, N, N - 1, 1, N - 5, -1.0, 4)[1][0] == 4
    voc.close()


def test_query_of_one_frame(pkg, qdb):
    """N = 1: the only frame has no earlier one"""
    c, _ = qdb
    voc = pkg.Vocabulary.from_text(Cs.TINY, max_kp=128)
    dV, nV = upload_vecs(c["vecs"][:1], 96)
    cand, cnt = run_query(pkg, voc, dV, nV, 96, 1, 0, 1, 0, -1.0, 4)
    assert cnt[0] == 0 and cand.tobytes() == R.query(c["vecs"][:1], 0, 1, 0, -1.0, 4)[0].tobytes()
    assert cand["frame"].tolist() == [[-1] * 4] and cand["score"].tobytes() == np.zeros(4).tobytes()
    voc.close()


# ---- hand-over from the front end -----------------------------------------------------------------------------------------------------------
def test_hand_over_from_the_front_end(pkg):
    """svo_frontend_batch_dev on 6 synthetic 640 x 240 pairs, followed at once by svo_bow_transform_dev(producer = ctx) with no
    host synchronisation in between == the twin on the downloaded descriptors, the same bytes on three runs; the tracker's
    records over the same frames are the same bytes with and without the svo_bow calls."""
    import torch
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    N, W, H, K = 6, 640, 240, 500
    L, Rr, _ = synth.render_sequence(N)
    dL = L[:, 100:100 + H, 300:300 + W].contiguous().cuda()
    dR = Rr[:, 100:100 + H, 300:300 + W].contiguous().cuda()
    cam = pkg.Camera(**pkg.KITTI_00_02)
    v = R.random_tree(7, 10, 3, stop=0.05)
    rec = pkg.TRACK_DTYPE.itemsize
    torch.cuda.synchronize()

    def run(with_bow):
        ctx = pkg.Svo(W, H, max_kp=K, max_batch=N)
        ctx.track_reset(cam)
        voc = lib_voc(pkg, v, max_kp=K, max_frames=N)
        voc.stream       # (the object's device side exists before the front end call: nothing but the calls in between)
        kp = torch.zeros((N, K, 28), dtype=torch.uint8, device="cuda")
        desc = torch.zeros((N, K, 32), dtype=torch.uint8, device="cuda")
        n = torch.zeros((N,), dtype=torch.int32, device="cuda")
        uR = torch.zeros((N, K), dtype=torch.float32, device="cuda")
        depth = torch.zeros((N, K), dtype=torch.float32, device="cuda")
        res = torch.zeros((N, rec), dtype=torch.uint8, device="cuda")
        words = torch.full((N, K), -7, dtype=torch.int32, device="cuda")
        vec = torch.zeros((N, K, 16), dtype=torch.uint8, device="cuda")
        fv = torch.zeros((N, K, 8), dtype=torch.uint8, device="cuda")
        vec_n = torch.zeros((N,), dtype=torch.int32, device="cuda")
        fv_n = torch.zeros((N,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.frontend_batch_dev(dL.data_ptr(), dR.data_ptr(), W, N, cam, kp.data_ptr(), desc.data_ptr(), n.data_ptr(), uR.data_ptr(),
                               depth.data_ptr())
        if with_bow:
            voc.transform_dev(desc, n, K, N, 1, words, vec, vec_n, fv, fv_n, producer=ctx)
        ctx.track_tail_dev(kp.data_ptr(), desc.data_ptr(), n.data_ptr(), depth.data_ptr(), K, N, res.data_ptr())
        voc.sync()
        ctx.sync()
        out = dict(res=res.cpu().numpy().tobytes(), desc=desc.cpu().numpy(), n=n.cpu().numpy(), words=words.cpu().numpy(),
                   vec=vec.cpu().numpy().reshape(-1).view(pkg.BOW_ENTRY_DTYPE).reshape(N, K), vec_n=vec_n.cpu().numpy(),
                   fv=fv.cpu().numpy().reshape(-1).view(pkg.BOW_FEATURE_DTYPE).reshape(N, K), fv_n=fv_n.cpu().numpy())
        voc.close()
        ctx.close()
        return out

    plain = run(False)
    runs = [run(True) for _ in range(3)]
    for r in runs:
        assert r["res"] == plain["res"], "the tracker's records changed"
        for key in ("desc", "n", "words", "vec", "vec_n", "fv", "fv_n"):
            assert r[key].tobytes() == runs[0][key].tobytes(), key
    r = runs[0]
    assert (r["n"] > 100).all() and np.array_equal(r["desc"], plain["desc"])
    for f in range(N):
        d = r["desc"][f, :r["n"][f]]
        w, vec, fv = R.transform(v, d, 1)
        assert np.array_equal(r["words"][f, :len(d)], w) and (r["words"][f, len(d):] == -1).all()
        assert r["vec_n"][f] == len(vec) > 20 and r["vec"][f, :len(vec)].tobytes() == vec.tobytes()
        assert r["fv_n"][f] == len(fv) and r["fv"][f, :len(fv)].tobytes() == fv.tobytes()


# ---- training --------------------------------------------------------------------------------------------------------------------------------
def test_training_tool_cpu_and_device_write_the_same_file(pkg, tmp_path):
    """tools/bow_train.py with --cpu and on the device from the same 3,000 seeded descriptors (k = 5, L = 3)"""
    rng = np.random.default_rng(17)
    descs = Cs.near(18, Cs.rand_desc(19, 60), 3000, flips=20)
    bounds = np.sort(rng.choice(np.arange(1, 3000), 29, replace=False))
    np.save(tmp_path / "desc.npy", descs)
    np.save(tmp_path / "bounds.npy", np.concatenate([[0], bounds, [3000]]))
    tool = os.path.join(ROOT, "tools", "bow_train.py")
    args = [sys.executable, tool, "--descriptors", str(tmp_path / "desc.npy"), "--documents", str(tmp_path / "bounds.npy"), "--k", "5",
            "--L", "3", "--seed", "4", "--weighting", "0"]
    subprocess.check_call(args + ["--cpu", "--out", str(tmp_path / "cpu.txt")])
    subprocess.check_call(args + ["--out", str(tmp_path / "gpu.txt")])
    a, b = (tmp_path / "cpu.txt").read_bytes(), (tmp_path / "gpu.txt").read_bytes()
    assert a == b and len(a) > 1000
    v = R.parse_text(a.decode())
    assert v.describe()["k"] == 5 and v.describe()["words"] > 60
    docs = [descs[s:e] for s, e in zip(np.concatenate([[0], bounds]), np.concatenate([bounds, [3000]]))]
    assert R.format_text(R.train(docs, 5, 3, R.TF_IDF, 4)).encode() == a
