"""The host side of loop verification: host/loop_check on a dump of two frames prints what the Python entry (LoopVerifier.verify)
and the twin give, with and without the refit; a bad file is refused.  stereo_kitti --loop-verify (Tracking::VerifyLoop) on four
frames writes what the Python entries give on the same frames."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import loop_cases as Cs  # noqa: E402
import loop_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "stereo-semantic-vo_amd", "host")


def dump(path, sc, f):
    S, So = sc["desc"].shape[1], sc["obs"].shape[1]
    with open(str(path), "wb") as out:
        out.write(np.array([S, So], np.int32).tobytes())
        out.write(np.array([Cs.CAM[k] for k in ("fx", "fy", "cx", "cy")], np.float32).tobytes())
        for k in ("desc", "kp", "n", "fv", "fv_n", "obs", "obs_n", "Tcw"):
            out.write(np.ascontiguousarray(sc[k][f]).tobytes())


@pytest.mark.gpu
def test_loop_check_against_the_python_entry_and_the_twin(pkg, tmp_path):
    c = Cs.planted(50, sizes=[(60, 50), (30, 40), (1, 0), (0, 2), (25, 25)])
    sc = c["scene"]
    dump(tmp_path / "pair.bin", sc, [0, 1])
    ver = pkg.LoopVerifier(max_kp=sc["desc"].shape[1], max_pairs=1)
    cam = pkg.Camera(bf=0.0, **Cs.CAM)
    for refine in (0, 1):
        P = R.params(refine=refine)
        p = subprocess.run([os.path.join(HOST, "loop_check"), str(tmp_path / "pair.bin"), str(refine)], capture_output=True, text=True,
                           timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        out = p.stdout.splitlines()
        m, res, inl = ver.verify(cam, pkg.LoopParams.default(**P), sc["desc"][:2], sc["kp"][:2], sc["n"][:2], sc["fv"][:2], sc["fv_n"][:2],
                                 sc["obs"][:2], sc["obs_n"][:2], sc["Tcw"][:2])
        want = R.verify(sc, [(0, 1)], Cs.CAM, P)
        assert np.array_equal(m, want[0][0]) and res.tobytes() == want[2][0].tobytes() and np.array_equal(inl, want[3][0])
        assert res["status"] == R.OK and res["n_inliers"] > 20
        head = [int(v) for v in out[0].split()]
        assert head == [res[k] for k in ("status", "n_matches", "bound", "visited", "winner", "n_inliers")] + list(res["sample"])
        assert np.array([float(v) for v in out[1].split()]).tobytes() == res["T12"].tobytes()      # %.17g round-trips a double
        assert [int(v) for v in out[2].split()] == list(m) and [int(v) for v in out[3].split()] == list(inl)
    ver.close()
    (tmp_path / "short.bin").write_bytes(open(str(tmp_path / "pair.bin"), "rb").read()[:1000])
    p = subprocess.run([os.path.join(HOST, "loop_check"), str(tmp_path / "short.bin")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "shorter" in p.stderr


def test_loop_check_is_built():
    assert os.access(os.path.join(HOST, "loop_check"), os.X_OK), "run __graft_entry__.build() first"


N, W, H = 4, 640, 240


@pytest.mark.gpu
def test_stereo_kitti_loop_verify_writes_the_python_entrys_results(pkg, tmp_path):
    """stereo_kitti --bow .. --write-map .. --loop-candidates .. --loop-verify (Tracking::VerifyLoop) on four 640 x 240 frames: every
    candidate's line is what LoopVerifier.verify gives on the same frames' keypoints, descriptors, FeatureVectors, map records and
    tracked poses, taken through the Python entries"""
    import bow_ref
    import test_bow_host as B
    keep, B.N = B.N, N
    try:
        L, Rr, seq, y = B._sequence(tmp_path)
    finally:
        B.N = keep
    v = bow_ref.random_tree(7, 10, 5, ragged=0.5, stop=0.05)
    (tmp_path / "voc.txt").write_text(bow_ref.format_text(v))
    cam = pkg.Camera(**pkg.KITTI_00_02)
    fe, tr = pkg.Svo(W, H, max_batch=1), pkg.Svo(W, H, max_batch=1)
    tr.track_reset(cam)
    voc = pkg.Vocabulary.from_text(str(tmp_path / "voc.txt"))
    S = 500
    sc = Cs.scene(N, S)
    vecs = []
    for k in range(N):
        g = fe.stereo_frame(L[k], Rr[k], cam)
        n = len(g["kpL"])
        assert 100 < n <= S
        sc["n"][k], sc["kp"][k][:n], sc["desc"][k][:n] = n, g["kpL"], g["dL"]
        _, vec, fv = voc.transform(g["dL"], 4)
        vecs.append(vec)
        sc["fv"][k][:len(fv)], sc["fv_n"][k] = fv, len(fv)
        obs, cnt = np.zeros(S, pkg.MAP_OBS_DTYPE), np.zeros(1, np.int32)
        tr.track_map_out(obs, cnt)
        res = tr.track_frame(L[k], Rr[k], 0.1 * k)
        sc["obs"][k], sc["obs_n"][k], sc["Tcw"][k] = obs, cnt[0], res["Tcw"]
    cand, cnt = bow_ref.query(vecs, 0, N, 0, 0.0, 2)
    ver = pkg.LoopVerifier(max_kp=S, max_pairs=1)
    want = []
    for k in range(N):
        for i in range(cnt[k]):
            f = [k, int(cand[k, i]["frame"])]
            m, r, _ = ver.verify(cam, pkg.LoopParams.default(), sc["desc"][f], sc["kp"][f], sc["n"][f], sc["fv"][f], sc["fv_n"][f],
                                 sc["obs"][f], sc["obs_n"][f], sc["Tcw"][f])
            tw = R.verify(dict(sc), [f], pkg.KITTI_00_02, R.params())
            assert np.array_equal(m, tw[0][0]) and r.tobytes() == tw[2][0].tobytes()
            want.append((k, f[1], r))
    for o in (fe, tr, voc, ver):
        o.close()
    d = tmp_path / "run"
    (d / "map").mkdir(parents=True)
    p = subprocess.run([os.path.join(HOST, "stereo_kitti"), "--bow", str(tmp_path / "voc.txt"), "--write-map", str(d / "map"),
                        "--loop-candidates", str(d / "loops.txt"), "--loop-gap", "0", "--loop-top", "2", "--loop-verify", str(d / "verify.txt"),
                        "ignored_vocabulary", str(y), str(seq)], capture_output=True, text=True, cwd=str(d), timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = (d / "verify.txt").read_text().splitlines()
    assert len(lines) == len(want) == 5
    for ln, (k, c, r) in zip(lines, want):
        t = ln.split()
        assert [int(x) for x in t[:5]] == [k, c, r["status"], r["n_matches"], r["n_inliers"]], ln
        assert np.array([float(x) for x in t[5:]]).tobytes() == r["T12"].tobytes(), ln
    assert max(r["n_matches"] for _, _, r in want) > 20


def test_stereo_kitti_loop_verify_refusals(tmp_path):
    """answered from the command line alone: no device, no sequence"""
    exe = os.path.join(HOST, "stereo_kitti")
    tiny = os.path.join(ROOT, "tests", "golden", "bow_tiny_voc.txt")
    for args in (["--bow", tiny, "--loop-verify", "v.txt", "voc", "s.yaml", "seq"],
                 ["--bow", tiny, "--loop-candidates", "c.txt", "--loop-verify", "v.txt", "voc", "s.yaml", "seq"]):
        p = subprocess.run([exe] + args, capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
        assert p.returncode == 1 and "--loop-verify needs --loop-candidates and --write-map" in p.stderr, (args, p.stderr)
