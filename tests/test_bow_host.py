"""The host side of the bag of words: host/bow_check against the twin on one frame; stereo_kitti --bow (Tracking::LoadVocabulary,
Tracking::LoopCandidates) on three 640 x 240 frames writes the vectors the Python entry gives; --pipelined --bow refuses."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import bow_cases as Cs  # noqa: E402
import bow_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "stereo-semantic-vo_amd", "host")
N, W, H = 3, 640, 240


def _write_pgm(path, img):
    with open(str(path), "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, np.uint8).tobytes())


def _parse(lines):
    """the "n_features n_words n_pairs" block of bow_check / --write-bow -> (words, vec, fv)"""
    n, nv, nf = (int(v) for v in lines[0].split())
    words = np.array([int(v) for v in lines[1].split()], np.int32)
    assert len(words) == n and len(lines) == 2 + nv + nf
    vec = np.zeros(nv, R.ENTRY)
    for i, ln in enumerate(lines[2:2 + nv]):
        vec[i] = (int(ln.split()[0]), 0, float(ln.split()[1]))
    fv = np.array([tuple(int(v) for v in ln.split()) for ln in lines[2 + nv:]], R.FEATURE).reshape(nf)
    return words, vec, fv


@pytest.mark.gpu
def test_bow_check_against_the_twin(tmp_path):
    c = Cs.walk_ragged(True)
    v = c["voc"]
    (tmp_path / "voc.txt").write_text(R.format_text(v))
    c["descs"].tofile(str(tmp_path / "desc.bin"))
    for ls in (0, 2):
        p = subprocess.run([os.path.join(HOST, "bow_check"), str(tmp_path / "voc.txt"), str(tmp_path / "desc.bin"), str(ls)],
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        out = p.stdout.splitlines()
        d = v.describe()
        assert [int(x) for x in out[0].split()[1:]] == [d["k"], d["L"], d["nodes"], d["words"], d["weighting"]]
        words, vec, fv = _parse(out[1:])
        rw, rvec, rfv = R.transform(v, c["descs"], ls)
        assert np.array_equal(words, rw) and vec.tobytes() == rvec.tobytes() and fv.tobytes() == rfv.tobytes(), ls
    (tmp_path / "bad.txt").write_text("4 3  1 0\n")
    p = subprocess.run([os.path.join(HOST, "bow_check"), str(tmp_path / "bad.txt"), str(tmp_path / "desc.bin")], capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 1 and "line 1: scoring" in p.stderr


def _sequence(tmp_path):
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    L, Rr, _ = synth.render_sequence(N)
    L = np.ascontiguousarray(L.numpy()[:, 100:100 + H, 300:300 + W])
    Rr = np.ascontiguousarray(Rr.numpy()[:, 100:100 + H, 300:300 + W])
    seq = tmp_path / "seq"
    (seq / "image_0").mkdir(parents=True)
    (seq / "image_1").mkdir()
    for k in range(N):
        _write_pgm(seq / "image_0" / ("%06d.pgm" % k), L[k])
        _write_pgm(seq / "image_1" / ("%06d.pgm" % k), Rr[k])
    (seq / "times.txt").write_text("".join("%e\n" % (0.1 * k) for k in range(N)))
    y = tmp_path / "s.yaml"
    y.write_text("%YAML:1.0\nCamera.fx: 718.856\nCamera.fy: 718.856\nCamera.cx: 607.1928\nCamera.cy: 185.2157\n"
                 "Camera.width: 640\nCamera.height: 240\nCamera.bf: 386.1448\n")
    return L, Rr, seq, y


@pytest.mark.gpu
def test_stereo_kitti_bow_writes_the_library_vectors(pkg, tmp_path):
    L, Rr, seq, y = _sequence(tmp_path)
    v = R.random_tree(7, 10, 5, ragged=0.5, stop=0.05)
    (tmp_path / "voc.txt").write_text(R.format_text(v))
    # the Python entry on the same frames' descriptors
    cam = pkg.Camera(**pkg.KITTI_00_02)
    svo = pkg.Svo(W, H, max_batch=1)
    voc = pkg.Vocabulary.from_text(str(tmp_path / "voc.txt"))
    want = []
    for k in range(N):
        d = svo.stereo_frame(L[k], Rr[k], cam)["dL"]
        assert 100 < len(d) <= 500
        want.append(voc.transform(d, 4))
        tw = R.transform(v, d, 4)
        assert np.array_equal(want[k][0], tw[0]) and want[k][1].tobytes() == tw[1].tobytes() and want[k][2].tobytes() == tw[2].tobytes()
    svo.close()
    voc.close()
    d = tmp_path / "run"
    (d / "bow").mkdir(parents=True)
    p = subprocess.run([os.path.join(HOST, "stereo_kitti"), "--bow", str(tmp_path / "voc.txt"), "--write-bow", str(d / "bow"), "--loop-candidates",
                        str(d / "loops.txt"), "--loop-gap", "0", "--loop-top", "2", "ignored_vocabulary", str(y), str(seq)],
                       capture_output=True, text=True, cwd=str(d), timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    for k in range(N):
        words, vec, fv = _parse((d / "bow" / ("%06d.txt" % k)).read_text().splitlines())
        assert np.array_equal(words, want[k][0]) and vec.tobytes() == want[k][1].tobytes() and fv.tobytes() == want[k][2].tobytes(), k
    cand, cnt = R.query([w[1] for w in want], 0, N, 0, 0.0, 2)
    lines = (d / "loops.txt").read_text().splitlines()
    at = 0
    for k in range(N):
        assert lines[at].split() == [str(k), str(cnt[k])]
        for i in range(cnt[k]):
            f, s = lines[at + 1 + i].split()
            assert int(f) == cand[k, i]["frame"] and float(s) == cand[k, i]["score"]
        at += 1 + cnt[k]
    assert at == len(lines) and cnt.tolist() == [0, 1, 2]


def test_stereo_kitti_bow_refusals(tmp_path):
    """answered from the command line alone: no device, no sequence"""
    exe = os.path.join(HOST, "stereo_kitti")
    for args, needle in ((["--pipelined", "--bow", Cs.TINY, "voc", "s.yaml", "seq"], "--bow: frame by frame only"),
                         (["--bow", Cs.TINY, "--pipelined", "voc", "s.yaml", "seq", "8"], "--bow: frame by frame only"),
                         (["--write-bow", "dir", "voc", "s.yaml", "seq"], "need --bow"),
                         (["--loop-candidates", "f.txt", "voc", "s.yaml", "seq"], "need --bow"),
                         (["--bow", Cs.TINY, "--loop-top", "17", "voc", "s.yaml", "seq"], "--loop-top")):
        p = subprocess.run([exe] + args, capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
        assert p.returncode == 1 and needle in p.stderr, (args, p.stderr)
