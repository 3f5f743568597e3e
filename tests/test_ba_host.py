"""The host side of the windowed bundle adjustment: stereo_kitti --local-ba (Tracking::LocalBA) and host/ba_check give the
library's poses (BundleAdjuster.window on the same records and poses) on three small frames."""
import importlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "stereo-semantic-vo_amd", "host")
N, W, K = 3, 1241, 500


def _write_pgm(path, img):
    with open(str(path), "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, np.uint8).tobytes())


@pytest.mark.gpu
def test_local_ba_and_ba_check_give_the_library_poses(pkg, tmp_path):
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    L, R, _ = synth.render_sequence(N)
    L, R = np.ascontiguousarray(L.numpy()), np.ascontiguousarray(R.numpy())
    # the library: the tracker's records and poses of the three frames, one window over them
    cam = pkg.Camera(**pkg.KITTI_00_02)
    ctx = pkg.Svo(W, L.shape[1], max_batch=N)
    ctx.track_reset(cam)
    raw = np.zeros(N * K * 32 + 16, np.uint8)
    obs = raw[(-raw.ctypes.data) % 16:][:N * K * 32]
    counts = np.zeros(N, np.int32)
    res = np.zeros(N, pkg.TRACK_DTYPE)
    ctx.track_map_out(obs, counts)
    ctx.track_batch_host(L.ctypes.data, R.ctypes.data, W, N, res)
    ctx.sync()
    ctx.close()
    rec = obs.view(pkg.MAP_OBS_DTYPE).reshape(N, K)
    par = pkg.BaParams.default(window=N)
    ba = pkg.BundleAdjuster(K, 1)
    T, pts, st = ba.window(cam, par, rec, counts, res["Tcw"].reshape(N, 4, 4))
    ba.close()
    assert int(st["status"]) == 0 and int(st["n_points"]) > 50 and float(st["chi2_final"]) <= float(st["chi2_initial"])

    # stereo_kitti --pipelined --write-map dir --local-ba 3
    seq = tmp_path / "seq"
    (seq / "image_0").mkdir(parents=True)
    (seq / "image_1").mkdir()
    for k in range(N):
        _write_pgm(seq / "image_0" / ("%06d.pgm" % k), L[k])
        _write_pgm(seq / "image_1" / ("%06d.pgm" % k), R[k])
    (seq / "times.txt").write_text("".join("%e\n" % (0.1 * k) for k in range(N)))
    y = tmp_path / "s.yaml"
    y.write_text("%YAML:1.0\nCamera.fx: 718.856\nCamera.fy: 718.856\nCamera.cx: 607.1928\nCamera.cy: 185.2157\n"
                 "Camera.width: 1241\nCamera.height: 376\nCamera.bf: 386.1448\n")
    d = tmp_path / "run"
    (d / "map").mkdir(parents=True)
    p = subprocess.run([os.path.join(HOST, "stereo_kitti"), "--write-map", str(d / "map"), "--local-ba", "3", "--pipelined", "voc", str(y),
                        str(seq), "3"], capture_output=True, text=True, cwd=str(d), timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = (d / "map" / "ba_000000.txt").read_text().splitlines()
    assert len(lines) == N + 1 and not (d / "map" / "ba_000001.txt").exists()
    for f in range(N):
        M = T[f]
        want = []
        for i in range(3):
            want += [M[0, i], M[1, i], M[2, i], -(M[0, i] * M[0, 3] + M[1, i] * M[1, 3] + M[2, i] * M[2, 3])]
        assert [float(v) for v in lines[f].split()] == [float(v) for v in want], f
    tail = lines[N].split()
    assert tail[0] == "#" and [int(v) for v in tail[1:8]] == [0] + [int(st[k]) for k in ("status", "n_points", "n_edges", "n_edges_stereo",
                                                                                      "iterations", "trials_total")]
    assert [float(v) for v in tail[8:]] == [float(st[k]) for k in ("chi2_initial", "chi2_final", "lambda_final")]
    # the option's refusals
    for bad in (["--local-ba", "3", "voc", str(y), str(seq)], ["--write-map", str(d / "map"), "--local-ba", "9", "--pipelined", "voc", str(y), str(seq)]):
        q = subprocess.run([os.path.join(HOST, "stereo_kitti")] + bad, capture_output=True, text=True, cwd=str(d), timeout=120)
        assert q.returncode == 1 and "--local-ba" in q.stderr

    # host/ba_check on the same records and poses
    with open(str(tmp_path / "records.bin"), "wb") as f:
        f.write(np.array([N, K], np.int32).tobytes() + counts.tobytes() + rec.tobytes())
    (tmp_path / "poses.txt").write_text("".join(" ".join("%.9g" % v for v in res["Tcw"][k]) + "\n" for k in range(N)))
    p = subprocess.run([os.path.join(HOST, "ba_check"), str(tmp_path / "records.bin"), str(tmp_path / "poses.txt")], capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout.splitlines()
    got = np.array([[float(v) for v in ln.split()] for ln in out[:N]]).reshape(N, 4, 4)
    assert got.tobytes() == T.tobytes()
    assert [int(v) for v in out[N].split()[1:7]] == [int(st[k]) for k in ("status", "n_points", "n_edges", "n_edges_stereo", "iterations",
                                                                          "trials_total")]
    rows = [ln.split() for ln in out[N + 1:]]
    assert [int(r[0]) for r in rows] == list(pts["gid"]) and [float(r[2]) for r in rows] == list(pts["X"])
