"""stereo_kitti --write-map / --write-cloud (Tracking::map_out): the pipelined and the frame-by-frame run write the same map."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from test_gating import boxes_for  # noqa: E402

N = 6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "stereo-semantic-vo_amd", "host", "stereo_kitti")


def _write_pgm(path, img):
    with open(str(path), "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, np.uint8).tobytes())


@pytest.mark.gpu
def test_pipelined_and_frame_by_frame_write_the_same_map(pkg, tmp_path):
    """Six frames with the box schedule of tests/test_gating.py, --pipelined in calls of 4 + 2 against frame by frame: the six
    NNNNNN.txt byte for byte; the PLY's vertex count is the number of `new = 1` lines, its vertices those lines' X Y Z in order;
    the trajectory files are those of the runs without the options."""
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    L, R, _ = synth.render_sequence(N)
    L, R = L.numpy(), R.numpy()
    seq = tmp_path / "seq"
    (seq / "image_0").mkdir(parents=True); (seq / "image_1").mkdir(); (seq / "boxes").mkdir()
    for k in range(N):
        _write_pgm(seq / "image_0" / ("%06d.pgm" % k), L[k]); _write_pgm(seq / "image_1" / ("%06d.pgm" % k), R[k])
        (seq / "boxes" / ("%d.txt" % (k + 1))).write_text("".join("%d %d %d %d\n" % tuple(b) for b in boxes_for(k)))
    (seq / "times.txt").write_text("".join("%e\n" % (0.1 * k) for k in range(N)))
    y = tmp_path / "s.yaml"
    y.write_text("%YAML:1.0\nCamera.fx: 718.856\nCamera.fy: 718.856\nCamera.cx: 607.1928\nCamera.cy: 185.2157\n"
                 "Camera.width: 1241\nCamera.height: 376\nCamera.bf: 386.1448\n")
    tail = ["voc", str(y), str(seq)]
    runs = {"pipe": ["--write-map", "MAP", "--write-cloud", "PLY", "--pipelined"] + tail + ["4"],
            "frame": ["--write-map", "MAP", "--write-cloud", "PLY"] + tail,
            "pipe_plain": ["--pipelined"] + tail + ["4"],
            "frame_plain": tail}
    for name, args in runs.items():
        d = tmp_path / name
        (d / "map").mkdir(parents=True)
        args = [str(d / "map") if a == "MAP" else str(d / "cloud.ply") if a == "PLY" else a for a in args]
        p = subprocess.run([EXE] + args, capture_output=True, text=True, cwd=str(d), timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
    new_lines = []
    for k in range(N):
        a = (tmp_path / "pipe" / "map" / ("%06d.txt" % k)).read_bytes()
        assert len(a) > 0 and a == (tmp_path / "frame" / "map" / ("%06d.txt" % k)).read_bytes(), k
        rows = [ln.split() for ln in a.decode().splitlines()]
        assert all(len(r) == 9 for r in rows)
        kps = [int(r[1]) for r in rows]
        assert kps == sorted(set(kps))
        new_lines += [r for r in rows if r[2] == "1"]
    assert os.listdir(str(tmp_path / "pipe_plain" / "map")) == [] and not (tmp_path / "pipe_plain" / "cloud.ply").exists()
    gids = [int(r[0]) for r in new_lines]
    assert len(gids) == len(set(gids)) > 100
    for name in ("pipe", "frame"):
        ply = (tmp_path / name / "cloud.ply").read_text().splitlines()
        assert ply[0] == "ply" and ply[1] == "format ascii 1.0" and ply[2] == "element vertex %d" % len(new_lines)
        body = ply[ply.index("end_header") + 1:]
        assert body == [" ".join(r[6:9]) for r in new_lines]
    for f in ("cameratrajectory_kitti.txt", "cameratrajectory_tum.txt"):
        for a, b in (("pipe", "pipe_plain"), ("frame", "frame_plain")):
            t = (tmp_path / a / f).read_bytes()
            assert len(t) > 0 and t == (tmp_path / b / f).read_bytes(), (a, f)
