"""The host tools of the rectification stage against the Python path: host/rect_check on one written pair, stereo_kitti --rectify
(Tracking::LoadRectification: Track() through svo_rect_process, TrackBatch() through svo_rect_batch_dev(consumer) +
svo_track_batch_dev) on three written raw frames against the same driver on the frames Rectifier.process made of them."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import rect_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "stereo-semantic-vo_amd", "host")
W, H, N = 640, 240, 3


def write_pnm(path, img):
    with open(path, "wb") as f:
        f.write(b"%s\n%d %d\n255\n" % (b"P5" if img.ndim == 2 else b"P6", img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img).tobytes())


def read_pnm(path):
    data = open(path, "rb").read()
    magic, wh, _, rest = data.split(b"\n", 3)
    w, h = (int(v) for v in wh.split())
    return np.frombuffer(rest, np.uint8).reshape((h, w) if magic == b"P5" else (h, w, 3))


def test_host_tool_is_built():
    assert os.path.exists(os.path.join(HOST, "rect_check")), "run __graft_entry__.build() first"


def test_rect_check_refuses_bad_settings(tmp_path):
    """No device is needed to get as far as the settings file."""
    bad = tmp_path / "bad.yaml"
    bad.write_text(open(os.path.join(rr.GOLDEN, "rect_euroc_like.yaml")).read().replace("LEFT.P:", "LEFT.Q:"))
    p = subprocess.run([os.path.join(HOST, "rect_check"), str(bad), "l.pgm", "r.pgm", "ol", "or"], capture_output=True, text=True)
    assert p.returncode == 1 and "LEFT.P" in p.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("cn", [1, 3])
def test_rect_check_equals_python(pkg, tmp_path, cn):
    settings = os.path.join(rr.GOLDEN, "rect_euroc_like.yaml")
    L, R = (a[0] for a in rr.case_sources("euroc", cn))
    ext = "pgm" if cn == 1 else "ppm"
    # (a PPM holds RGB; the tool hands the library BGR, like cv::imread: the same three planes either way)
    write_pnm(str(tmp_path / ("l." + ext)), L if cn == 1 else L[..., ::-1])
    write_pnm(str(tmp_path / ("r." + ext)), R if cn == 1 else R[..., ::-1])
    p = subprocess.run([os.path.join(HOST, "rect_check"), settings, str(tmp_path / ("l." + ext)), str(tmp_path / ("r." + ext)),
                        str(tmp_path / ("ol." + ext)), str(tmp_path / ("or." + ext))], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    rect = pkg.Rectifier.from_settings(settings)
    wantL, wantR = rect.process(L, R)
    rect.close()
    gotL, gotR = read_pnm(str(tmp_path / ("ol." + ext))), read_pnm(str(tmp_path / ("or." + ext)))
    if cn == 3:
        gotL, gotR = gotL[..., ::-1], gotR[..., ::-1]
    assert np.array_equal(gotL, wantL) and np.array_equal(gotR, wantR)
    # ... which is the restatement's image (the C++ parser read the same calibration as the Python loader)
    assert np.array_equal(wantL, rr.remap(L, rr.case_maps("euroc")[0][3])[0])


SETTINGS = """%%YAML:1.0
Camera.fx: %(fx)r
Camera.fy: %(fy)r
Camera.cx: %(cx)r
Camera.cy: %(cy)r
Camera.width: 640
Camera.height: 240
Camera.bf: 209.6
"""
RAW_KEYS = """Camera.k1: -0.05
Camera.k2: 0.01
Camera.p1: 0.0005
Camera.p2: -0.0003
"""


@pytest.mark.gpu
def test_stereo_kitti_rectify_equals_rectified_sequence(pkg, tmp_path):
    """Three raw frames and a flat-key calibration (R = I, P = K).  stereo_kitti --rectify on the raw files, frame by frame and
    --pipelined, writes the trajectory the plain driver writes on the frames Rectifier.process made of them: the same rows frame
    by frame (the same images go through the same code), and within the existing pipelined-against-frame tolerance otherwise."""
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    cam = dict(fx=400.0, fy=400.0, cx=319.5, cy=119.5)
    L, R, _ = synth.render_sequence(N, cam=dict(W=W, H=H, bf=215.0, **cam))
    L, R = L.numpy(), R.numpy()
    y = tmp_path / "raw.yaml"
    y.write_text(SETTINGS % cam + RAW_KEYS)
    s = pkg.load_rect_settings(str(y))
    rect = pkg.Rectifier(W, H, s["left"], s["right"])
    for name, make in (("raw", lambda a, b: (a, b)), ("rectified", rect.process)):
        seq = tmp_path / name
        (seq / "image_0").mkdir(parents=True); (seq / "image_1").mkdir()
        for k in range(N):
            a, b = make(L[k], R[k])
            write_pnm(str(seq / "image_0" / ("%06d.pgm" % k)), a)
            write_pnm(str(seq / "image_1" / ("%06d.pgm" % k)), b)
        (seq / "times.txt").write_text("".join("%e\n" % (0.1 * k) for k in range(N)))
    rect.close()
    plain = tmp_path / "plain.yaml"
    plain.write_text(SETTINGS % cam)   # (P = K: the rectified camera is the file's)
    out = {}
    for mode, args in (("reference", ["voc", str(plain), str(tmp_path / "rectified")]),
                       ("frame", ["--rectify", str(y), "voc", str(y), str(tmp_path / "raw")]),
                       ("pipelined", ["--rectify", str(y), "--pipelined", "voc", str(y), str(tmp_path / "raw"), "2"])):
        d = tmp_path / ("run_" + mode)
        d.mkdir()
        p = subprocess.run([os.path.join(HOST, "stereo_kitti")] + args, capture_output=True, text=True, cwd=str(d))
        assert p.returncode == 0, mode + ": " + p.stdout + p.stderr
        out[mode] = (open(str(d / "cameratrajectory_kitti.txt")).read(), np.loadtxt(str(d / "cameratrajectory_kitti.txt")))
    assert out["reference"][1].shape == (N, 12)
    assert out["frame"][0] == out["reference"][0]
    assert np.abs(out["pipelined"][1] - out["reference"][1]).max() < 1e-4
    assert out["reference"][1][-1, 11] > 1.0, "the rectified frames no longer track (two metres of travel)"
