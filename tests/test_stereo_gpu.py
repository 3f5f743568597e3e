"""GPU suite (-m gpu): k_stereo_match and k_stereo_median on the hand-made keypoints of tests/stereo_cases.py, through
svo_debug_stereo_match, against orc_stereo_match (uR, depth: bit for bit) and the numpy twin tests/stereo_ref.py (the best SAD
before the median cut); and svo_stereo_frame on images of 600, 1100 and 2100 rows, where the matcher's 512 row buckets hold 2, 4
and 8 rows each.  tests/test_stereo_cpu.py shows without a GPU that every case reaches the branch it was made for."""
import ctypes as C

import numpy as np
import pytest

import stereo_cases
import util

pytestmark = pytest.mark.gpu


def same_kp(a, b):
    assert len(a) == len(b)
    for f in ("x", "y", "size", "angle", "response", "octave", "class_id"):
        assert a[f].tobytes() == b[f].tobytes(), f


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", stereo_cases.NAMES)
def test_debug_stereo_match_equals_oracle_and_twin(pkg, orc, name):
    c = stereo_cases.CASES[name]
    twin, uR_o, depth_o = stereo_cases.reference(name, orc)
    nL = len(c["kpL"])
    cam = pkg.Camera(c["fx"], c["fx"], c["W"] / 2.0, c["H"] / 2.0, c["bf"])
    svo = pkg.Svo(c["W"], c["H"], max_kp=c["max_kp"], max_batch=1)
    uR, depth, sad = svo.debug_stereo_match(c["L"], c["R"], cam, c["kpL"], c["dL"], c["kpR"], c["dR"])
    again = svo.debug_stereo_match(c["L"], c["R"], cam, c["kpL"], c["dL"], c["kpR"], c["dR"])
    svo.close()
    assert len(uR) == len(depth) == len(sad) == c["max_kp"]
    bad = np.flatnonzero((bits(uR[:nL]) != bits(uR_o)) | (bits(depth[:nL]) != bits(depth_o)) | (sad[:nL] != twin["sad"]))
    print(name, "differing keypoints:", [(int(i), twin["reason"][i], float(uR[i]), float(uR_o[i]), int(sad[i]), int(twin["sad"][i]))
                                         for i in bad[:8]])
    assert np.array_equal(bits(uR[:nL]), bits(uR_o))
    assert np.array_equal(bits(depth[:nL]), bits(depth_o))
    assert np.array_equal(sad[:nL], twin["sad"])
    assert (uR[nL:] == -1).all() and (depth[nL:] == -1).all() and (sad[nL:] == -1).all()
    for a, b in zip((uR, depth, sad), again):
        assert a.tobytes() == b.tobytes()


def test_debug_stereo_match_rejects_invalid_arguments(pkg, orc):
    c = stereo_cases.CASES["median_nd3"]
    W, H, K = c["W"], c["H"], c["max_kp"]
    cam = pkg.Camera(c["fx"], c["fx"], W / 2.0, H / 2.0, c["bf"])
    svo = pkg.Svo(W, H, max_kp=K, max_batch=1)

    def run(**kw):
        a = dict({k: c[k] for k in ("kpL", "dL", "kpR", "dR")}, **kw)
        return svo.debug_stereo_match(c["L"], c["R"], cam, a["kpL"], a["dL"], a["kpR"], a["dR"])

    good = run()
    for side, dside in (("kpL", "dL"), ("kpR", "dR")):
        for field, bad in (("octave", 8), ("octave", -1), ("x", np.nan), ("y", np.nan), ("x", np.inf), ("y", -np.inf), ("y", -1.0),
                           ("y", float(H)), ("x", -W - 1.0), ("x", 2.0 * W + 1.0)):
            k = c[side].copy()
            k[field][1] = bad
            with pytest.raises(pkg.SvoError):
                run(**{side: k})
        many = np.zeros(K + 1, c[side].dtype)            # more than max_kp
        many["y"] = 5.0
        with pytest.raises(pkg.SvoError):
            run(**{side: many, dside: np.zeros((K + 1, 32), np.uint8)})
    out = [np.zeros(K, np.float32), np.zeros(K, np.float32), np.zeros(K, np.int32)]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    L, R = np.ascontiguousarray(c["L"]), np.ascontiguousarray(c["R"])
    for nL, nR, stride in ((-1, 3, W), (3, -1, W), (3, 3, W - 1)):
        assert svo.lib.svo_debug_stereo_match(svo.h, p(L), stride, p(R), W, C.byref(cam), p(c["kpL"]), p(c["dL"]), nL, p(c["kpR"]),
                                              p(c["dR"]), nR, p(out[0]), p(out[1]), p(out[2])) == -1
    k = c["kpL"].copy()                                  # the limits themselves are legal (x < 0: no candidate, the gate under test)
    k["x"][0], k["x"][1], k["y"][2] = -W, 2 * W, np.nextafter(np.float32(H), np.float32(0))
    uR, depth, sad = run(kpL=k)
    assert (uR[:3] == -1).all() and (sad[:3] == -1).all()
    for a, b in zip(good, run()):                        # and the context is as usable as before
        assert a.tobytes() == b.tobytes()
    svo.close()


@pytest.mark.parametrize("W,H,shift", [(160, 600, 1), (128, 1100, 2), (96, 2100, 3)])
def test_stereo_frame_tall_images_bit_exact(pkg, orc, W, H, shift):
    """512 rows and more: the matcher's row buckets hold 2^shift rows; ORB's own keypoints, the whole frame against the oracle."""
    assert 256 <= (H >> shift) < 512
    L, R = util.shifted_pair(W * 7 + H, W, H, disparity=9)
    cam = pkg.Camera(**pkg.KITTI_00_02)
    s = pkg.Svo(W, H, max_batch=1)
    g = s.stereo_frame(L, R, cam)
    s.close()
    r = orc.stereo_frame(L, R, cam.bf, cam.fx)
    same_kp(g["kpL"], r["kpL"]); same_kp(g["kpR"], r["kpR"])
    assert np.array_equal(g["dL"], r["dL"]) and np.array_equal(g["dR"], r["dR"])
    assert np.array_equal(g["uR"].view(np.uint32), r["uR"].view(np.uint32))
    assert np.array_equal(g["depth"].view(np.uint32), r["depth"].view(np.uint32))
    assert len(g["kpL"]) > 200 and (g["depth"] > 0).sum() > 100
    assert g["kpL"]["y"].max() > 0.9 * H and g["kpL"]["y"].min() < 0.1 * H        # keypoints, and so buckets, from top to bottom
