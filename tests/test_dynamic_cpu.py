"""CPU suite of the dynamic-keypoint loop inside the tracker (svo_track_dynamic): the host-only entries, and the seed rule
restated in tests/dyn_ref.py against the CPU oracle's matching on the fixture the GPU tests use."""
import ctypes as C
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import dyn_ref  # noqa: E402
from test_gating import boxes_for  # noqa: E402

N = 6
# keypoints strictly inside a box / of those without a map point after both passes, per frame of the fixture
INSIDE = [120, 239, 250, 242, 241, 256]
NO_MP = [120, 237, 249, 239, 241, 256]


def test_default_params(pkg):
    p = pkg.dyn_default_params()
    assert (p.enable, p.colour, p.seed_frames, p.max_pts) == (0, 0, 2, 512)
    d = pkg.lk_default_params()
    assert (p.lk.winSize, p.lk.maxLevel, p.lk.maxCount, p.lk.epsilon, p.lk.minEigThreshold) == \
           (d.winSize, d.maxLevel, d.maxCount, d.epsilon, d.minEigThreshold)
    assert pkg.load_library().svo_dyn_default_params(None) == -1


def test_null_arguments_are_invalid(pkg):
    lib = pkg.load_library()
    p = pkg.dyn_default_params()
    lists = np.zeros(2 * 512, np.float32); counts = np.zeros(1, np.int32)
    assert lib.svo_track_dynamic(None, C.byref(p)) == -1
    assert lib.svo_track_dynamic(None, None) == -1
    assert lib.svo_track_dynamic_out(None, lists.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p), None) == -1


def test_seed_rule_on_the_fixture(pkg, orc):
    """orc.Tracker's keypoints and map-point indices through dyn_ref's seed rule: the counts the issue states - and at frame 1
    two inside keypoints HAVE a map point, so the "no map point" half of the rule is exercised."""
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    L, R, _ = synth.render_sequence(N)
    L, R = L.numpy(), R.numpy()
    assert L.shape[1:] == (376, 1241)
    cam = pkg.KITTI_00_02
    trk = orc.Tracker(L.shape[2], L.shape[1], cam)
    xy, has_mp = [], []
    for k in range(N):
        fe = orc.stereo_frame(L[k], R[k], cam["bf"], cam["fx"])
        res, cur = trk.track(L[k], R[k], boxes_for(k))
        kp = fe["kpL"]
        assert res["n_kp"] == len(kp)
        xy.append(np.stack([kp["x"], kp["y"]], 1).astype(np.float32)); has_mp.append(cur[:len(kp)] >= 0)
    trk.close()
    assert len(xy[0]) == 485
    for k in range(N):
        inside = dyn_ref.strictly_inside(xy[k], boxes_for(k))
        assert int(inside.sum()) == INSIDE[k], k
        assert int((inside & ~has_mp[k]).sum()) == NO_MP[k], k
    assert not has_mp[0].any()
    assert int((dyn_ref.strictly_inside(xy[1], boxes_for(1)) & has_mp[1]).sum()) == 2
    for k, want in ((0, (120, 120)), (1, (0, 237)), (2, (0, 0))):
        init, create = dyn_ref.frame_seeds(xy[k], has_mp[k], boxes_for(k), k)
        assert (len(init), len(create)) == want, k
    # the loop without a tracker that loses anything: 240 seeds at frame 0, 237 more at frame 1, the capacity rule cuts the end
    lists, counts, dropped = dyn_ref.loop(N, lambda k: xy[k], lambda k: has_mp[k], boxes_for, lambda k, p: (p, np.ones(len(p), np.uint8)),
                                          max_pts=300)
    assert counts.tolist() == [240, 300, 300, 300, 300, 300] and dropped.tolist() == [0, 177, 0, 0, 0, 0]
    assert lists[1, :240].tobytes() == lists[0, :240].tobytes()
    # a point on a box's edge is no seed
    assert not dyn_ref.strictly_inside(np.array([[500, 250]], np.float32), boxes_for(0))[0]
