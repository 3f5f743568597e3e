"""numpy restatement of what svo_track_map_out's records must hold (tests/test_map_cpu.py, tests/test_map_gpu.py).

float32 / float64 exactly where k_tp_frame has them (csrc/svo_track.hip, "SetPose (CV_32F ...)" and tk_unproject):
  SetPose     Rwc = transpose of the record's float32 rotation, twc[i] = (float)-((double)Rwc[3i] T[3] + (double)Rwc[3i+1] T[7]
              + (double)Rwc[3i+2] T[11]), the sum left to right;
  unproject   x = (u - cx) * z * (1 / fx), y likewise, all float32, one rounding per operation; world[r] = (float)((double)Rwc[3r] x
              + (double)Rwc[3r+1] y + (double)Rwc[3r+2] z + (double)twc[r]), the sum left to right; a row with z <= 0 has no point.
"""
import numpy as np

MAP_NEW = 1
OBS = np.dtype([("gid", "<i4"), ("kp", "<i2"), ("flags", "<u2"), ("u", "<f4"), ("v", "<f4"), ("depth", "<f4"),
                ("X", "<f4"), ("Y", "<f4"), ("Z", "<f4")])
IDENTITY = np.eye(4, dtype=np.float32).reshape(16)


def set_pose(Tcw):
    """(Rwc (9,), twc (3,)) float32 of a record's float32 Tcw (16, row-major)."""
    T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
    Rwc = np.array([T[4 * (i % 3) + i // 3] for i in range(9)], np.float32)
    twc = np.zeros(3, np.float32)
    for i in range(3):
        acc = np.float64(Rwc[3 * i]) * np.float64(T[3]) + np.float64(Rwc[3 * i + 1]) * np.float64(T[7])
        acc = acc + np.float64(Rwc[3 * i + 2]) * np.float64(T[11])
        twc[i] = np.float32(-acc)
    return Rwc, twc


def unproject(uvz, cam, Rwc, twc):
    """uvz (n, 3) float32, cam (fx, fy, cx, cy) -> (xyz (n, 3) float32, valid (n,) bool); rows with z <= 0 are skipped (xyz 0)."""
    uvz = np.ascontiguousarray(uvz, np.float32).reshape(-1, 3)
    fx, fy, cx, cy = (np.float32(v) for v in cam[:4])
    u, v, z = uvz[:, 0], uvz[:, 1], uvz[:, 2]
    one = np.float32(1)
    x = ((u - cx) * z).astype(np.float32) * (one / fx)
    y = ((v - cy) * z).astype(np.float32) * (one / fy)
    x = x.astype(np.float32); y = y.astype(np.float32)
    R = np.ascontiguousarray(Rwc, np.float32).reshape(9).astype(np.float64)
    t = np.ascontiguousarray(twc, np.float32).reshape(3).astype(np.float64)
    xd, yd, zd = x.astype(np.float64), y.astype(np.float64), z.astype(np.float64)
    out = np.zeros((len(uvz), 3), np.float32)
    for r in range(3):
        acc = R[3 * r] * xd + R[3 * r + 1] * yd
        acc = acc + R[3 * r + 2] * zd
        out[:, r] = (acc + t[r]).astype(np.float32)
    valid = z > 0
    out[~valid] = 0
    return out, valid


def expected(frame_id, match_gid, new_gid, kp_xy, depth, cam, Tcw, positions):
    """The record list of one frame.  match_gid / new_gid: per keypoint (svo_debug_track_frames), kp_xy (n, 2) and depth (n,)
    float32: the frame's keypoints and what its depth source gave them, Tcw: the frame's result record's pose, positions: dict
    gid -> float32 (3,) of the points that exist - the frame's new points are added to it.  New points are placed with the
    identity pose at frame 0 (Tracking::init) and with the frame's SetPose otherwise (frame::createmappoint)."""
    n = len(kp_xy)
    match_gid = np.asarray(match_gid)[:n]; new_gid = np.asarray(new_gid)[:n]
    assert not ((match_gid >= 0) & (new_gid >= 0)).any(), "per keypoint exactly one of matched / created"
    Rwc, twc = set_pose(IDENTITY if frame_id == 0 else Tcw)
    uvz = np.concatenate([np.asarray(kp_xy, np.float32).reshape(n, 2), np.asarray(depth, np.float32).reshape(n, 1)], 1)
    world, valid = unproject(uvz, cam, Rwc, twc)
    out = []
    for j in range(n):
        if match_gid[j] >= 0:
            gid, new = int(match_gid[j]), frame_id == 0
        elif new_gid[j] >= 0:
            gid, new = int(new_gid[j]), True
        else:
            continue
        if new:
            assert valid[j] and gid not in positions, (frame_id, j, gid)
            positions[gid] = world[j].copy()
        p = positions[gid]
        out.append((gid, j, MAP_NEW if new else 0, uvz[j, 0], uvz[j, 1], uvz[j, 2], p[0], p[1], p[2]))
    return np.array(out, OBS) if out else np.zeros(0, OBS)
