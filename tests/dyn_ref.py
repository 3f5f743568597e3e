"""The dynamic-keypoint loop of the reference's Tracking::Track (src/Tracking.cc:189-223, seeds at src/Tracking.cc:70-85 and
src/frame.cc:209-222) restated in numpy - what svo_track_dynamic runs inside the tracker:

    list(f) = survivors(f) ++ init_seeds(f) ++ create_seeds(f)        (cut at max_pts)

The tracker itself (calcOpticalFlowPyrLK) is handed in as a function, so the same loop serves the CPU test (seed rule alone)
and the GPU tests (driven by the single-pair entries)."""
import numpy as np


def strictly_inside(xy, boxes):
    """xy: n x 2 float32; boxes: m x 4 (left, right, top, bottom).  u > left && u < right && v > top && v < bottom, no padding."""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    m = np.zeros(len(xy), bool)
    for b in np.asarray(boxes, np.int32).reshape(-1, 4):
        m |= (xy[:, 0] > b[0]) & (xy[:, 0] < b[1]) & (xy[:, 1] > b[2]) & (xy[:, 1] < b[3])
    return m


def can_seed(frame_id, seed_frames):
    return seed_frames < 0 or frame_id < seed_frames


def frame_seeds(xy, has_mp, boxes, frame_id, seed_frames=2):
    """(init_seeds, create_seeds) of one frame, each n x 2 float32 in keypoint order."""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    inside = strictly_inside(xy, boxes)
    none = xy[:0]
    init = xy[inside] if (frame_id == 0 and seed_frames != 0) else none
    create = xy[inside & ~np.asarray(has_mp, bool)] if can_seed(frame_id, seed_frames) else none
    return init, create


def append(cur, seeds, max_pts):
    """k_lk_compact's append: seeds while the list has room, the rest dropped from the end.  -> (list, dropped)"""
    take = min(len(seeds), max_pts - len(cur))
    return np.concatenate([cur, seeds[:take]]).astype(np.float32), len(seeds) - take


def loop(n_frames, xy_of, has_mp_of, boxes_of, track, seed_frames=2, max_pts=512):
    """The whole loop.  track(k, pts) -> (next_pts, status): pts followed from left image k - 1 into left image k.
    -> lists (n_frames x max_pts x 2 float32, unused entries 0), counts, dropped (int32)."""
    lists = np.zeros((n_frames, max_pts, 2), np.float32)
    counts = np.zeros(n_frames, np.int32); dropped = np.zeros(n_frames, np.int32)
    cur = np.zeros((0, 2), np.float32)
    for k in range(n_frames):
        if k > 0 and len(cur):
            nx, st = track(k, cur)
            cur = np.asarray(nx, np.float32).reshape(-1, 2)[np.asarray(st) != 0]
        init, create = frame_seeds(xy_of(k), has_mp_of(k), boxes_of(k), k, seed_frames)
        cur, dropped[k] = append(cur, np.concatenate([init, create]), max_pts)
        lists[k, :len(cur)] = cur; counts[k] = len(cur)
    return lists, counts, dropped
