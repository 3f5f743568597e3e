"""GPU suite of the dynamic-keypoint loop in the many-sequence tracker mode (svo_track_dynamic, then svo_track_multi_reset;
svo_track_multi_step_dev / svo_track_multi_step_bgr_dev).

Sequence q walks the synthetic frames q, q + 1, ... with a box schedule of its own.  Every expectation comes from EXISTING code:
S single-sequence contexts with the loop on, fed each sequence's frames and boxes through svo_track_batch[_bgr]_dev (itself held
to tests/dyn_ref.py by tests/test_dynamic_dev_gpu.py), and for sequence 0 also dyn_ref.loop over svo_lk_track[_bgr] directly.
Lists are compared as uint32 views over the used entries, counts and dropped exactly, records as bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from test_dynamic_dev_gpu import Fixture, params, N, W, H, PITCH, BPITCH  # noqa: E402
from test_gating import boxes_for, BIG  # noqa: E402

NONE = np.zeros((0, 4), np.int32)
SMALL = np.array([[560, 700, 220, 300]], np.int32)
BSTRIDE = 4


def sched_none(k):
    return NONE


def sched_small(k):
    return SMALL


def sched_late(k):
    """the first boxes arrive at step 2: create-seeds only, never init-seeds"""
    return NONE if k < 2 else BIG


@pytest.fixture(scope="module")
def fx(pkg):
    f = Fixture(pkg)
    f._single = {}
    yield f
    f.close()


def _boxes(torch, scheds, T):
    """step t, sequence q: scheds[q](t) -> device arrays (T x S x BSTRIDE x 4, T x S)"""
    S = len(scheds)
    b = np.zeros((T, S, BSTRIDE, 4), np.int32); n = np.zeros((T, S), np.int32)
    for t in range(T):
        for q in range(S):
            bq = scheds[q](t)
            b[t, q, :len(bq)] = bq; n[t, q] = len(bq)
    return torch.from_numpy(b).cuda(), torch.from_numpy(n).cuda()


def single(fx, q, T, sched, kind="gray", dyn=True, **kw):
    """The expectation for one sequence: a single-sequence context with the same svo_dyn_params over frames q .. q + T - 1 and the
    boxes sched(0 .. T - 1), one svo_track_batch[_bgr]_dev call.  -> lists (T x max_pts x 2), counts, dropped, records (T byte
    strings).  Computed once per key."""
    key = (q, T, sched.__name__, kind, dyn, tuple(sorted(kw.items())))
    if key not in fx._single:
        torch, pkg = fx.torch, fx.pkg
        mp = kw.get("max_pts", 512)
        dL, dR = fx.dev(kind)
        pitch = PITCH if kind == "gray" else BPITCH
        tb, tn = _boxes(torch, [sched], T)
        rec = pkg.TRACK_DTYPE.itemsize
        res = torch.zeros((T, rec), dtype=torch.uint8, device="cuda")
        lists = torch.zeros((T, mp, 2), dtype=torch.float32, device="cuda")
        counts = torch.zeros(T, dtype=torch.int32, device="cuda"); dropped = torch.zeros(T, dtype=torch.int32, device="cuda")
        ctx = pkg.Svo(W, H, max_batch=T)
        if dyn:
            ctx.track_dynamic(params(pkg, **kw))
        ctx.track_reset(fx.cam)
        if dyn:
            ctx.track_dynamic_out(lists.data_ptr(), counts.data_ptr(), dropped.data_ptr())
        entry = ctx.track_batch_dev if kind == "gray" else ctx.track_batch_bgr_dev
        entry(dL.data_ptr() + q * H * pitch, dR.data_ptr() + q * H * pitch, pitch, T, res.data_ptr(),
              boxes=pkg.boxes_dev(tb.data_ptr(), tn.data_ptr(), BSTRIDE))
        ctx.sync()
        torch.cuda.synchronize()
        r = res.cpu().numpy()
        fx._single[key] = (lists.cpu().numpy(), counts.cpu().numpy(), dropped.cpu().numpy(), [r[t].tobytes() for t in range(T)])
        ctx.close()
    return fx._single[key]


def multi(fx, ctx, scheds, T, kind="gray", max_pts=512, attach=None, with_dropped=True, with_boxes=True, frames=None):
    """T steps of len(scheds) sequences on a context that was reset for them, no synchronisation between the steps.  attach[t]
    False: step t gets no svo_track_dynamic_out (None: the loop is off).  frames: the device images instead of fx.dev(kind).
    -> lists (T x S x max_pts x 2), counts, dropped (T x S; unattached steps stay 0 / -7), records (T x S byte strings)"""
    torch, pkg = fx.torch, fx.pkg
    S = len(scheds)
    dL, dR = frames if frames is not None else fx.dev(kind)
    pitch = PITCH if kind == "gray" else BPITCH
    tb, tn = _boxes(torch, scheds, T)
    rec = pkg.TRACK_DTYPE.itemsize
    res = torch.zeros((T, S, rec), dtype=torch.uint8, device="cuda")
    lists = torch.zeros((T, S, max_pts, 2), dtype=torch.float32, device="cuda")
    counts = torch.zeros((T, S), dtype=torch.int32, device="cuda"); dropped = torch.full((T, S), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    entry = ctx.track_multi_step_dev if kind == "gray" else ctx.track_multi_step_bgr_dev
    for t in range(T):
        if attach is not None and attach[t]:
            ctx.track_dynamic_out(lists[t].data_ptr(), counts[t].data_ptr(), dropped[t].data_ptr() if with_dropped else None)
        bx = pkg.boxes_dev(tb[t].data_ptr(), tn[t].data_ptr(), BSTRIDE) if with_boxes else None
        entry(dL.data_ptr() + t * H * pitch, dR.data_ptr() + t * H * pitch, pitch, S, res[t].data_ptr(), boxes=bx)
    ctx.sync()
    torch.cuda.synchronize()
    r = res.cpu().numpy()
    return lists.cpu().numpy(), counts.cpu().numpy(), dropped.cpu().numpy(), [[r[t, q].tobytes() for q in range(S)] for t in range(T)]


def check(got, refs, steps=None, dropped=True):
    """sequence q of `got` against refs[q] (a single()'s result, or dyn_ref.loop's three arrays) over `steps`"""
    gl, gc, gd = got[:3]
    T = gl.shape[0]
    for q, want in enumerate(refs):
        if want is None:
            continue
        wl, wc, wd = want[:3]
        for t in (range(T) if steps is None else steps):
            assert gc[t, q] == wc[t], (q, t, gc[t, q], wc[t])
            assert not dropped or gd[t, q] == wd[t], (q, t, gd[t, q], wd[t])
            assert np.array_equal(gl[t, q, :wc[t]].view(np.uint32), wl[t, :wc[t]].view(np.uint32)), (q, t)


def same_runs(a, b):
    """two multi() results: counts, dropped and records exactly, lists over the used entries"""
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
    T, S = a[1].shape
    for t in range(T):
        for q in range(S):
            assert np.array_equal(a[0][t, q, :a[1][t, q]].view(np.uint32), b[0][t, q, :a[1][t, q]].view(np.uint32)), (t, q)


def check_records(got, refs):
    for q, want in enumerate(refs):
        for t in range(len(got[3])):
            assert got[3][t][q] == want[3][t], (q, t)


def new_multi(fx, S, p, max_batch=None, pipeline=0):
    ctx = fx.pkg.Svo(W, H, max_batch=max_batch or S)
    if pipeline:
        ctx.set_option("multi_pipeline", 1)
    if p is not None:
        ctx.track_dynamic(p)
    ctx.track_multi_reset(S, fx.cam)
    return ctx


@pytest.mark.gpu
def test_mixed_lengths_and_pipelining(pkg, fx):
    """S = 3, 4 steps, max_pts 100: a sequence whose first frame's seeds overflow the list, one without boxes at every step (counts
    and dropped stay 0 beside full lists), one with a small box.  The same steps with "multi_pipeline" = 1: identical lists and
    records.  Records are those of the loop switched off."""
    scheds, T, S = [boxes_for, sched_none, sched_small], 4, 3
    refs = [single(fx, q, T, scheds[q], max_pts=100) for q in range(S)]
    direct = fx.ref(max_pts=100)                         # sequence 0: dyn_ref.loop over svo_lk_track
    assert direct[1][0] == 100 and direct[2][0] == 140   # (frame 0's seeds overflow 100)
    assert refs[0][2][0] != 0 and not refs[1][1].any() and not refs[1][2].any()
    assert any(len({int(refs[q][1][t]) for q in range(S)}) > 1 for t in range(T)), "two sequences must differ in length at one step"
    assert any(0 < refs[2][1][t] and refs[2][1][t] != refs[0][1][t] for t in range(T)), "the small box must give a length of its own"
    ctx = new_multi(fx, S, params(pkg, max_pts=100))
    got = multi(fx, ctx, scheds, T, max_pts=100, attach=[True] * T)
    check(got, refs)
    check(got, [direct])
    check_records(got, refs)
    ctx.set_option("multi_pipeline", 1)
    ctx.track_multi_reset(S, fx.cam)
    piped = multi(fx, ctx, scheds, T, max_pts=100, attach=[True] * T)
    ctx.close()
    same_runs(piped, got)
    check(piped, refs)
    off = new_multi(fx, S, None)
    plain = multi(fx, off, scheds, T, max_pts=100)
    off.close()
    assert plain[3] == got[3], "the loop must not change a record"
    assert not plain[1].any()


@pytest.mark.gpu
@pytest.mark.parametrize("seed_frames", [-1, 0, 2])
def test_halves_reused_and_late_seeds(pkg, fx, seed_frames):
    """5 steps (each arena half and each list half is written at least twice) of a sequence whose first boxes arrive at step 2 -
    create-seeds only - beside one with the usual schedule, seeding at every frame, never, and for ids < 2."""
    scheds, T, S = [sched_late, boxes_for], 5, 2
    refs = [single(fx, q, T, scheds[q], seed_frames=seed_frames) for q in range(S)]
    direct = fx.ref(seed_frames=seed_frames, boxes_of=sched_late, tag="late")
    if seed_frames == -1:
        assert not direct[1][:2].any() and direct[1][2] > 0 and refs[1][1][T - 1] > 0
    if seed_frames == 0:
        assert not refs[0][1].any() and not refs[1][1].any()
    if seed_frames == 2:
        assert not refs[0][1].any() and refs[1][1][T - 1] > 0
    ctx = new_multi(fx, S, params(pkg, seed_frames=seed_frames))
    got = multi(fx, ctx, scheds, T, attach=[True] * T)
    ctx.close()
    check(got, refs)
    check(got, [direct])
    check_records(got, refs)


@pytest.mark.gpu
def test_output_attachment(pkg, fx):
    """A step without svo_track_dynamic_out in the middle still advances every chain; dropped = NULL is accepted; a run without
    boxes leaves every list empty."""
    scheds, T, S = [boxes_for, sched_small], 4, 2
    refs = [single(fx, q, T, scheds[q], seed_frames=-1) for q in range(S)]
    assert refs[0][1][T - 1] > 0
    ctx = new_multi(fx, S, params(pkg, seed_frames=-1))
    got = multi(fx, ctx, scheds, T, attach=[True, False, True, True])
    check(got, refs, steps=(0, 2, 3))
    assert not got[1][1].any() and not got[0][1].any() and (got[2][1] == -7).all()
    ctx.track_multi_reset(S, fx.cam)
    got = multi(fx, ctx, scheds, T, attach=[True] * T, with_dropped=False)
    check(got, refs, dropped=False)
    assert (got[2] == -7).all()
    ctx.track_multi_reset(S, fx.cam)
    got = multi(fx, ctx, scheds, T, attach=[True] * T, with_boxes=False)
    ctx.close()
    assert not got[1].any() and not got[2].any()


@pytest.mark.gpu
def test_one_sequence_and_a_changed_sequence_count(pkg, fx):
    """svo_track_multi_reset(1) runs the loop like the single-sequence entry; a second svo_track_multi_reset that takes S from 3
    to 2 starts with empty lists and gives the right ones."""
    T = 4
    ref0 = single(fx, 0, T, boxes_for)
    ctx = new_multi(fx, 1, params(pkg), max_batch=3)
    got = multi(fx, ctx, [boxes_for], T, attach=[True] * T)
    check(got, [ref0])
    check(got, [fx.ref()])
    check_records(got, [ref0])
    scheds = [boxes_for, sched_small, sched_late]
    ctx.track_multi_reset(3, fx.cam)
    got = multi(fx, ctx, scheds, T, attach=[True] * T)
    check(got, [single(fx, q, T, scheds[q]) for q in range(3)])
    ctx.track_multi_reset(2, fx.cam)
    got = multi(fx, ctx, scheds[:2], T, attach=[True] * T)
    ctx.close()
    check(got, [single(fx, q, T, scheds[q]) for q in range(2)])
    assert got[1][0, 1] == single(fx, 1, T, sched_small)[1][0]


def _made_gray(fx):
    """bgr_to_gray of the colour frames, in HBM like fx.dev("gray")"""
    if "made" not in fx._dev:
        torch = fx.torch
        gL = np.stack([fx.fe.bgr_to_gray(c) for c in fx.cL]); gR = np.stack([fx.fe.bgr_to_gray(c) for c in fx.cR])
        dL = torch.zeros((N, H, PITCH), dtype=torch.uint8, device="cuda"); dR = torch.zeros_like(dL)
        dL[:, :, :W] = torch.from_numpy(gL).cuda(); dR[:, :, :W] = torch.from_numpy(gR).cuda()
        torch.cuda.synchronize()
        fx._dev["made"] = (dL, dR)
    return fx._dev["made"]


@pytest.mark.gpu
def test_colour_entry_without_the_loop(pkg, fx):
    """svo_track_multi_step_bgr_dev with the loop off: records byte-identical to svo_track_multi_step_dev on bgr_to_gray of the same
    frames and to S svo_track_batch_bgr_dev chains; gray and colour steps alternate within a run."""
    scheds, T, S = [boxes_for, sched_small, sched_none], 4, 3
    refs = [single(fx, q, T, scheds[q], kind="bgr", dyn=False) for q in range(S)]
    ctx = new_multi(fx, S, None)
    got = multi(fx, ctx, scheds, T, kind="bgr")
    check_records(got, refs)
    ctx.track_multi_reset(S, fx.cam)
    gray = multi(fx, ctx, scheds, T, kind="gray", frames=_made_gray(fx))
    assert gray[3] == got[3]
    # alternating: steps 0 and 2 colour, 1 and 3 gray (on the made gray)
    torch = fx.torch
    ctx.track_multi_reset(S, fx.cam)
    tb, tn = _boxes(torch, scheds, T)
    rec = pkg.TRACK_DTYPE.itemsize
    res = torch.zeros((T, S, rec), dtype=torch.uint8, device="cuda")
    cL, cR = fx.dev("bgr"); gL, gR = _made_gray(fx)
    for t in range(T):
        bx = pkg.boxes_dev(tb[t].data_ptr(), tn[t].data_ptr(), BSTRIDE)
        if t % 2 == 0:
            ctx.track_multi_step_bgr_dev(cL.data_ptr() + t * H * BPITCH, cR.data_ptr() + t * H * BPITCH, BPITCH, S, res[t].data_ptr(), boxes=bx)
        else:
            ctx.track_multi_step_dev(gL.data_ptr() + t * H * PITCH, gR.data_ptr() + t * H * PITCH, PITCH, S, res[t].data_ptr(), boxes=bx)
    ctx.sync()
    torch.cuda.synchronize()
    r = res.cpu().numpy()
    ctx.close()
    assert [[r[t, q].tobytes() for q in range(S)] for t in range(T)] == got[3]


@pytest.mark.gpu
@pytest.mark.parametrize("colour,pipeline", [(1, 0), (1, 1), (0, 0), (0, 1)])
def test_colour_entry_with_the_loop(pkg, fx, colour, pipeline):
    """colour = 1: LK on the BGR left frames, the single-sequence _bgr loop's lists (the tint makes them differ from gray LK);
    colour = 0 through the colour entry: the gray loop on the gray the entry made - also pipelined, where the next step's
    conversion must wait for the loop's copy of that gray."""
    scheds, T, S = [boxes_for, sched_small], 4, 2
    refs = [single(fx, q, T, scheds[q], kind="bgr", colour=colour) for q in range(S)]
    direct = fx.ref(kind="bgr", colour=colour)
    assert direct[1][T - 1] > 0
    if colour:
        assert not np.array_equal(direct[0], fx.ref(kind="bgr", colour=0)[0])
    ctx = new_multi(fx, S, params(pkg, colour=colour), pipeline=pipeline)
    got = multi(fx, ctx, scheds, T, kind="bgr", attach=[True] * T)
    check(got, refs)
    check(got, [direct])
    check_records(got, refs)
    if not colour:   # ... and equal to the gray entry on the made gray; the two kinds of step may alternate
        ctx.track_multi_reset(S, fx.cam)
        gray = multi(fx, ctx, scheds, T, kind="gray", frames=_made_gray(fx), attach=[True] * T)
        same_runs(gray, got)
    ctx.close()


@pytest.mark.gpu
def test_argument_checks(pkg, fx):
    lib = pkg.load_library()
    torch = fx.torch
    dL, dR = fx.dev("gray")
    cL, cR = fx.dev("bgr")
    rec = pkg.TRACK_DTYPE.itemsize
    res = torch.zeros((N, rec), dtype=torch.uint8, device="cuda")
    lists = torch.zeros((4, 512, 2), dtype=torch.float32, device="cuda"); counts = torch.zeros(4, dtype=torch.int32, device="cuda")
    vp = lambda t: C.c_void_p(t.data_ptr())
    # the loop adopted by svo_track_multi_reset: the single-sequence entries refuse, by name, and the context goes on
    ctx = new_multi(fx, 1, params(pkg), max_batch=4)
    with pytest.raises(pkg.SvoError, match="svo_track_batch_dev"):
        ctx.track_batch_dev(dL.data_ptr(), dR.data_ptr(), PITCH, 2, res.data_ptr())
    with pytest.raises(pkg.SvoError, match="svo_track_frame"):
        ctx.track_frame(fx.L[0], fx.R[0])
    with pytest.raises(pkg.SvoError, match="svo_track_batch_bgr_dev"):
        ctx.track_batch_bgr_dev(cL.data_ptr(), cR.data_ptr(), BPITCH, 2, res.data_ptr())
    with pytest.raises(pkg.SvoError, match="svo_track_tail_dev"):
        ctx.track_tail_dev(res.data_ptr(), res.data_ptr(), res.data_ptr(), res.data_ptr(), 500, 1, res.data_ptr())
    with pytest.raises(pkg.SvoError, match="svo_track_sharded_dev"):
        pkg.Svo.track_sharded_dev([ctx], [dL.data_ptr()], [dR.data_ptr()], PITCH, 2, res.data_ptr())
    got = multi(fx, ctx, [boxes_for], 4, attach=[True] * 4)
    check(got, [single(fx, 0, 4, boxes_for)])
    # bad stride or sequence count, both entries
    call = lambda f, a, b, stride, n: f(ctx.h, vp(a), vp(b), stride, n, None, vp(res))
    assert call(lib.svo_track_multi_step_dev, dL, dR, W - 1, 1) == -1
    assert call(lib.svo_track_multi_step_dev, dL, dR, PITCH, 2) == -1
    assert call(lib.svo_track_multi_step_dev, dL, dR, PITCH, 0) == -1
    assert call(lib.svo_track_multi_step_bgr_dev, cL, cR, 3 * W - 1, 1) == -1
    assert call(lib.svo_track_multi_step_bgr_dev, cL, cR, BPITCH, 2) == -1
    assert lib.svo_track_multi_step_bgr_dev(ctx.h, None, vp(cR), BPITCH, 1, None, vp(res)) == -1
    # dense depth sources stay out of the many-sequence mode
    ctx.set_option("depth_source", 3)
    with pytest.raises(pkg.SvoError, match="depth_source"):
        ctx.track_multi_step_dev(dL.data_ptr(), dR.data_ptr(), PITCH, 1, res.data_ptr())
    with pytest.raises(pkg.SvoError, match="depth_source"):
        ctx.track_multi_step_bgr_dev(cL.data_ptr(), cR.data_ptr(), BPITCH, 1, res.data_ptr())
    ctx.set_option("depth_source", 0)
    # colour = 1 through the gray many-sequence entry: refused at that call; the colour entry runs
    ctx.track_dynamic(params(pkg, colour=1))
    ctx.track_multi_reset(2, fx.cam)
    with pytest.raises(pkg.SvoError, match="colour"):
        ctx.track_multi_step_dev(dL.data_ptr(), dR.data_ptr(), PITCH, 2, res.data_ptr())
    ctx.track_multi_step_bgr_dev(cL.data_ptr(), cR.data_ptr(), BPITCH, 2, res.data_ptr())
    ctx.sync()
    # the loop adopted by svo_track_reset: the many-sequence entries refuse, both of them
    ctx.track_dynamic(params(pkg))
    ctx.track_reset(fx.cam)
    with pytest.raises(pkg.SvoError, match="svo_track_multi_step_bgr_dev"):
        ctx.track_multi_step_bgr_dev(cL.data_ptr(), cR.data_ptr(), BPITCH, 1, res.data_ptr())
    # switched off, then svo_track_multi_reset: no attachment possible, plain records
    ctx.track_dynamic(params(pkg, enable=0))
    ctx.track_multi_reset(2, fx.cam)
    assert lib.svo_track_dynamic_out(ctx.h, vp(lists), vp(counts), None) == -1
    assert b"not enabled" in lib.svo_last_error(ctx.h)
    scheds = [boxes_for, sched_small]
    got = multi(fx, ctx, scheds, 4)
    ctx.close()
    check_records(got, [single(fx, q, 4, scheds[q], dyn=False) for q in range(2)])
