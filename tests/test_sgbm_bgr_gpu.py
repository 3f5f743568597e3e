"""GPU suite of the colour (cn = 3) semi-global block matcher (svo_sgbm_*_bgr): the device against the numpy restatement
tests/sgbm_bgr_ref.py, bit for bit, stage by stage through svo_sgbm_debug_volume and then the final maps (the cases are
tests/sgbm_bgr_cases.py's); strided rows; the batch entry across its chunk; replicated gray against the gray entry; one arena
for gray and colour calls in turn; the argument checks; "sgbm_colour" in the tracker's _bgr entries."""
import ctypes as C
import importlib

import numpy as np
import pytest

import sgbm_bgr_cases as cases
import sgbm_cases

STAGES = ("C", "S4", "S", "disp2", "disp1_lr")   # svo_sgbm_debug_volume's `which` 0 .. 4
CHUNK = 2                                        # colour pairs per chunk of the arena (include/svo.h: svo_sgbm_batch_bgr_dev)


@pytest.fixture(scope="module")
def svo(pkg):
    s = pkg.Svo(640, 240, max_batch=1)
    yield s
    s.close()


def _params(pkg, H, D, colour=True):
    p = (pkg.sgbm_default_params_bgr if colour else pkg.sgbm_default_params)(H)
    p.numDisparities = D
    return p


def _run(pkg, svo, L, R, D):
    maps = svo.sgbm_process_bgr(L, R, _params(pkg, L.shape[0], D))
    return [svo.sgbm_debug_volume(which) for which in range(len(STAGES))], maps


def _assert_stages(stages, maps, ref, name):
    D = ref["D"]
    for key, got in zip(STAGES, stages):
        bad = np.argwhere(got != ref[key])
        assert len(bad) == 0, "%s: stage %s differs at %d places, first (y, x[, d]) %s" % (name, key, len(bad), bad[:4].tolist())
    d16, d = maps
    assert np.array_equal(d16, ref["disp16"])
    assert d.dtype == np.float32 and np.array_equal(d.view(np.uint32), ref["disp"].view(np.uint32))
    assert np.all(d[d16 == -16] == -1.0) and np.all(d16[:, :D] == -16)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["minimal25x2d16", "shifted96x40d32", "noise120x24d48", "noise120x24d64", "portrait28x60d16"])
def test_every_stage_equals_the_restatement(pkg, svo, name):
    """The smallest legal image, real winners on which the channels disagree, both lane groups of 64, and H > W - D."""
    L, R, D, ref = cases.ref(name)
    stages, maps = _run(pkg, svo, L, R, D)
    _assert_stages(stages, maps, ref, name)
    if name == "minimal25x2d16":
        assert (stages[4] != -16).any() and np.all(maps[0] == -16)      # 18 pixels: all of them speckles
    else:
        assert (maps[0] != -16).mean() > 0.2


@pytest.mark.gpu
def test_wrapped_block_sums_and_carries_equal_the_restatement(pkg, svo):
    """The sawtooth pair: the true block sum passes 32 767 on a quarter of the volume (C negative there), carried steps leave
    int16 and the four-direction sums need more than 16 bits before they are saturated."""
    L, R, D, ref = cases.ref(cases.WRAP_CASE)
    cen = cases.census(ref)
    assert cen["block_sum_over"] > 0 and cen["carried_out"] > 0 and (ref["C"] < 0).any()
    stages, maps = _run(pkg, svo, L, R, D)
    _assert_stages(stages, maps, ref, cases.WRAP_CASE)
    assert (stages[0] < 0).sum() == cen["block_sum_over"]


def _process_strided(pkg, svo, L, R, D, stride, fill=0xA5):
    H, W = L.shape[:2]
    bufs = []
    for img in (L, R):
        b = np.full((H, stride), fill, np.uint8)
        b[:, :3 * W] = img.reshape(H, 3 * W)
        bufs.append(b)
    d16 = np.full((H, W), 77, np.int16); d = np.full((H, W), 77, np.float32)
    p = _params(pkg, H, D)
    rc = svo.lib.svo_sgbm_process_bgr(svo.h, bufs[0].ctypes.data_as(C.c_void_p), bufs[1].ctypes.data_as(C.c_void_p), stride, W, H,
                                      C.byref(p), d16.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p))
    assert rc == 0, svo.lib.svo_last_error(svo.h)
    stages = []
    for which in range(len(STAGES)):
        out = np.zeros((H, W, D) if which < 3 else (H, W), np.int16)
        assert svo.lib.svo_sgbm_debug_volume(svo.h, which, out.ctypes.data_as(C.c_void_p)) == 0
        stages.append(out)
    return stages, (d16, d)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["shifted96x40d32", "portrait28x60d16"])
def test_strided_rows_give_the_contiguous_calls_bytes(pkg, svo, name):
    """stride = 3 W + 5, the five bytes between the rows 0xA5: a kernel or a copy that read them would change the costs."""
    L, R, D, ref = cases.ref(name)
    want_stages, want_maps = _run(pkg, svo, L, R, D)
    svo.sgbm_process_bgr(R, L, _params(pkg, L.shape[0], D))       # something else in the arena in between
    stages, maps = _process_strided(pkg, svo, L, R, D, 3 * L.shape[1] + 5)
    for key, a, b in zip(STAGES, stages, want_stages):
        assert a.tobytes() == b.tobytes(), (name, key)
    assert maps[0].tobytes() == want_maps[0].tobytes() and maps[1].tobytes() == want_maps[1].tobytes()
    _assert_stages(stages, maps, ref, name)


def _batch(pkg, ctx, pairs, D, pitch, sentinel=7.0):
    """svo_sgbm_batch_bgr_dev on resident pairs whose rows are `pitch` bytes apart; the output is prefilled with `sentinel`."""
    import torch
    B = len(pairs)
    H, W = pairs[0][0].shape[:2]
    dev = torch.device("cuda", 0)
    dL = torch.full((B, H, pitch), 0xA5, dtype=torch.uint8, device=dev); dR = torch.full_like(dL, 0xA5)
    dL[:, :, :3 * W] = torch.from_numpy(np.stack([a.reshape(H, 3 * W) for a, _ in pairs])).to(dev)
    dR[:, :, :3 * W] = torch.from_numpy(np.stack([b.reshape(H, 3 * W) for _, b in pairs])).to(dev)
    out = torch.full((B, H, W), sentinel, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.sgbm_batch_bgr_dev(dL.data_ptr(), dR.data_ptr(), pitch, W, H, B, out.data_ptr(), _params(pkg, H, D))
    return out.cpu().numpy()


def _debug_rc(svo, which=0):
    sink = np.zeros(1 << 20, np.int16)
    return svo.lib.svo_sgbm_debug_volume(svo.h, which, sink.ctypes.data_as(C.c_void_p))


@pytest.mark.gpu
def test_batches_across_the_chunk_equal_single_calls(pkg, svo):
    """chunk + 1 and 2 chunk + 1 pairs (chunks of 2, 1 and of 2, 2, 1), rows 256 bytes apart, the output prefilled with 7.0."""
    W, H, D, pitch = 70, 18, 16, 256
    pairs = [cases.noise_pair(60 + b, W, H) for b in range(2 * CHUNK)] + [cases.wrap_pair(W, H)]
    single = [svo.sgbm_process_bgr(L, R, _params(pkg, H, D)) for L, R in pairs]
    assert len({s[0].tobytes() for s in single}) == len(pairs) and all((s[0] != -16).mean() > 0.2 for s in single)
    for B in (CHUNK + 1, 2 * CHUNK + 1):
        ctx = pkg.Svo(640, 240, max_batch=1)
        try:
            use = pairs[-B:]
            got = _batch(pkg, ctx, use, D, pitch)
        finally:
            ctx.close()
        for b, (d16, d) in enumerate(single[-B:]):
            assert np.array_equal(got[b].view(np.uint32), d.view(np.uint32)), (B, b)
            assert np.all(got[b][d16 == -16] == -1.0), (B, b)


@pytest.mark.gpu
def test_replicated_gray_gives_the_gray_entrys_map(pkg, svo):
    """svo_sgbm_process_bgr on (g, g, g) and svo_sgbm_process on g: the same disp16 (tests/test_sgbm_bgr_cpu.py has the
    precondition and the reason), and S is three times gray's."""
    gL, gR = cases.gray_pair()
    L, R, D, ref = cases.ref(cases.GRAY_CASE)
    g16, gd = svo.sgbm_process(gL, gR, _params(pkg, gL.shape[0], D, colour=False))
    gS = svo.sgbm_debug_volume(2)
    c16, cd = svo.sgbm_process_bgr(L, R, _params(pkg, L.shape[0], D))
    cS = svo.sgbm_debug_volume(2)
    assert np.array_equal(c16, g16) and cd.tobytes() == gd.tobytes()
    assert np.array_equal(cS.astype(np.int32), 3 * gS.astype(np.int32))
    assert np.array_equal(c16, ref["disp16"]) and (c16 != -16).mean() > 0.5


@pytest.mark.gpu
def test_one_arena_serves_gray_and_colour_calls_in_turn(pkg):
    """A gray call, a colour call of another size (larger in pixels, so the arena grows), the same gray call again: the gray
    bytes are unchanged and the colour call is right.  After a colour batch there is no volume to report."""
    ctx = pkg.Svo(640, 240, max_batch=1)
    try:
        gL, gR, gD, gref = sgbm_cases.ref("noise83x37")
        gp = _params(pkg, gL.shape[0], gD, colour=False)
        first = ctx.sgbm_process(gL, gR, gp)
        first_stages = [ctx.sgbm_debug_volume(w) for w in range(5)]
        assert np.array_equal(first[0], gref["disp16"])
        for name in ("shifted96x40d32", "minimal25x2d16"):
            L, R, D, ref = cases.ref(name)
            stages, maps = _run(pkg, ctx, L, R, D)
            _assert_stages(stages, maps, ref, name + " after a gray call")
        last = ctx.sgbm_process(gL, gR, gp)
        last_stages = [ctx.sgbm_debug_volume(w) for w in range(5)]
        assert first[0].tobytes() == last[0].tobytes() and first[1].tobytes() == last[1].tobytes()
        for a, b in zip(first_stages, last_stages):
            assert a.tobytes() == b.tobytes()
        assert _debug_rc(ctx) == 0
        L, R, D, ref = cases.ref("portrait28x60d16")
        got = _batch(pkg, ctx, [(L, R)] * 3, D, 3 * L.shape[1] + 1)
        assert all(np.array_equal(got[b].view(np.uint32), ref["disp"].view(np.uint32)) for b in range(3))
        assert all(_debug_rc(ctx, w) == -1 for w in range(5))          # SVO_E_INVALID: the batch entry leaves no volume to report
    finally:
        ctx.close()


@pytest.mark.gpu
def test_argument_checks(pkg, svo):
    L, R, D, _ = cases.ref("shifted96x40d32")
    H, W = L.shape[:2]
    gray = np.ascontiguousarray(L[:, :, 0]), np.ascontiguousarray(R[:, :, 0])
    with pytest.raises(pkg.SvoError, match="invalid"):
        svo.sgbm_process_bgr(L, R, _params(pkg, H, D, colour=False))          # gray's P1 / P2 into a colour entry
    with pytest.raises(pkg.SvoError, match="invalid"):
        svo.sgbm_process(gray[0], gray[1], _params(pkg, H, D))                # colour's into a gray entry
    for change in (dict(numDisparities=24), dict(blockSize=7), dict(P2=2592)):
        p = _params(pkg, H, D)
        for k, v in change.items():
            setattr(p, k, v)
        with pytest.raises(pkg.SvoError, match="invalid"):
            svo.sgbm_process_bgr(L, R, p)
    p = _params(pkg, H, D)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert svo.lib.svo_sgbm_process_bgr(svo.h, ptr(L), ptr(R), 3 * W - 1, W, H, C.byref(p), None, None) == -1     # stride < 3 W
    assert svo.lib.svo_sgbm_batch_bgr_dev(svo.h, ptr(L), ptr(R), 3 * W - 1, W, H, 1, C.byref(p), ptr(L)) == -1
    with pytest.raises(pkg.SvoError, match="invalid"):
        svo.sgbm_process_bgr(L[:, :D + 8], R[:, :D + 8], p)                   # W <= D + 8
    big = pkg.sgbm_default_params_bgr(100)
    rc = svo.lib.svo_sgbm_process_bgr(None, ptr(L), ptr(R), 3 * 3073, 3073, 100, C.byref(big), None, None)
    assert rc not in (0, -1) and rc == svo.lib.svo_sgbm_process(None, ptr(L), ptr(R), 3073, 3073, 100, C.byref(pkg.sgbm_default_params(100)), None, None)
    svo.set_option("sgbm_colour", 1)
    with pytest.raises(pkg.SvoError):
        svo.set_option("sgbm_colour", 2)
    svo.set_option("sgbm_colour", 0)


# ---- the tracker with depth_source = 3 and "sgbm_colour" ---------------------------------------------------------------------
N_TRACK = 4


def _colourise(g):
    """Three channels that are no copies of each other: B the complement about mid-gray at half the contrast, G the gray, R the
    gray with a ramp across the columns.  The complement sits in the channel that BGR2GRAY weighs least (0.114): the gray the
    entries make keeps -0.057 + 0.587 + 0.299 = 0.83 of the texture, so ORB still finds its corners (with the complement in G
    the three terms cancel to -0.03 and no keypoint is left)."""
    g = g.astype(np.int64)
    ramp = (np.arange(g.shape[1]) % 64)[None, :]
    return np.stack([128 + (128 - g) // 2, g, np.clip(g + ramp - 32, 0, 255)], -1).astype(np.uint8)


@pytest.mark.gpu
def test_tracker_bgr_entries_take_their_depth_from_the_colour_solver_when_asked(pkg):
    """svo_track_batch_bgr_dev on four synthetic colour frames with depth_source 3.  With sgbm_colour = 1 the depth of every
    keypoint of frame 0 is bf / disp at the truncated keypoint position of svo_sgbm_batch_bgr_dev's map of that pair (-bf
    where the map is invalid); with 0, of svo_sgbm_batch_dev's map of the gray the entry makes.  The two differ."""
    import torch
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    dev = torch.device("cuda", 0)
    gl, gr, _ = synth.render_sequence(N_TRACK, device=dev)
    gl, gr = gl.cpu().numpy(), gr.cpu().numpy()
    H, W = gl.shape[1:]
    bL = np.stack([_colourise(x) for x in gl]); bR = np.stack([_colourise(x) for x in gr])
    cam = pkg.Camera(**pkg.KITTI_00_02)
    tL, tR = torch.from_numpy(bL).to(dev), torch.from_numpy(bR).to(dev)
    ctx = pkg.Svo(W, H, max_batch=N_TRACK)
    try:
        # the two maps of pair 0
        cmap = torch.full((1, H, W), 7.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        ctx.sgbm_batch_bgr_dev(tL.data_ptr(), tR.data_ptr(), 3 * W, W, H, 1, cmap.data_ptr())
        g0 = torch.from_numpy(np.stack([ctx.bgr_to_gray(bL[0]), ctx.bgr_to_gray(bR[0])])).to(dev)
        gmap = torch.full((1, H, W), 7.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        ctx.sgbm_batch_dev(g0[0].data_ptr(), g0[1].data_ptr(), W, W, H, 1, gmap.data_ptr())
        maps = {1: cmap.cpu().numpy()[0], 0: gmap.cpu().numpy()[0]}
        assert (maps[1] != -1).mean() > 0.3 and (maps[0] != -1).mean() > 0.3 and not np.array_equal(maps[0], maps[1])
        ctx.set_option("depth_source", 3)
        depths, records = {}, {}
        out = torch.zeros(N_TRACK * pkg.TRACK_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        for colour in (1, 0):
            ctx.set_option("sgbm_colour", colour)
            ctx.track_reset(cam)
            out.zero_()
            torch.cuda.synchronize()
            ctx.track_batch_bgr_dev(tL.data_ptr(), tR.data_ptr(), 3 * W, N_TRACK, out.data_ptr())
            ctx.sync()
            records[colour] = out.cpu().numpy().view(pkg.TRACK_DTYPE).copy()
            kp, z = ctx.debug_track_depths(0)
            assert len(kp) == records[colour]["n_kp"][0] > 100
            disp = maps[colour][kp["y"].astype(np.int32), kp["x"].astype(np.int32)]
            with np.errstate(divide="ignore"):
                want = np.where(disp != 0, np.float32(cam.bf) / disp, np.float32(-1.0)).astype(np.float32)    # src/frame.cc:140-164
            assert np.array_equal(z.view(np.uint32), want.view(np.uint32)), colour
            assert np.all(z[disp == -1.0] == -np.float32(cam.bf)) and (disp == -1.0).any() and (disp > 0).sum() > 50
            depths[colour] = (kp.copy(), z.copy())
        assert depths[0][0].tobytes() == depths[1][0].tobytes()               # ORB sees the same gray either way
        assert (depths[0][1] != depths[1][1]).any()
        assert records[1]["n_kp"].tolist() == records[0]["n_kp"].tolist() and ctx.track_overflowed() == 0
        # the gray entry is not affected by the option
        gL_t, gR_t = torch.from_numpy(gl).to(dev), torch.from_numpy(gr).to(dev)
        rec = []
        for colour in (0, 1):
            ctx.set_option("sgbm_colour", colour)
            ctx.track_reset(cam)
            out.zero_()
            torch.cuda.synchronize()
            ctx.track_batch_dev(gL_t.data_ptr(), gR_t.data_ptr(), W, N_TRACK, out.data_ptr())
            ctx.sync()
            rec.append(out.cpu().numpy().tobytes())
        assert rec[0] == rec[1]
        # frame by frame and host-fed: the colour entries agree with the batched one
        ctx.set_option("sgbm_colour", 1)
        ctx.track_reset(cam)
        got = b"".join(ctx.track_frame_bgr(bL[k], bR[k]).tobytes() for k in range(N_TRACK))
        assert got == records[1].tobytes(), "svo_track_frame_bgr"
        ctx.track_reset(cam)
        res = np.zeros(N_TRACK, pkg.TRACK_DTYPE)
        ctx.track_batch_bgr_host(bL.ctypes.data, bR.ctypes.data, 3 * W, N_TRACK, res)
        ctx.sync()
        assert res.tobytes() == records[1].tobytes(), "svo_track_batch_bgr_host"
        ctx.track_multi_reset(2, cam)
        with pytest.raises(pkg.SvoError, match="depth_source must be 0"):
            ctx.track_multi_step_dev(gL_t.data_ptr(), gR_t.data_ptr(), W, 2, out.data_ptr())
    finally:
        ctx.close()
