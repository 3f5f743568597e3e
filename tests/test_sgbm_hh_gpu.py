"""GPU suite of the semi-global block matcher's eight-direction mode (MODE_HH; svo_sgbm_*_mode with mode 1, "sgbm_mode" in
the tracker): the device against the numpy restatement tests/sgbm_hh_ref.py, bit for bit, stage by stage through
svo_sgbm_debug_volume and then the final maps, gray and colour (the cases are tests/sgbm_hh_cases.py's); mode 0 through the new
entries against the entries without a mode; batches across the chunks, with strided rows; the arena growing between modes;
colour after gray; the tracker's depths at depth_source 3."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import sgbm_bgr_cases
import sgbm_cases
import sgbm_hh_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGES = ("C", "S4", "S", "disp2", "disp1_lr")   # svo_sgbm_debug_volume's `which` 0 .. 4
HH = 1


@pytest.fixture(scope="module")
def svo(pkg):
    s = pkg.Svo(640, 240, max_batch=1)
    yield s
    s.close()


def _params(pkg, H, D, colour):
    p = (pkg.sgbm_default_params_bgr if colour else pkg.sgbm_default_params)(H)
    p.numDisparities = D
    return p


def _run(pkg, ctx, L, R, D, mode):
    colour = L.ndim == 3
    maps = (ctx.sgbm_process_bgr if colour else ctx.sgbm_process)(L, R, _params(pkg, L.shape[0], D, colour), mode=mode)
    return [ctx.sgbm_debug_volume(which) for which in range(len(STAGES))], maps


def _assert_stages(stages, maps, ref, name):
    D = ref["D"]
    for key, got in zip(STAGES, stages):
        bad = np.argwhere(got != ref[key])
        assert len(bad) == 0, "%s: stage %s differs at %d places, first (y, x[, d]) %s" % (name, key, len(bad), bad[:4].tolist())
    d16, d = maps
    assert np.array_equal(d16, ref["disp16"])
    assert d.dtype == np.float32 and np.array_equal(d.view(np.uint32), ref["disp"].view(np.uint32))
    assert np.all(d[d16 == -16] == -1.0) and np.all(d16[:, :D] == -16)


def _same_bytes(a, b):
    (sa, ma), (sb, mb) = a, b
    return all(x.tobytes() == y.tobytes() for x, y in zip(sa, sb)) and ma[0].tobytes() == mb[0].tobytes() and ma[1].tobytes() == mb[1].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name", cases.GRAY_CASES)
def test_gray_every_stage_equals_the_restatement(pkg, svo, name):
    L, R, D, ref = cases.ref(name)
    stages, maps = _run(pkg, svo, L, R, D, HH)
    _assert_stages(stages, maps, ref, name)
    old = sgbm_cases.ref(name)[3]
    assert np.array_equal(stages[1], old["S4"]) and (stages[2] != old["S"]).any()     # which = 1 is still S4; S is another volume


@pytest.mark.gpu
@pytest.mark.parametrize("name", cases.BGR_CASES)
def test_colour_every_stage_equals_the_restatement(pkg, svo, name):
    L, R, D, ref = cases.ref_bgr(name)
    stages, maps = _run(pkg, svo, L, R, D, HH)
    _assert_stages(stages, maps, ref, name)
    if name == cases.GRAY_REPLICATED_CASE:
        assert (stages[2] == -32768).sum() == 984         # sum8 saturated on the low side
    if name == cases.WRAP_CASE:
        assert (stages[2] == 32767).sum() >= 4834 and (stages[0] < 0).any()


def _raw_process(pkg, ctx, L, R, D, stride, mode, fill=0xA5):
    """The library's entries called directly on rows `stride` bytes apart (the bytes between the rows `fill`); mode None: the
    entry without a mode."""
    colour = L.ndim == 3
    H, W = L.shape[:2]
    row = W * (3 if colour else 1)
    bufs = []
    for img in (L, R):
        b = np.full((H, stride), fill, np.uint8)
        b[:, :row] = img.reshape(H, row)
        bufs.append(b)
    d16 = np.full((H, W), 77, np.int16); d = np.full((H, W), 77, np.float32)
    p = _params(pkg, H, D, colour)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    lib = ctx.lib
    if mode is None:
        rc = (lib.svo_sgbm_process_bgr if colour else lib.svo_sgbm_process)(ctx.h, ptr(bufs[0]), ptr(bufs[1]), stride, W, H, C.byref(p), ptr(d16), ptr(d))
    else:
        rc = (lib.svo_sgbm_process_bgr_mode if colour else lib.svo_sgbm_process_mode)(ctx.h, ptr(bufs[0]), ptr(bufs[1]), stride, W, H, C.byref(p),
                                                                                      int(mode), ptr(d16), ptr(d))
    assert rc == 0, lib.svo_last_error(ctx.h)
    stages = []
    for which in range(len(STAGES)):
        out = np.zeros((H, W, D) if which < 3 else (H, W), np.int16)
        assert lib.svo_sgbm_debug_volume(ctx.h, which, ptr(out)) == 0
        stages.append(out)
    return stages, (d16, d)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,name", [("gray", "noise83x37"), ("gray", "urban200x26"), ("bgr", "portrait28x60d16"), ("bgr", "wrap80x12d16")])
def test_mode_0_gives_the_bytes_of_the_entries_without_a_mode(pkg, svo, kind, name):
    """svo_sgbm_process[_bgr]_mode with SVO_SGBM_MODE_SGBM against svo_sgbm_process[_bgr], and both against the five-direction
    restatement, with an eight-direction call in between."""
    if kind == "gray":
        L, R, D, ref = sgbm_cases.ref(name)
        row = L.shape[1]
    else:
        L, R, D, ref = sgbm_bgr_cases.ref(name)
        row = 3 * L.shape[1]
    old = _raw_process(pkg, svo, L, R, D, row, None)
    _run(pkg, svo, L, R, D, HH)
    new = _raw_process(pkg, svo, L, R, D, row, 0)
    assert _same_bytes(old, new)
    _assert_stages(new[0], new[1], ref, name)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,name", [("gray", "portrait41x90d16"), ("bgr", "portrait28x60d16")])
def test_strided_rows_give_the_contiguous_calls_bytes(pkg, svo, kind, name):
    """Rows 5 bytes further apart than they are long, the bytes between them 0xA5."""
    L, R, D, ref = cases.ref(name) if kind == "gray" else cases.ref_bgr(name)
    row = L.shape[1] * (1 if kind == "gray" else 3)
    stages, maps = _raw_process(pkg, svo, L, R, D, row + 5, HH)
    _assert_stages(stages, maps, ref, name)


def _batch(pkg, ctx, pairs, D, pitch, mode, raw_old=False, sentinel=7.0):
    """svo_sgbm_batch[_bgr]_mode_dev on resident pairs whose rows are `pitch` bytes apart; the output is prefilled with
    `sentinel`.  raw_old: the entry without a mode."""
    import torch
    colour = pairs[0][0].ndim == 3
    B = len(pairs)
    H, W = pairs[0][0].shape[:2]
    row = W * (3 if colour else 1)
    dev = torch.device("cuda", 0)
    dL = torch.full((B, H, pitch), 0xA5, dtype=torch.uint8, device=dev); dR = torch.full_like(dL, 0xA5)
    dL[:, :, :row] = torch.from_numpy(np.stack([a.reshape(H, row) for a, _ in pairs])).to(dev)
    dR[:, :, :row] = torch.from_numpy(np.stack([b.reshape(H, row) for _, b in pairs])).to(dev)
    out = torch.full((B, H, W), sentinel, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    p = _params(pkg, H, D, colour)
    if raw_old:
        entry = ctx.lib.svo_sgbm_batch_bgr_dev if colour else ctx.lib.svo_sgbm_batch_dev
        rc = entry(ctx.h, C.c_void_p(dL.data_ptr()), C.c_void_p(dR.data_ptr()), pitch, W, H, B, C.byref(p), C.c_void_p(out.data_ptr()))
        assert rc == 0, ctx.lib.svo_last_error(ctx.h)
    else:
        (ctx.sgbm_batch_bgr_dev if colour else ctx.sgbm_batch_dev)(dL.data_ptr(), dR.data_ptr(), pitch, W, H, B, out.data_ptr(), p, mode=mode)
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,B", [("gray", 5), ("bgr", 3)])
def test_batches_across_the_chunk_equal_single_calls(pkg, svo, kind, B):
    """Five gray pairs are chunks of 4 and 1, three colour pairs chunks of 2 and 1; rows 256 bytes apart; a fresh context, so the
    batch entry itself is the first to ask for the mode's volumes.  The same pairs in mode 0 equal the entry without a mode."""
    W, H, D, pitch = 70, 18, 16, 256
    noise = sgbm_cases.noise_pair if kind == "gray" else sgbm_bgr_cases.noise_pair
    pairs = [noise(80 + b, W, H) for b in range(B)]
    single = [_run(pkg, svo, L, R, D, HH)[1] for L, R in pairs]
    assert len({s[0].tobytes() for s in single}) == B and all((s[0] != -16).mean() > 0.2 for s in single)
    ctx = pkg.Svo(640, 240, max_batch=1)
    try:
        got = _batch(pkg, ctx, pairs, D, pitch, HH)
        sink = np.zeros(W * H * D, np.int16)
        assert ctx.lib.svo_sgbm_debug_volume(ctx.h, 2, sink.ctypes.data_as(C.c_void_p)) == -1     # a batch leaves no volume to report
        five = _batch(pkg, ctx, pairs, D, pitch, 0)
        old = _batch(pkg, ctx, pairs, D, pitch, None, raw_old=True)
    finally:
        ctx.close()
    for b, (d16, d) in enumerate(single):
        assert np.array_equal(got[b].view(np.uint32), d.view(np.uint32)), b
        assert np.all(got[b][d16 == -16] == -1.0), b
    assert five.tobytes() == old.tobytes() and five.tobytes() != got.tobytes()


@pytest.mark.gpu
def test_modes_in_turn_on_one_context_while_the_arena_grows(pkg):
    """Mode 0, then 1 (the context's first: the arena gets its two further volumes; then a larger image: everything grows), then
    0 again: the third call's bytes are the first's."""
    ctx = pkg.Svo(640, 240, max_batch=1)
    try:
        L, R, D, ref0 = sgbm_cases.ref("noise83x37")
        first = _run(pkg, ctx, L, R, D, 0)
        _assert_stages(first[0], first[1], ref0, "mode 0 first")
        second = _run(pkg, ctx, L, R, D, HH)
        _assert_stages(second[0], second[1], cases.ref("noise83x37")[3], "mode 1 on the same size")
        Lb, Rb, Db, refb = cases.ref("urban200x26")
        assert Lb.size * Db > L.size * D
        big = _run(pkg, ctx, Lb, Rb, Db, HH)
        _assert_stages(big[0], big[1], refb, "mode 1 on a larger image")
        third = _run(pkg, ctx, L, R, D, 0)
        assert _same_bytes(first, third)
        again = _run(pkg, ctx, L, R, D, HH)
        assert _same_bytes(second, again)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_colour_after_gray_on_one_context_both_in_mode_1(pkg):
    ctx = pkg.Svo(640, 240, max_batch=1)
    try:
        L, R, D, ref = cases.ref("noise120x30d32")
        stages, maps = _run(pkg, ctx, L, R, D, HH)
        _assert_stages(stages, maps, ref, "gray")
        for name in ("noise120x24d48", "minimal25x2d16"):
            cL, cR, cD, cref = cases.ref_bgr(name)
            stages, maps = _run(pkg, ctx, cL, cR, cD, HH)
            _assert_stages(stages, maps, cref, name + " after a gray call")
        stages, maps = _run(pkg, ctx, L, R, D, HH)
        _assert_stages(stages, maps, ref, "gray again")
    finally:
        ctx.close()


@pytest.mark.gpu
def test_argument_checks_with_a_context(pkg, svo):
    L, R, D, _ = cases.ref("noise83x37")
    for mode in (2, -1, 3):
        with pytest.raises(pkg.SvoError, match="invalid"):
            svo.sgbm_process(L, R, _params(pkg, L.shape[0], D, False), mode=mode)
    svo.set_option("sgbm_mode", 1)
    for bad in (2, -1):
        with pytest.raises(pkg.SvoError):
            svo.set_option("sgbm_mode", bad)
    svo.set_option("sgbm_mode", 0)


# ---- the tracker with depth_source = 3 and "sgbm_mode" -----------------------------------------------------------------------
N_TRACK = 5            # one more than the gray chunk, and two colour chunks and a half


def _colourise(g):
    """tests/test_sgbm_bgr_gpu.py's recipe: three channels that are no copies of each other, whose gray keeps the texture."""
    g = g.astype(np.int64)
    ramp = (np.arange(g.shape[1]) % 64)[None, :]
    return np.stack([128 + (128 - g) // 2, g, np.clip(g + ramp - 32, 0, 255)], -1).astype(np.uint8)


@pytest.fixture(scope="module")
def sequence(pkg):
    import torch
    synth = importlib.import_module("stereo_semantic_vo_amd.synth")
    L, R, _ = synth.render_sequence(N_TRACK, device=torch.device("cuda", 0))
    return L.cpu().numpy(), R.cpu().numpy()


def _track(pkg, ctx, entry, tL, tR, pitch, cam):
    import torch
    out = torch.zeros(N_TRACK * pkg.TRACK_DTYPE.itemsize, dtype=torch.uint8, device=tL.device)
    ctx.track_reset(cam)
    torch.cuda.synchronize()
    entry(tL.data_ptr(), tR.data_ptr(), pitch, N_TRACK, out.data_ptr())
    ctx.sync()
    return out.cpu().numpy().view(pkg.TRACK_DTYPE).copy()


def _assert_depths_come_from(ctx, cam, maps, records):
    """svo_debug_track_depths of every frame of the last call: bf / disp at the truncated keypoint position of that frame's map
    (src/frame.cc:140-164; an invalid pixel is -1, so -bf)."""
    for k in range(N_TRACK):
        kp, z = ctx.debug_track_depths(k)
        assert len(kp) == records["n_kp"][k] > 100
        disp = maps[k][kp["y"].astype(np.int32), kp["x"].astype(np.int32)]
        with np.errstate(divide="ignore"):
            want = np.where(disp != 0, np.float32(cam.bf) / disp, np.float32(-1.0)).astype(np.float32)
        assert np.array_equal(z.view(np.uint32), want.view(np.uint32)), k
        assert np.all(z[disp == -1.0] == -np.float32(cam.bf)) and (disp > 0).sum() > 50


@pytest.mark.gpu
def test_tracker_takes_its_depths_from_the_maps_of_the_mode_asked_for(pkg, sequence):
    """svo_track_batch_dev at depth_source 3 with sgbm_mode 1: the depth of every keypoint of every frame is read off the map
    svo_sgbm_batch_mode_dev gives for that pair in mode 1, which is not the mode 0 map; with sgbm_mode 0 again the records are
    those of a context that never heard of the option."""
    import torch
    L, R = sequence
    H, W = L.shape[1:]
    dev = torch.device("cuda", 0)
    cam = pkg.Camera(**pkg.KITTI_00_02)
    tL, tR = torch.from_numpy(L).to(dev), torch.from_numpy(R).to(dev)
    plain = pkg.Svo(W, H, max_batch=N_TRACK)
    ctx = pkg.Svo(W, H, max_batch=N_TRACK)
    try:
        maps = {}
        for mode in (0, 1):
            m = torch.full((N_TRACK, H, W), 7.0, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            plain.sgbm_batch_dev(tL.data_ptr(), tR.data_ptr(), W, W, H, N_TRACK, m.data_ptr(), mode=mode)
            maps[mode] = m.cpu().numpy()
        assert all((maps[1][k] != maps[0][k]).any() and (maps[1][k] != -1).mean() > 0.3 for k in range(N_TRACK))
        plain.set_option("depth_source", 3)
        want0 = _track(pkg, plain, plain.track_batch_dev, tL, tR, W, cam)
        _assert_depths_come_from(plain, cam, maps[0], want0)
        ctx.set_option("depth_source", 3)
        ctx.set_option("sgbm_mode", 1)
        rec1 = _track(pkg, ctx, ctx.track_batch_dev, tL, tR, W, cam)
        _assert_depths_come_from(ctx, cam, maps[1], rec1)
        z0, z1 = plain.debug_track_depths(0)[1], ctx.debug_track_depths(0)[1]
        assert len(z0) == len(z1) and (z0 != z1).any()
        # frame by frame: the same records
        ctx.track_reset(cam)
        got = b"".join(ctx.track_frame(L[k], R[k]).tobytes() for k in range(N_TRACK))
        assert got == rec1.tobytes(), "svo_track_frame"
        ctx.set_option("sgbm_mode", 0)
        rec0 = _track(pkg, ctx, ctx.track_batch_dev, tL, tR, W, cam)
        assert rec0.tobytes() == want0.tobytes()
        # 0 -> 1 on a context that has tracked in mode 0: the arena gets its two further volumes in the middle of a batched call
        plain.set_option("sgbm_mode", 1)
        late = _track(pkg, plain, plain.track_batch_dev, tL, tR, W, cam)
        assert late.tobytes() == rec1.tobytes()
        _assert_depths_come_from(plain, cam, maps[1], late)
        assert ctx.track_overflowed() == 0
        ctx.set_option("sgbm_mode", 1)
        ctx.track_multi_reset(2, cam)
        out = torch.zeros(N_TRACK * pkg.TRACK_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        with pytest.raises(pkg.SvoError, match="depth_source must be 0"):
            ctx.track_multi_step_dev(tL.data_ptr(), tR.data_ptr(), W, 2, out.data_ptr())
    finally:
        plain.close(); ctx.close()


@pytest.mark.gpu
def test_tracker_bgr_entries_take_their_depths_from_the_colour_maps_of_the_mode(pkg, sequence):
    """svo_track_batch_bgr_dev at depth_source 3 with sgbm_colour 1 and sgbm_mode 1: depths off svo_sgbm_batch_bgr_mode_dev's
    mode 1 maps; with sgbm_colour 0, off the mode 1 maps of the gray the entry makes."""
    import torch
    gl, gr = sequence
    H, W = gl.shape[1:]
    dev = torch.device("cuda", 0)
    cam = pkg.Camera(**pkg.KITTI_00_02)
    bL = np.stack([_colourise(x) for x in gl]); bR = np.stack([_colourise(x) for x in gr])
    tL, tR = torch.from_numpy(bL).to(dev), torch.from_numpy(bR).to(dev)
    ctx = pkg.Svo(W, H, max_batch=N_TRACK)
    try:
        cmap = torch.full((N_TRACK, H, W), 7.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        ctx.sgbm_batch_bgr_dev(tL.data_ptr(), tR.data_ptr(), 3 * W, W, H, N_TRACK, cmap.data_ptr(), mode=1)
        gray = torch.from_numpy(np.stack([[ctx.bgr_to_gray(bL[k]), ctx.bgr_to_gray(bR[k])] for k in range(N_TRACK)])).to(dev)
        gL_t, gR_t = gray[:, 0].contiguous(), gray[:, 1].contiguous()
        gmap = torch.full((N_TRACK, H, W), 7.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        ctx.sgbm_batch_dev(gL_t.data_ptr(), gR_t.data_ptr(), W, W, H, N_TRACK, gmap.data_ptr(), mode=1)
        cmap, gmap = cmap.cpu().numpy(), gmap.cpu().numpy()
        assert (cmap != gmap).any()
        ctx.set_option("depth_source", 3)
        ctx.set_option("sgbm_mode", 1)
        for colour, maps in ((1, cmap), (0, gmap)):
            ctx.set_option("sgbm_colour", colour)
            rec = _track(pkg, ctx, ctx.track_batch_bgr_dev, tL, tR, 3 * W, cam)
            _assert_depths_come_from(ctx, cam, maps, rec)
        assert ctx.track_overflowed() == 0
    finally:
        ctx.close()


def _write_pnm(path, img):
    with open(path, "wb") as f:
        f.write(b"P%d\n%d %d\n255\n" % (5 if img.ndim == 2 else 6, img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img[:, :, ::-1] if img.ndim == 3 else img, np.uint8).tobytes())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["gray", "bgr"])
def test_host_classes_count_the_restatements_valid_pixels_with_hh(tmp_path, kind):
    """frame::SGBMMatch and frame::ElasMatchBgr with a mode (host/sgbm_check --hh [--bgr]): the eight-direction restatement's
    valid-pixel count and disparity sum, which are not the five-direction one's."""
    import sgbm_hh_ref
    exe = os.path.join(ROOT, "stereo-semantic-vo_amd", "host", "sgbm_check")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    if kind == "gray":
        L, R, _ = sgbm_cases.case("noise83x37")          # H = 37: ElasMatch's own numDisparities is 16
        want, other = cases.ref("noise83x37")[3], sgbm_cases.ref("noise83x37")[3]
        ext, flags = ".pgm", ["--hh"]
    else:
        L, R, _ = sgbm_bgr_cases.case("portrait28x60d16")
        want, other = cases.ref_bgr("portrait28x60d16")[3], sgbm_bgr_cases.ref("portrait28x60d16")[3]
        ext, flags = ".ppm", ["--hh", "--bgr"]
    assert sgbm_hh_ref.default_D(L.shape[0]) == want["D"] == 16
    _write_pnm(tmp_path / ("l" + ext), L); _write_pnm(tmp_path / ("r" + ext), R)
    r = subprocess.run([exe] + flags + [str(tmp_path / ("l" + ext)), str(tmp_path / ("r" + ext))], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    tok = r.stdout.split()
    valid = want["disp16"] != -16
    assert tok[0] == "sgbm_valid" and int(tok[1]) == int(valid.sum()) > 0 and int(tok[3]) == valid.size
    assert int(tok[5]) == int(want["disp16"][valid].astype(np.int64).sum())
    ovalid = other["disp16"] != -16
    assert (int(ovalid.sum()), int(other["disp16"][ovalid].astype(np.int64).sum())) != (int(tok[1]), int(tok[5]))
