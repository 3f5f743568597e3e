"""ORB extraction on the device, stage by stage, on the hand-made cases of tests/orb_cases.py: pyramid levels
(svo_debug_pyramid_level), corner sets (svo_debug_fast_corners), keypoints and descriptors equal the oracle's and the numpy twin's
(tests/orb_ref.py) bit for bit - there is no tolerance anywhere in this file - and each twin stage fed the DEVICE's previous
stage equals the device's next one, which names the stage when something differs.  With the pyramid as one launch per level and
fused, through svo_orb_extract and svo_frontend_batch_dev, with k_fast's candidate list at 0, 7 and 2048 entries, and with images
of very different density alternating on one context and side by side in one batch.  tests/test_orb_cpu.py shows that every
case reaches the edge it was made for."""
import numpy as np
import pytest

import orb_cases
import orb_ref

pytestmark = pytest.mark.gpu

FUSED = (0, 1)


@pytest.fixture(scope="module")
def ctxs(pkg):
    """One context per (W, H, max_kp, max_batch), shared by the cases of this file."""
    made = {}

    def get(W, H, max_kp, max_batch=1):
        key = (W, H, max_kp, max_batch)
        if key not in made:
            made[key] = pkg.Svo(W, H, max_kp=max_kp, max_batch=max_batch)
        svo = made[key]
        svo.set_option("pyr_fused", 1)
        svo.set_option("fast_cand_cap", 2048)
        return svo
    yield get
    for svo in made.values():
        svo.close()


def ctx_of(ctxs, name, fused=1, cap=2048):
    c = orb_cases.CASES[name]
    svo = ctxs(c["W"], c["H"], c["max_kp"])
    svo.set_option("pyr_fused", fused)
    svo.set_option("fast_cand_cap", cap)
    return svo


def device_stages(svo, slot=0, level0=True):
    levels = [svo.debug_pyramid_level(slot, l) if (l or level0) else None for l in range(8)]
    corners = [orb_ref.sort_corners(svo.debug_fast_corners(slot, l)) for l in range(8)]
    return levels, corners


def assert_kp_equal(kp, desc, want_kp, want_desc, what=""):
    assert len(kp) == len(want_kp), (what, len(kp), len(want_kp))
    for f in want_kp.dtype.names:
        assert np.array_equal(kp[f].view(np.uint32), want_kp[f].view(np.uint32)), (what, "keypoint field", f)
    assert np.array_equal(desc, want_desc), (what, "descriptors")


def assert_equals_reference(name, levels, corners, kp, desc, what=""):
    r = orb_cases.reference(name)
    for l in range(8):
        if levels[l] is not None:
            assert np.array_equal(levels[l], r["levels"][l]), (what, "level", l)
        assert np.array_equal(corners[l], r["corners"][l]), (what, "corners of level", l)
    assert_kp_equal(kp, desc, r["kp"], r["desc"], what)


@pytest.mark.parametrize("fused", FUSED)
@pytest.mark.parametrize("name", orb_cases.NAMES)
def test_device_equals_twin_and_oracle(ctxs, orc, name, fused):
    svo = ctx_of(ctxs, name, fused)
    img = orb_cases.image(name)
    kp, desc = svo.orb_extract(img)
    levels, corners = device_stages(svo)
    assert_equals_reference(name, levels, corners, kp, desc)
    okp, odesc, opyr = orc.orb_extract(img, orb_cases.CASES[name]["max_kp"], want_pyramid=True)
    olev = orc.pyramid_levels(opyr, img.shape[1], img.shape[0])
    for l in range(8):
        assert np.array_equal(levels[l], olev[l]) and np.array_equal(corners[l], orc.fast_corners(olev[l])), ("oracle, level", l)
    assert_kp_equal(kp, desc, okp, odesc, "oracle")


@pytest.mark.parametrize("fused", FUSED)
@pytest.mark.parametrize("name", orb_cases.NAMES)
def test_each_twin_stage_from_the_devices_previous_stage(ctxs, name, fused):
    svo = ctx_of(ctxs, name, fused)
    img = orb_cases.image(name)
    kp, desc = svo.orb_extract(img)
    levels, corners = device_stages(svo)
    w, h, scale, quota = svo.geometry()
    assert np.array_equal(levels[0], img)
    at = 0
    for l in range(8):
        if l:
            assert np.array_equal(orb_ref.resize_fixed(levels[l - 1], int(w[l]), int(h[l])), levels[l]), ("pyramid -> level", l)
        assert np.array_equal(orb_ref.fast_corners(levels[l]), corners[l]), ("level -> corners", l)
        rows = orb_ref.select(levels[l], corners[l], int(quota[l]))
        k = kp[kp["octave"] == l]
        d = desc[kp["octave"] == l]
        assert len(k) == len(rows), ("corners -> selection, level", l, len(k), len(rows))
        assert np.array_equal(np.nonzero(kp["octave"] == l)[0], np.arange(at, at + len(rows)))       # octave ascending
        at += len(rows)
        if not rows:
            continue
        xs = np.array([r[0] for r in rows]); ys = np.array([r[1] for r in rows])
        f = np.float32
        assert np.array_equal(k["x"], xs.astype(f) * scale[l]) and np.array_equal(k["y"], ys.astype(f) * scale[l]), ("selection order", l)
        assert np.array_equal(k["response"].view(np.uint32), np.array([orb_ref.response(r[2]) for r in rows], f).view(np.uint32))
        assert np.array_equal(k["size"], np.full(len(rows), f(31.0) * scale[l], f)) and (k["class_id"] == -1).all()
        assert np.array_equal(orb_ref.angles(levels[l], xs, ys).view(np.uint32), k["angle"].view(np.uint32)), ("selection -> angle", l)
        assert np.array_equal(orb_ref.describe(orb_ref.blur(levels[l]), xs, ys, k["angle"]), d), ("angle -> descriptor", l)
    assert at == len(kp)


@pytest.mark.parametrize("cap", (0, 7, 2048))
@pytest.mark.parametrize("name", orb_cases.FAST_NAMES + ["regular_texture_1188", "blocky_kp512"])
def test_fast_candidate_list_and_overflow_scan(ctxs, name, cap):
    """k_fast with a candidate list of 0 and 7 entries (every tile with a corner takes the overflow scan) and the full 2048."""
    for fused in FUSED:
        svo = ctx_of(ctxs, name, fused, cap)
        kp, desc = svo.orb_extract(orb_cases.image(name))
        levels, corners = device_stages(svo)
        assert_equals_reference(name, levels, corners, kp, desc, "cap %d fused %d" % (cap, fused))


class Batch:
    """Images in HBM at a pitched stride and the output arrays of svo_frontend_batch_dev."""

    def __init__(self, pkg, svo, lefts, rights):
        import torch
        self.B = B = len(lefts)
        H, W = lefts[0].shape
        K = svo.max_kp
        self.pitch = pitch = (W + 63) // 64 * 64 + 64
        dev = torch.device("cuda", 0)
        self.dL = torch.full((B, H, pitch), 77, dtype=torch.uint8, device=dev)      # the padding is not zero
        self.dR = torch.full((B, H, pitch), 77, dtype=torch.uint8, device=dev)
        for i in range(B):
            self.dL[i, :, :W] = torch.from_numpy(np.array(lefts[i])).to(dev)
            self.dR[i, :, :W] = torch.from_numpy(np.array(rights[i])).to(dev)
        kp = torch.zeros((B, K, pkg.KP_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        desc = torch.zeros((B, K, 32), dtype=torch.uint8, device=dev)
        n = torch.zeros(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        cam = pkg.Camera(**pkg.KITTI_00_02)
        svo.frontend_batch_dev(self.dL.data_ptr(), self.dR.data_ptr(), pitch, B, cam, kp.data_ptr(), desc.data_ptr(), n.data_ptr())
        svo.sync()
        self.n = n.cpu().numpy()
        self.kp = kp.cpu().numpy().reshape(B, -1).view(pkg.KP_DTYPE).reshape(B, K)
        self.desc = desc.cpu().numpy()

    def result(self, i):
        return self.kp[i, :self.n[i]], self.desc[i, :self.n[i]]


@pytest.mark.parametrize("fused", FUSED)
@pytest.mark.parametrize("name", orb_cases.NAMES)
def test_batch_entry_equals_twin(pkg, ctxs, name, fused):
    """The whole chain through svo_frontend_batch_dev (images read in place from HBM at a pitched stride)."""
    svo = ctx_of(ctxs, name, fused)
    img = orb_cases.image(name)
    b = Batch(pkg, svo, [img], [np.full_like(img, 100)])
    kp, desc = b.result(0)
    levels, corners = device_stages(svo, 0, level0=False)
    assert_equals_reference(name, levels, corners, kp, desc)
    assert all(len(svo.debug_fast_corners(1, l)) == 0 for l in range(8))       # the flat right image


# ---- state: what one image leaves behind must not reach the next -------------------------------------------------------------------
STATE = [("identical_1024", "blocky_kp8"), ("regular_texture_1188", None), ("identical_1025", "cap1_plus_strong")]


def _state_images(orc, a, b):
    ca = orb_cases.CASES[a]
    A = orb_cases.image(a)
    if b is None:                                   # a textured image at this context's max_kp, the oracle as its reference
        import util
        Bimg = util.blocky_image(23, ca["W"], ca["H"])
        want_b = orc.orb_extract(Bimg, ca["max_kp"])
    else:
        assert (orb_cases.CASES[b]["W"], orb_cases.CASES[b]["H"], orb_cases.CASES[b]["max_kp"]) == (ca["W"], ca["H"], ca["max_kp"])
        Bimg = orb_cases.image(b)
        want_b = (orb_cases.reference(b)["kp"], orb_cases.reference(b)["desc"])
    ra = orb_cases.reference(a)
    return A, Bimg, (ra["kp"], ra["desc"]), want_b


@pytest.mark.parametrize("a,b", STATE)
def test_alternating_images_on_one_context(ctxs, orc, a, b):
    """Dense A, a flat image, dense B, A again on one context: each call returns its own image's result - the score histogram is
    handed back zeroed, the counters are reset, and a level that was full is empty when it has to be (and the other way round)."""
    A, Bimg, want_a, want_b = _state_images(orc, a, b)
    svo = ctx_of(ctxs, a)
    flat = np.full_like(A, 100)
    for img, want, what in ((A, want_a, "A"), (flat, None, "flat"), (Bimg, want_b, "B"), (A, want_a, "A again"), (Bimg, want_b, "B again")):
        kp, desc = svo.orb_extract(img)
        if want is None:
            assert len(kp) == 0 and all(len(svo.debug_fast_corners(0, l)) == 0 for l in range(8))
        else:
            assert_kp_equal(kp, desc, want[0], want[1], what)


@pytest.mark.parametrize("a,b", STATE)
def test_batched_slots_do_not_mix(pkg, ctxs, orc, a, b):
    """B = 3 at a pitched stride, left [A, flat, B], right [flat, A, B]: every slot gives its left image's own result, and the
    corner lists of the right images' slots are their images' too."""
    A, Bimg, want_a, want_b = _state_images(orc, a, b)
    c = orb_cases.CASES[a]
    svo = ctxs(c["W"], c["H"], c["max_kp"], 3)
    flat = np.full_like(A, 100)
    for rep in range(2):                                       # the second call starts from what the first left behind
        bt = Batch(pkg, svo, [A, flat, Bimg], [flat, A, Bimg])
        assert_kp_equal(*bt.result(0), want_a[0], want_a[1], "slot 0 = A")
        assert bt.n[1] == 0
        assert_kp_equal(*bt.result(2), want_b[0], want_b[1], "slot 2 = B")
        ra = orb_cases.reference(a)
        for l in range(8):
            assert np.array_equal(orb_ref.sort_corners(svo.debug_fast_corners(0, l)), ra["corners"][l])
            assert np.array_equal(orb_ref.sort_corners(svo.debug_fast_corners(4, l)), ra["corners"][l])      # right image of pair 1 = A
            assert len(svo.debug_fast_corners(1, l)) == 0 and len(svo.debug_fast_corners(3, l)) == 0
            assert np.array_equal(orb_ref.sort_corners(svo.debug_fast_corners(2, l)), orb_ref.sort_corners(svo.debug_fast_corners(5, l)))
