"""MSA dense stereo on the device (csrc/svo_msa.hip) against the numpy twin tests/msa_ref.py on the hand-made cases of
tests/msa_cases.py: volumes, masks, maps and aggregates bit for bit - no tolerance anywhere, the code promises bit parity - and every
case that names a path (k_msa_dp_bfs in one launch, with or without the LDS opt-in, or the launch-per-level kernels) asserts it
through the probe Svo.msa_plan() (svo_debug_msa_plan).  tests/test_msa_cpu.py shows, without a GPU, that the twin equals the C oracle
on the same cases, that every case reaches its edge, and that every neighbouring rule would be caught.  One context per module."""
import ctypes
import functools
import os

import numpy as np
import pytest

import msa_cases as Cs
import msa_ref as R

INIT_KEYS = ("costL", "costR", "m3L", "m3R", "r_graL", "c_graL", "r_graR", "c_graR")


@pytest.fixture(scope="module")
def svo(pkg):
    assert "SVO_MSA_LEVEL_LAUNCHES" not in os.environ       # every path below is the one the host code picks on its own
    s = pkg.Svo(640, 240)
    yield s
    s.close()


@functools.lru_cache(maxsize=None)
def tree_twin(name, o):
    c = Cs.tree_cases()[name]
    a = R.tree_dp(*c.args(), R.exp_table(o))
    a.setflags(write=False)
    return a


def run_tree_case(s, name):
    """the case on context s: the aggregate equals the twin's bytes, and the probe reports the path and the numbers the case predicts"""
    c = Cs.tree_cases()[name]
    for o in c.os:
        g = s.msa_tree_dp(*c.args(), o)
        plan = s.msa_plan()
        print(name, o, plan)
        assert g.tobytes() == tree_twin(name, o).tobytes(), (name, o, int((g != tree_twin(name, o)).sum()))
        assert (plan["bfs"], plan["maxw"], plan["levels"], plan["lds"]) == (c.expect_bfs, c.maxw, c.levels, c.lds), (name, plan)
        assert plan["lds"] == Cs.lds_bytes(plan["maxw"], plan["levels"])
        if c.expect_bfs:
            assert plan["lds_state"] == 1, (name, plan)      # asked for once per context, granted on this device
    return plan


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(Cs.tree_cases()))
def test_gpu_tree_case_equals_twin_on_the_path_it_names(svo, name):
    run_tree_case(svo, name)


@pytest.mark.gpu
def test_gpu_lds_budgets_are_crossed_where_the_cases_say(svo):
    """recomputed from lds() as the probe reports it: 64 KB between maxw 3,966 and 3,967 (both one launch, the second only by the
    opt-in), 150 KB between maxw 9,470 and 9,471 and between 1,886 and 1,887 levels (one launch | one per level)"""
    p = {n: run_tree_case(svo, n) for n in ("lds64k_maxw3966", "lds64k_maxw3967", "lds150k_maxw9470", "lds150k_maxw9471",
                                            "lds150k_levels1886", "lds150k_levels1887")}
    assert p["lds64k_maxw3966"]["lds"] <= 65536 < p["lds64k_maxw3967"]["lds"]
    assert p["lds64k_maxw3966"]["bfs"] == p["lds64k_maxw3967"]["bfs"] == 1 and p["lds64k_maxw3967"]["lds_state"] == 1
    for below, above in (("lds150k_maxw9470", "lds150k_maxw9471"), ("lds150k_levels1886", "lds150k_levels1887")):
        assert p[below]["lds"] <= 150 * 1024 < p[above]["lds"] and (p[below]["bfs"], p[above]["bfs"]) == (1, 0)


@pytest.mark.gpu
def test_gpu_fallback_and_fast_path_alternate_on_a_fresh_context(pkg):
    """Every fall-back case after a fast-path case and before one, on one context that starts with nothing planned and the opt-in
    not tried: a tree too wide for 150 KB decides before the opt-in is asked for and leaves it untried; the first tree that could
    run in one launch asks for it, once."""
    s = pkg.Svo(640, 240)
    try:
        first = s.msa_plan()
        assert (first["bfs"], first["lds_state"]) == (-1, 0)
        c = Cs.tree_cases()["lds150k_maxw9471"]
        assert s.msa_tree_dp(*c.args(), 0.1).tobytes() == tree_twin(c.name, 0.1).tobytes()
        assert (s.msa_plan()["bfs"], s.msa_plan()["lds_state"]) == (0, 0)
        assert run_tree_case(s, "lds64k_maxw3967")["lds_state"] == 1       # above 64 KB as the context's first one-launch aggregation
        fast = ["star_255ch", "lds150k_maxw9470", "n1", "stride_levels", "random3000_D255", "lds150k_levels1886", "path65"]
        slow = [n for n, c in Cs.tree_cases().items() if not c.expect_bfs]
        assert len(slow) == 7 and all(Cs.tree_cases()[n].expect_bfs for n in fast)
        for f, n in zip(fast, slow):
            run_tree_case(s, n)
            run_tree_case(s, f)
            run_tree_case(s, n)
    finally:
        s.close()


# ---- the per-pixel stages -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("W,H", Cs.INIT_SIZES)
def test_gpu_init_case_equals_twin(svo, W, H):
    for disp in Cs.INIT_DISPS:
        g = svo.msa_init(*Cs.init_pair(W, H), disp)
        t = Cs.init_twin(W, H, disp)
        for k in INIT_KEYS:
            assert g[k].dtype == t[k].dtype and g[k].tobytes() == t[k].tobytes(), (disp, k)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,disp,step", [(7, 40, 49, 3 * 7 + 1), (5, 5, 6, 64), (300, 2, 256, 1024)])
def test_gpu_init_with_a_row_step_larger_than_the_row(svo, W, H, disp, step):
    """rows `step` > 3 W bytes apart, the bytes between the rows filled with a value the images do not hold in that place"""
    L, Rr = Cs.init_pair(W, H)
    pad = lambda a: np.ascontiguousarray(np.concatenate([a.reshape(H, 3 * W), np.full((H, step - 3 * W), 0xEE, np.uint8)], 1))
    a, b = pad(L), pad(Rr)
    o = dict(costL=np.zeros((H, W, disp), np.float32), costR=np.zeros((H, W, disp), np.float32), m3L=np.zeros_like(L), m3R=np.zeros_like(L),
             r_graL=np.zeros((H, W)), c_graL=np.zeros((H, W)), r_graR=np.zeros((H, W)), c_graR=np.zeros((H, W)))
    p = lambda x: ctypes.c_void_p(x.ctypes.data)
    svo._chk(svo.lib.svo_msa_init(svo.h, p(a), p(b), W, H, step, disp, *[p(o[k]) for k in INIT_KEYS]))
    t = Cs.init_twin(W, H, disp)
    for k in INIT_KEYS:
        assert o[k].tobytes() == t[k].tobytes(), k


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", Cs.WTA_SIZES)
def test_gpu_wta_case_equals_twin(svo, W, H):
    A, _ = Cs.wta_volume(W, H)
    assert np.array_equal(svo.msa_wta(A, H, W), R.wta(A, H, W))


@pytest.mark.gpu
@pytest.mark.parametrize("W", [256, 257])
def test_gpu_lrcheck_case_equals_twin(svo, W):
    d1, d2, named = Cs.lr_maps(W)
    vol, mask = R.lrcheck(d1, d2, 256)
    gv, gm = svo.msa_lrcheck(d1, d2, 256)
    for why, ((i, j), m) in named.items():
        assert gm[i, j] == m, why
    assert np.array_equal(gm, mask) and gv.dtype == vol.dtype and gv.tobytes() == vol.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", Cs.CTMF_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gpu_ctmf_case_is_the_clamped_median(svo, shape):
    """images smaller than the window (the compiled reference asserts on them): the definition is the judge"""
    a = Cs.ctmf_image(shape)
    for r in (1, 2):
        assert np.array_equal(svo.ctmf(a, r), R.median_clamped(a, r)), r


# ---- whole solves ---------------------------------------------------------------------------------------------------------------------------
def run_solve_case(s, case):
    name, W, H, d, shift, scales, bfs = case
    L, Rr = Cs.solve_pair(W, H, shift)
    t = Cs.solved(name)
    for sc in scales:
        g = s.msa_solve(L, Rr, d, sc)
        plan = s.msa_plan()
        print(name, sc, plan)
        assert np.array_equal(g, R.output(t["disp0"], sc)), (name, sc, int((g != R.output(t["disp0"], sc)).sum()))
        widths = [Cs.level_widths(x[1], x[2], x[3], x[0]) for x in (t["treeL"], t["treeR"])]
        assert plan["bfs"] == bfs and plan["maxw"] == max(max(w) for w in widths) and plan["levels"] == max(len(w) for w in widths), (name, plan)


@pytest.mark.gpu
@pytest.mark.parametrize("case", Cs.SOLVE_CASES, ids=[c[0] for c in Cs.SOLVE_CASES])
def test_gpu_solve_case_equals_twin(svo, case):
    run_solve_case(svo, case)


@pytest.mark.gpu
def test_gpu_solves_alternate_between_the_paths_on_one_context(svo):
    """d = 254 (one launch per aggregation) and d = 255 (the gather tile no longer fits: one launch per level, reached by a caller
    without any variable) in both orders on one context: same arena, the trees' by-pixel arrays rebuilt from the records"""
    by = {c[0]: c for c in Cs.SOLVE_CASES}
    for name in ("48x32_d254", "48x32_d255", "48x32_d254", "5x5_d16", "48x32_d255", "33x21_d0", "48x32_d255", "48x32_d254"):
        run_solve_case(svo, by[name])


@pytest.mark.gpu
@pytest.mark.parametrize("d,bfs", [(255, 0), (0, 1), (255, 0)])
def test_gpu_batch_case_equals_twin(svo, d, bfs):
    """B = 3 gray pairs of 48 x 32 in rows 64 bytes apart, the 16 padding bytes of every row filled with 0xEE: a chunk of three on
    the natural fall-back (d = 255) and with D = 1 (d = 0).  That the padding, read as pixels, would change every frame's map at
    d = 255 is shown on the twin (msa_cases.prove_batch_padding, run by tests/test_msa_cpu.py)."""
    import torch
    W, H, pitch, B = 48, 32, Cs.BATCH_PITCH, 3
    dev = torch.device("cuda", 0)
    frames = Cs.batch_frames(B, W, H)
    host = np.full((2, B, H, pitch), Cs.BATCH_FILL, np.uint8)
    for b, (gl, gr) in enumerate(frames):
        host[0, b, :, :W], host[1, b, :, :W] = gl, gr
    dL, dR = torch.from_numpy(host[0]).to(dev), torch.from_numpy(host[1]).to(dev)
    out = torch.full((B, H, W), -1.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    svo.msa_batch_dev(dL.data_ptr(), dR.data_ptr(), pitch, W, H, B, out.data_ptr(), d)
    got = out.cpu().numpy()
    plan = svo.msa_plan()
    print(d, plan)
    for b, want in enumerate(Cs.batch_twin_maps(d, B)):
        assert np.array_equal(got[b], want), (b, int((got[b] != want).sum()))
    assert plan["bfs"] == bfs
