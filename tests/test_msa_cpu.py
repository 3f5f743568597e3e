"""MSA dense stereo without a GPU: the numpy twin (tests/msa_ref.py, written from the reference's MSA.cpp as definitions) against the
C oracle (oracle/orc_msa.c, orc_msa_graph.cpp) bit for bit and stage by stage on every named case of tests/msa_cases.py - two
restatements by different routes; every case's `prove` (its edge is reached, asserted on the twin's data alone); the literal costR
chain against the closed form the product computes; the pins; and the mutant table: every switch of the twin flipped is told
apart from the reference's rule by a named case.  tests/test_msa_gpu.py holds the device to the same twin on the same cases."""
import json
import math
import os
import sys

import numpy as np
import pytest

import msa_cases as Cs
import msa_ref as R
from oracle import binding as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INIT_KEYS = ("costL", "costR", "m3L", "m3R", "r_graL", "c_graL", "r_graR", "c_graR")


@pytest.mark.parametrize("o", [0.1, 0.05, 0.2, 1.0])
def test_exp_table_is_the_oracles_bit_for_bit(o):
    """math.exp(-i * 1.0 / o / 255) in Python and exp() of the C library on the same expression: the same 256 doubles"""
    assert R.exp_table(o).tobytes() == ob.msa_exp_table(o).tobytes()
    assert R.exp_table(o)[0] == 1.0 and R.exp_table(o)[255] == math.exp(-1.0 / o)


# ---- trees ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Cs.tree_cases()))
def test_tree_case_reaches_its_edge_and_twin_equals_oracle(name):
    c = Cs.tree_cases()[name]
    c.prove()
    for o in c.os:
        a = R.tree_dp(*c.args(), R.exp_table(o))
        assert np.isfinite(a).all()
        assert a.tobytes() == ob.msa_tree_dp(*c.args(), ob.msa_exp_table(o)).tobytes(), (name, o)


def test_tree_cases_cover_both_sides_of_every_budget():
    cs = Cs.tree_cases().values()
    assert {c.max_children for c in cs} >= {254, 255, 256, 300}
    assert any(c.lds <= Cs.KB64 for c in cs if c.maxw == 3966) and any(Cs.KB64 < c.lds <= Cs.KB150 for c in cs if c.maxw == 3967)
    for below, above in (("lds150k_maxw9470", "lds150k_maxw9471"), ("lds150k_levels1886", "lds150k_levels1887")):
        a, b = Cs.tree_cases()[below], Cs.tree_cases()[above]
        assert a.lds <= Cs.KB150 < b.lds and (a.expect_bfs, b.expect_bfs) == (1, 0)
    assert Cs.lds_bytes(9000, 1886) == Cs.KB150                       # the last level table that fits, to the byte
    assert 2 * Cs.tree_cases()["lds150k_levels1887"].levels < 4000    # launches of the deepest fall-back
    assert Cs.gather_tile_bytes(255) == Cs.KB64 < Cs.gather_tile_bytes(256)
    w = Cs.tree_cases()["stride_levels"].widths
    assert {Cs.T_DP - 1, Cs.T_DP, Cs.T_DP + 1, 2 * Cs.T_DP + 1} <= set(w)


def test_zero_weight_edges_copy_the_parent():
    """c = 0: w = 1 and 1 - w * w = 0, so every node's aggregate is the root's"""
    c = Cs.tree_cases()["weights_all_0"]
    A, up = R.tree_dp(*c.args(), R.exp_table(0.1), keep_up=True)
    assert (A == A[c.root][None, :]).all() and (A[c.root] == up[c.root]).all()


# ---- MSA::init ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", Cs.INIT_SIZES)
@pytest.mark.parametrize("disp", Cs.INIT_DISPS)
def test_init_case_reaches_its_edges_and_twin_equals_oracle(W, H, disp):
    Cs.prove_init(W, H, disp)
    o = Cs.init_twin(W, H, disp)
    r = ob.msa_init(*Cs.init_pair(W, H), disp)
    for k in INIT_KEYS:
        assert o[k].dtype == r[k].dtype and o[k].tobytes() == r[k].tobytes(), k
    # the chain `pR[j][d] = pR[j][d - 1]`, literally, is the closed form costL[j + d'][d'], d' = min(d, m - 1 - j)
    assert np.array_equal(o["costR"], R.cost_right_closed_form(o["costL"]))


# ---- WTA, LRcheck, ctmf ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", Cs.WTA_SIZES)
def test_wta_case(W, H):
    Cs.prove_wta(W, H)
    A, _ = Cs.wta_volume(W, H)
    assert np.array_equal(R.wta(A, H, W), ob.msa_wta(A, H, W))


@pytest.mark.parametrize("W", [256, 257])
def test_lrcheck_case(W):
    Cs.prove_lr(W)
    d1, d2, _ = Cs.lr_maps(W)
    vol, mask = R.lrcheck(d1, d2, 256)
    rv, rm = ob.msa_lrcheck(d1, d2, 256)
    assert vol.dtype == rv.dtype and vol.tobytes() == rv.tobytes() and np.array_equal(mask, rm)


def median_by_loops(a, r):
    a3 = a.reshape(a.shape[0], a.shape[1], -1)
    H, W, cn = a3.shape
    out = np.zeros_like(a3)
    for i in range(H):
        for j in range(W):
            for c in range(cn):
                v = sorted(int(a3[min(max(i + di, 0), H - 1), min(max(j + dj, 0), W - 1), c]) for di in range(-r, r + 1) for dj in range(-r, r + 1))
                out[i, j, c] = v[len(v) // 2]
    return out.reshape(a.shape)


@pytest.mark.parametrize("shape", Cs.CTMF_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ctmf_case_is_the_clamped_median(shape):
    a = Cs.ctmf_image(shape)
    for r in (1, 2):
        assert np.array_equal(R.median_clamped(a, r), median_by_loops(a, r))
    if shape[:2] == (1, 1):
        assert np.array_equal(R.median_clamped(a, 2), a)


# ---- whole solves ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", Cs.SOLVE_CASES, ids=[c[0] for c in Cs.SOLVE_CASES])
def test_solve_case_twin_equals_oracle_stage_by_stage(case):
    name, W, H, d, shift, scales, bfs = case
    D = d + 1
    L, Rr = Cs.solve_pair(W, H, shift)
    s = Cs.solved(name)
    r = ob.msa_init(L, Rr, D)
    for k in INIT_KEYS:
        assert s[k].tobytes() == r[k].tobytes(), k
    for side, t in (("L", s["treeL"]), ("R", s["treeR"])):          # the product's trees are the literal restatement's
        rt = ob.msa_tree(r["m3" + side], r["r_gra" + side], r["c_gra" + side])
        assert t[0] == rt[0] and all(np.array_equal(x, y) for x, y in zip(t[1:], rt[1:]))
    E, E2 = ob.msa_exp_table(0.1), ob.msa_exp_table(0.05)
    dp = lambda cost, t, Ex: ob.msa_tree_dp(cost.reshape(-1, D), t[1], t[2], t[3], t[4], int(t[0]), Ex)
    assert s["A_R"].tobytes() == dp(r["costR"], s["treeR"], E).tobytes()
    assert s["A_L"].tobytes() == dp(r["costL"], s["treeL"], E).tobytes()
    assert np.array_equal(s["disp1"], ob.msa_wta(s["A_R"].reshape(H, W, D), H, W))
    assert np.array_equal(s["disp0_first"], ob.msa_wta(s["A_L"].reshape(H, W, D), H, W))
    rc, rm = ob.msa_lrcheck(s["disp0_first"], s["disp1"], D)
    assert s["cost_checked"].tobytes() == rc.tobytes() and np.array_equal(s["mask"], rm)
    assert s["A_refined"].tobytes() == dp(rc, s["treeL"], E2).tobytes()
    for sc in scales:
        assert np.array_equal(R.output(s["disp0"], sc), ob.msa_solve(L, Rr, d, sc)), sc
    # the edges the whole-solve cases are there for
    tl = s["treeL"]
    widths = Cs.level_widths(tl[1], tl[2], tl[3], tl[0])
    predicted = int(Cs.gather_tile_bytes(D) <= Cs.KB64 and Cs.lds_bytes(max(widths), len(widths)) <= Cs.KB150 and int(np.diff(tl[2]).max()) <= 255)
    assert predicted == bfs
    if name == "33x21_d0":
        assert not s["mask"].any() and not s["out"].any()
    if name == "5x5_d16":
        assert len(np.unique(s["disp0"])) == 1              # the r = 2 window is the whole image: one median everywhere
    if name == "shift40":
        assert (s["disp0"] == 40).mean() > 0.9
        assert [int(R.output(np.array([40], np.uint8), sc)[0]) for sc in scales] == [40, 120, 24]      # 280 wraps to 24


@pytest.mark.parametrize("d", [255, 0])
def test_batch_case_twin_equals_oracle(d):
    for (gl, gr), m in zip(Cs.batch_frames(), Cs.batch_twin_maps(d)):
        assert np.array_equal(m, ob.msa_solve(Cs.gray_to_bgr(gl), Cs.gray_to_bgr(gr), d, 1).astype(np.float32))
    maps = Cs.batch_twin_maps(d)
    assert all(not m.any() for m in maps) if d == 0 else all(m.any() for m in maps)
    if d:
        assert maps[0].tobytes() != maps[1].tobytes() != maps[2].tobytes()
        Cs.prove_batch_padding(d)       # the padding bytes, read as pixels, would show in every frame's map


# ---- the mutant table: each neighbour of a rule is told apart by a named case -------------------------------------------------------------------
def _tree(name, o=0.1):
    c = Cs.tree_cases()[name]
    return lambda r: R.tree_dp(*c.args(), R.exp_table(o), r).tobytes()


def _init(W, H, disp, keys=INIT_KEYS):
    return lambda r: b"".join(R.init(*Cs.init_pair(W, H), disp, r)[k].tobytes() for k in keys)


def _wta(W, H):
    return lambda r: R.wta(Cs.wta_volume(W, H)[0], H, W, r).tobytes()


def _lr(W):
    return lambda r: b"".join(x.tobytes() for x in R.lrcheck(*Cs.lr_maps(W)[:2], 256, r))


def _refined(name):
    def run(r):
        _, W, H, d, shift, _, _ = next(c for c in Cs.SOLVE_CASES if c[0] == name)
        s = Cs.solved(name)
        t = R.solve(*Cs.solve_pair(W, H, shift), d, 1, s["treeL"], s["treeR"], r)
        return t["A_refined"].tobytes() + t["out"].tobytes()
    return run


MUTANTS = [
    ("children added in reverse", dict(dp_children_reversed=True), _tree("star_300ch")),
    ("children added in reverse (255 children, the fast path's limit)", dict(dp_children_reversed=True), _tree("star_255ch")),
    ("w * up rounded to float before the add", dict(dp_round_product=True), _tree("star_255ch")),
    ("(1 - w) * (1 - w) for 1 - w * w", dict(dp_one_minus_w_sq=True), _tree("path63")),
    ("Exp with o not halved in the refinement", dict(refine_o_not_halved=True), _refined("40x5_d48")),
    ("last minimum in WTA", dict(wta_last=True), _wta(5, 5)),
    ("<= in WTA", dict(wta_le=True), _wta(300, 5)),
    ("dd >= 0 in LRcheck", dict(lr_dd_ge0=True), _lr(256)),
    ("j - dd > 0 in LRcheck", dict(lr_j_gt=True), _lr(257)),
    ("|d - d2| <= 1 in LRcheck", dict(lr_tol1=True), _lr(256)),
    ("occ = column 0 of the left image", dict(occ_left_col0=True), _init(7, 40, 6, ("costL",))),
    ("costR clamped to disparity 0 instead of the chain", dict(costR_clamp0=True), _init(5, 5, 49, ("costR",))),
    ("the colour cap at 8", dict(col_cap8=True), _init(7, 40, 1, ("costL",))),
    ("the gradient cap applied before abs", dict(gra_cap_before_abs=True), _init(7, 40, 6, ("costL",))),
    ("gray without + 0.5", dict(gray_no_half=True), _init(5, 5, 1)),
    ("the border gradient halved", dict(border_grad_halved=True), _init(2, 2, 1)),
    ("the median's rank off by one (r = 1, colour)", dict(median_rank_off=True), _init(5, 5, 1, ("m3L", "m3R"))),
    ("the median's rank off by one (r = 2, 3 x 3)", dict(median_rank_off=True), lambda r: R.median_clamped(Cs.ctmf_image((3, 3)), 2, r).tobytes()),
    ("scale saturating instead of wrapping", dict(scale_saturate=True), lambda r: R.output(Cs.solved("shift40")["disp0"], 7, r).tobytes()),
]


@pytest.mark.parametrize("name,kw,run", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_mutant_is_killed(name, kw, run):
    assert run(R.CONTRACT) != run(R.Rules(**kw)), name
    assert run(R.CONTRACT) == run(R.Rules()), "the case is not deterministic"


def test_every_switch_has_a_mutant():
    """no switch of the twin without a row above: none is dropped silently (none needed an equivalence argument)"""
    assert {k for m in MUTANTS for k in m[1]} == set(vars(R.Rules()))


def test_restatement_pins():
    """counts and digests of the twin's results on the named cases (tools/make_msa_pins.py wrote them)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_msa_pins
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "msa_restatement_pins.json")))
    got = make_msa_pins.pins()
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
