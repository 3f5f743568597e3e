"""CPU checks of the semantic gate's test material: the plain references of gate_ref.py against the C oracle, the committed
high-precision 8-point fixture against the oracle (where the per-case tolerances of the device tests are measured), and
the case generators against the properties their cases are named for.  No test here needs a GPU."""
import inspect
import os

import numpy as np
import pytest

import gate_cases
import gate_ref
import util

FM = np.load(os.path.join(util.GOLDEN, "fmat_cases.npz"))
NAMES = [str(n) for n in FM["names"]]
TAGS = dict(zip(NAMES, (str(t) for t in FM["tags"])))
EPS = 2.0 ** -52
NS = [8, 9, 63, 64, 65, 127, 128, 129, 448, 511, 512]


# ---- references against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", gate_cases.BF_SHAPES)
def test_bf_ref_equals_oracle(orc, M, N):
    q, t = gate_cases.bf_shape_case(M, N)
    for a, r in zip(gate_ref.bf_match_ref(q, t), orc.bf_match(q, t)):
        assert np.array_equal(a, r)


def test_bf_ref_equals_oracle_on_ties_and_minima(orc):
    for q, t in gate_cases.bf_tie_case():
        for a, r in zip(gate_ref.bf_match_ref(q, t), orc.bf_match(q, t)):
            assert np.array_equal(a, r)
    for gmin in (0, 16):
        q, t, thr = gate_cases.bf_minimum_case(gmin)
        for a, r in zip(gate_ref.bf_match_ref(q, t), orc.bf_match(q, t)):
            assert np.array_equal(a, r)


def test_bf_cases_have_their_properties():
    (q, t), (q2, t2) = gate_cases.bf_tie_case()
    ti, d, keep = gate_ref.bf_match_ref(q, t)
    assert list(ti) == [3] * 6 and list(d) == [0, 1, 7, 30, 31, 64]          # three-way tie: the lowest index
    assert list(keep) == [1, 1, 1, 1, 0, 0]
    ti, d, keep = gate_ref.bf_match_ref(q2, t2)
    assert list(ti) == [67] * 6                                               # two-way tie over a trip and a lane
    for gmin in (0, 16):
        q, t, thr = gate_cases.bf_minimum_case(gmin)
        ti, d, keep = gate_ref.bf_match_ref(q, t)
        assert list(ti[:3]) == [5, 9, 11] and list(d[:3]) == [gmin, thr, thr + 1] and d[3] > thr + 1
        assert list(keep) == [1, 1, 0, 0]
    ti, d, keep = gate_ref.bf_match_ref(*gate_cases.bf_shape_case(4, 0))
    assert list(ti) == [-1] * 4 and list(d) == [-1] * 4 and not keep.any()


@pytest.mark.parametrize("M,N", gate_cases.GATED_SHAPES)
def test_greedy_ref_without_boxes_equals_oracle(orc, M, N):
    c, _ = gate_cases.gated_case(M, N)
    got = gate_ref.greedy_gated_ref(c["q"], c["q_skip"], c["t"], c["assigned"], c["max_dist"], c["ratio"], c["q_xy"], c["t_xy"],
                                    None, c["F"])
    ref = orc.match_greedy(c["q"], c["t"], c["assigned"], c["max_dist"], c["ratio"], q_skip=c["q_skip"])
    for a, r in zip(got[:5], ref):
        assert np.array_equal(a, r)
    assert not got[5].any()
    c, _ = gate_cases.gated_case(64, 64, 30, 2.0)
    got = gate_ref.greedy_gated_ref(c["q"], c["q_skip"], c["t"], c["assigned"], 30, 2.0, c["q_xy"], c["t_xy"], None, c["F"])
    for a, r in zip(got[:5], orc.match_greedy(c["q"], c["t"], c["assigned"], 30, 2.0, q_skip=c["q_skip"])):
        assert np.array_equal(a, r)


def test_gate_helpers_equal_oracle(orc):
    """in_boxes_ref / epipolar_distance_ref against orc_point_in_boxes / orc_epipolar_distance on the edge points and on
    random pairs (bit for bit: both evaluate the written operation order in float64)."""
    import ctypes as C
    l = orc.lib()
    l.orc_point_in_boxes.argtypes = [C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_int]
    c, _, _ = gate_cases.box_edge_case()
    bx = np.ascontiguousarray(c["boxes"], np.int32)
    for x, y in c["t_xy"]:
        assert bool(l.orc_point_in_boxes(float(x), float(y), bx.ctypes.data, len(bx), 10)) == gate_ref.in_boxes_ref(x, y, bx)
    rng = np.random.default_rng(5)
    F = gate_cases.general_F()
    for _ in range(50):
        a = rng.uniform(0, 1241, 2).astype(np.float32); b = rng.uniform(0, 376, 2).astype(np.float32)
        assert orc.epipolar_distance(F, a, b) == gate_ref.epipolar_distance_ref(F, a, b)
    assert np.isnan(gate_ref.epipolar_distance_ref(np.zeros(9), (1, 2), (3, 4)))


# ---- generator checks: each gated case has the property it is named for, by the reference alone ----------------------------
@pytest.mark.parametrize("M,N", gate_cases.GATED_SHAPES)
def test_gated_cases_are_well_conditioned(M, N):
    c, ref = gate_cases.gated_case(M, N)
    assert gate_cases.well_conditioned(c, ref)
    bi, b, s, acc, asg, vet, info = ref
    assert len(c["release"]) >= 1
    for i, j in c["release"]:           # a vetoed row claims nothing: the next row takes the same column
        assert vet[i] and not acc[i] and acc[i + 1] and bi[i] == bi[i + 1] == j and asg[j]
    assert (c["boxes"][:, 0] - 10).min() < 0
    assert not (vet & acc).any() and not vet[c["q_skip"] != 0].any()
    # the gate bites: the ungated result differs
    free = gate_ref.greedy_gated_ref(c["q"], c["q_skip"], c["t"], c["assigned"], c["max_dist"], c["ratio"], c["q_xy"], c["t_xy"],
                                     None, c["F"])
    assert not np.array_equal(free[3], acc)


def test_special_gated_cases_have_their_properties():
    c, ref = gate_cases.gated_case(64, 64, 30, 2.0)
    assert gate_cases.well_conditioned(c, ref) and ref[3].sum() > 0
    c, ref = gate_cases.gated_case(65, 65, many_boxes=True)
    assert len(c["boxes"]) == 64 and gate_cases.well_conditioned(c, ref)
    # only the last three boxes hold any point
    assert not any(gate_ref.in_boxes_ref(x, y, c["boxes"][:61]) for x, y in c["t_xy"])
    c, ref, expect = gate_cases.threshold_case()
    ys = c["t_xy"][:, 1].astype(np.float64)
    assert ys[0] < ys[1] < 100.1 < ys[2] < ys[3] and np.nextafter(np.float32(ys[1]), np.float32(200)) == np.float32(ys[2])
    assert np.array_equal(expect, (np.abs(ys - 100.0) > 0.1).astype(np.uint8))       # |cy - 100| is exact in float64
    assert np.array_equal(ref[5], expect) and np.array_equal(ref[3], 1 - expect)
    c, ref, expect = gate_cases.box_edge_case()
    assert np.array_equal(ref[5], expect) and np.array_equal(ref[3], 1 - expect)
    assert expect.sum() == 8 and sum(1 for i, _, inb, _ in ref[6] if inb and ref[3][i]) == 2
    c, ref = gate_cases.zero_F_case()
    assert all(gate_ref.in_boxes_ref(x, y, c["boxes"]) for x, y in c["t_xy"])
    assert not ref[5].any() and all(np.isnan(d) for _, _, inb, d in ref[6]) and len(ref[6]) > 0
    free = gate_ref.greedy_gated_ref(c["q"], c["q_skip"], c["t"], c["assigned"], 15, 0.0, c["q_xy"], c["t_xy"], None, c["F"])
    for a, r in zip(ref[:5], free[:5]):
        assert np.array_equal(a, r)


def test_binding_has_the_gated_entry(pkg):
    """Svo.match_greedy_gated: match_greedy's arguments and results first, then the gate's."""
    a = list(inspect.signature(pkg.Svo.match_greedy).parameters)
    g = list(inspect.signature(pkg.Svo.match_greedy_gated).parameters)
    assert g[:6] == a[:6] and g[6:] == ["q_xy", "t_xy", "boxes", "F", "q_skip", "vetoed"]
    assert "svo_match_greedy_gated" in pkg.ABI_SYMBOLS


# ---- the committed high-precision 8-point fixture ----------------------------------------------------------------------------
def test_fmat_fixture_covers_the_case_list():
    tags = list(TAGS.values())
    assert len(NAMES) == len(set(NAMES)) and tags.count("ungapped") * 4 <= len(tags)
    ns = {len(FM[n + "/p1"]) for n in NAMES if n.startswith("general_")}
    assert ns == set(NS)
    for fam in ("forward", "sideways", "anytrans"):
        assert sum(1 for n in NAMES if n.startswith(fam) and TAGS[n] == "raw") >= 1
        assert sum(1 for n in NAMES if n.startswith(fam) and TAGS[n] == "norm") >= 1
    for fam in ("offset10000", "offset1e+06", "patch", "equal_diagonal", "pts2_identical", "pts1_identical", "one_pair_x8", "planar",
                "collinear"):
        assert any(n.startswith(fam) for n in NAMES), fam
    assert os.path.getsize(os.path.join(util.GOLDEN, "fmat_cases.npz")) < 512 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_fmat_case_has_its_property(name):
    p1, p2, F, lam, tag = FM[name + "/p1"], FM[name + "/p2"], FM[name + "/F"], FM[name + "/lam"], TAGS[name]
    f8 = float(FM[name + "/f8"][0])
    if tag == "zero":
        assert not F.any()
        assert (np.ptp(p1, axis=0) == 0).all() or (np.ptp(p2, axis=0) == 0).all()
        return
    gap = (lam[1] - lam[0]) / lam[2]
    assert abs(np.linalg.norm(F) - 1) < 1e-15 and F.reshape(9)[np.argmax(np.abs(F))] > 0
    if tag == "ungapped":
        assert gap < 1e-8
        return
    assert gap >= 1e-7                      # ten times clear of the 1e-8 below which entries are not compared
    if tag == "raw":                        # pure translation, noise-free: skew-symmetric F, the un-normalised branch
        assert abs(f8) < 1e-9 and gap >= 1e-6
        assert np.abs(F + F.T).max() < 1e-9
    else:
        assert abs(f8) > 1e-3               # far above the 1.19e-7 switch
        if name.split("_")[0] in ("forward", "sideways", "anytrans"):
            assert abs(F[2, 2]) > 1e-3      # |F[8]| / ||F||
    if name.startswith("offset"):
        assert p1.mean() >= float(name[6:].split("_")[0])
    if name.startswith("patch"):
        assert np.ptp(p1, axis=0).max() <= 2.0
    if name.startswith("equal_diagonal"):   # the padding eigenvalue (largest diagonal entry) ties with the real ones
        A, _, _ = gate_ref.design_matrix(p1, p2)
        d = np.diag(A.T @ A)
        assert (d.max() - d.min()) / d.max() < 1e-2
    # the stored reference solves the problem it was made for: a textbook SVD-based float64 implementation (LAPACK, no
    # normal matrix) lands within the first-order perturbation bound of it, and no unit vector beats lam1
    A, T1, T2 = gate_ref.design_matrix(p1, p2)
    U, S, Vt = np.linalg.svd(np.linalg.svd(A)[2][-1].reshape(3, 3))
    Fs = T2.T @ (U @ np.diag([S[0], S[1], 0]) @ Vt) @ T1
    assert gate_ref.entry_deviation(Fs, F) <= 64 * EPS / gap
    assert gate_ref.algebraic_residual(F, p1, p2) ** 2 >= lam[0] - 1e-12 * lam[2]
    assert abs(np.linalg.det(F)) < 1e-15


@pytest.mark.parametrize("name", NAMES)
def test_oracle_8point_against_the_fixture(orc, name):
    """Where the device's tolerances come from: the oracle's deviation from the 50-digit F, measured by the generator and
    re-measured here; the stored bounds are max(16 x it, 64 eps lam9 / (lam2 - lam1)).  The oracle's entries are held
    to the floor alone (a cyclic Jacobi is backward stable); its probe distances also carry the de-normalisation's
    cancellation (offsets of 1e6 px against a spread of 300), which is why that deviation is measured and not derived."""
    p1, p2, F, lam, tag = FM[name + "/p1"], FM[name + "/p2"], FM[name + "/F"], FM[name + "/lam"], TAGS[name]
    Fo = orc.fundamental_8point(p1, p2)
    if tag == "zero":
        assert not Fo.any()
        return
    assert np.isfinite(Fo).all() and Fo.any()
    if tag == "ungapped":
        # the eigenvector is any unit vector of a two- or three-dimensional null space: only the residual and the rank
        # are defined.  lam1 is zero to 50 digits, so the residual is rounding alone.
        assert gate_ref.algebraic_residual(Fo, p1, p2) <= np.sqrt(64 * EPS * lam[2])
        assert abs(np.linalg.det(Fo)) <= 1e-12 * np.linalg.norm(Fo) ** 3
        return
    gap = (lam[1] - lam[0]) / lam[2]
    spread = float(np.linalg.norm(p1 - p1.mean(0), axis=1).mean())
    dev = np.array([gate_ref.entry_deviation(Fo, F), gate_ref.probe_deviation(Fo, F, FM[name + "/last"], FM[name + "/cur"], spread)])
    floor = 64 * EPS / gap
    print(name, "oracle deviation", dev, "bound", FM[name + "/bound"], "floor", floor)
    assert np.array_equal(FM[name + "/bound"], np.maximum(16 * FM[name + "/dev"], floor))
    assert (dev <= FM[name + "/bound"]).all()        # (a rebuilt oracle may round differently: inside the bound, not equal)
    assert dev[0] <= floor
    if tag == "norm":
        assert Fo[2, 2] == 1.0
    else:
        assert abs(Fo[2, 2]) < 1.1920929e-07
    assert abs(np.linalg.det(Fo)) <= 1e-12 * np.linalg.norm(Fo) ** 3
