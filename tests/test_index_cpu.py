"""The tracker's matching passes without a GPU: the plain restatement (index_ref.py) against the C oracle's tail on every
hand-made case (index_cases.py), each case's own property from the restatement and the list model alone, the round scheme
restated against the sequential scan, and the mutant table - every subtly wrong variant of the restatement must change what at
least one case expects, which is the proof that the cases can tell such a kernel from a right one."""
import numpy as np
import pytest

import index_cases
import index_ref

NAMES = index_cases.NAMES
SMALL = [n for n in NAMES if not n.startswith("rows_") and "300" not in n]
COUNTERS = ("n_match_pass1", "n_match_pass2", "n_new_mappoints", "n_local_map")


@pytest.fixture(scope="module")
def cam(pkg):
    return dict(pkg.KITTI_00_02)


def run_ref(case, veto_of=None, rounds=False, **rules):
    trk = index_ref.Tracker(rounds=rounds, **rules)
    out = []
    for f, (kp, desc, depth, boxes) in enumerate(case["frames"]):
        veto, nocreate = (veto_of or case["fiat"]).get(f, (None, None))
        out.append(trk.step(desc, depth, veto=veto, nocreate=nocreate))
    return out


def signature(results):
    return [(r["match_gid"].tolist(), r["new_gid"].tolist(), r["rows"].tolist()) + tuple(r[c] for c in COUNTERS) for r in results]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_oracle(orc, cam, name):
    case = index_cases.build(name, cam)
    assert len(case["frames"]) <= 8 and max(len(f[0]) for f in case["frames"]) <= index_cases.MAX_KP
    ora = index_cases.oracle_tail(orc, cam, name)
    veto_of = {}
    for f, (kp, desc, depth, boxes) in enumerate(case["frames"]):
        if len(boxes) and f > 0:
            veto, dist, nocreate = index_cases.oracle_veto(orc, ora[f][4], boxes, case["frames"][f - 1][0], kp)
            veto_of[f] = (veto, nocreate)
    ref = run_ref(case, veto_of)
    assert signature(ref) == signature(case["ref"])          # the veto the builder assumed is the one the geometry gives
    for f, (r, (res, cur, mg, ng, F, nv)) in enumerate(zip(ref, ora)):
        n = len(case["frames"][f][0])
        assert res["n_kp"] == n
        want_m, want_n = index_ref.as_reported(r, f)
        assert np.array_equal(want_m, mg[:n]) and (mg[n:] == -1).all(), (name, f)
        assert np.array_equal(want_n, ng[:n]) and (ng[n:] == -1).all(), (name, f)
        assert np.array_equal(r["rows"], cur[:n]), (name, f)
        for c in COUNTERS:
            assert r[c] == res[c], (name, f, c, r[c], res[c])
        assert len(r["vetoed"]) == nv, (name, f)


@pytest.mark.parametrize("name", NAMES)
def test_case_has_its_property(cam, name):
    case = index_cases.build(name, cam)
    ref = case["ref"]
    assert case["expect"] or name.startswith(("rows_", "counts"))
    for f, col, src, which in case["expect"]:
        want = -1 if src is None else ref[src[0]]["new_gid"][src[1]]
        assert src is None or want >= 0
        assert ref[f]["match_gid"][col] == want, (name, f, col, src)
        assert ref[f]["pass_of"][col] == which, (name, f, col, which)
    key = name if name in PROPERTIES else name.split("_")[0]           # dense_15 -> dense, rows_1024 -> rows, cull_1 -> cull
    PROPERTIES[key](case, name)


def _model(r, which):
    D = r["D1" if which == 1 else "D2"]
    thr = 15 if which == 1 else 30
    active = D.min(1) < thr
    ncols, entries = index_ref.list_model(D[active])
    return ncols, entries


def _p_ties_dense(case, name):
    for f, which, n in ((2, 2, 16), (4, 1, 16)):
        ncols, _ = _model(case["ref"][f], which)
        assert (ncols > 8).sum() >= n


def _p_ties_packed(case, name):
    for f, which in ((2, 2), (4, 1)):
        ncols, _ = _model(case["ref"][f], which)
        assert (ncols <= 8).all() and (ncols == 2).sum() >= 12 and (ncols == 3).sum() >= 4    # dense at track_lcap 1 / 2


def _p_chain300(case, name):
    r = case["ref"][2]
    ncols, _ = _model(r, 1 if "p1" in name else 2)
    assert (ncols >= 300).sum() == 300 and r["active"][0 if "p1" in name else 1] >= 300


def _p_dense_k(case, name):
    K = int(name.split("_")[1])
    ncols, _ = _model(case["ref"][2], 2)
    assert (ncols > 8).sum() == K and case["ref"][2]["active"][1] == K


def _p_alternating(case, name):
    ncols, entries = _model(case["ref"][2], 2)
    assert (ncols > 8).sum() == 61 and case["ref"][2]["n_match_pass2"] == 31


def _p_blockers(case, name):
    ncols, entries = _model(case["ref"][2], 2)
    nb = [e[2] for row in entries for e in row]
    assert nb.count(4) >= 2 and nb.count(1) >= 3 and (ncols <= 8).all()      # a fourth blocker: only the `more` bit knows
    inside = [row for row in entries if len(row) == 2 and row[0][1] == 20 and row[1][1] == 12]
    assert len(inside) == 2                                                  # the blocker inside the list


def _p_dense_join(case, name):
    ncols, entries = _model(case["ref"][2], 2)
    assert (ncols > 8).sum() == 40
    assert sum(1 for row, n in zip(entries, ncols) if n <= 8 and any(e[2] == 4 for e in row)) == 2


def _p_dense_lcap(case, name):
    ncols, _ = _model(case["ref"][2], 2)
    assert {1, 2, 3, 8, 9, 12} <= set(ncols.tolist())


def _p_rows(case, name):
    N = int(name.split("_")[1])
    r = case["ref"][3]
    assert r["active"] == [0, N] and len(r["D2"]) >= N
    ncols, _ = _model(r, 2)
    if N == 1440:
        assert sorted(set(ncols.tolist())) == [1, 30] and (ncols[1024:] == 30).sum() == 30    # a dense chain past row 1024
    else:
        assert (ncols == 1).all()                            # all packed: rows 1024 and up are dense by their number alone
    late = np.isin(r["rows"], r["rows2"][1024:]).sum()
    assert late == {1023: 0, 1024: 0, 1025: 1, 1300: 56, 1440: 30, 1500: 0}[N]      # rows 1024 and up that win a column (clusters 224, 229 .. 499)


def _p_counts(case, name):
    assert [len(f[0]) for f in case["frames"]] == [0, 64, 500, 0, 63, 65, 1, 500]
    assert [r["n_match_pass1"] + r["n_match_pass2"] for r in case["ref"]] == [0, 0, 64, 0, 63, 65, 1, 1]


def _p_counts_no_depth(case, name):
    assert (case["frames"][1][2] == -1).all() and case["ref"][1]["n_new_mappoints"] == 0 and case["ref"][3]["n_new_mappoints"] == 20


def _p_cull(case, name):
    assert case["ref"][4]["n_pool"] < case["ref"][4]["n_pool_before"]       # the compaction dropped rows


def _p_veto(case, name):
    r = case["ref"][2]
    assert r["vetoed"] == [1] and r["n_new_mappoints"] == 0
    assert all(q["n_pool"] >= 101 for q in case["ref"][2:5]) and case["ref"][5]["n_pool"] == 100   # bad, kept while local


PROPERTIES = {"ties_dense": _p_ties_dense, "ties_packed": _p_ties_packed, "chain_p1_300": _p_chain300, "chain_p2_300": _p_chain300,
              "dense": _p_dense_k, "chain_alternating": _p_alternating, "blockers": _p_blockers, "dense_join": _p_dense_join,
              "dense_lcap": _p_dense_lcap, "rows": _p_rows, "counts": _p_counts, "counts_no_depth": _p_counts_no_depth,
              "cull": _p_cull, "veto_chain": _p_veto, "thresholds": lambda c, n: None, "chains_small": lambda c, n: None}


def test_cull_cases_meet_pool_sizes_around_a_multiple_of_four(cam):
    seen = set()
    for name in ("cull_0", "cull_1", "cull_2"):
        for r in index_cases.build(name, cam)["ref"]:
            seen.add(("before", r["n_pool_before"] % 4)); seen.add(("after", r["n_pool"] % 4))
    assert {(w, m) for w in ("before", "after") for m in (3, 0, 1)} <= seen


def test_veto_geometry_is_far_from_the_threshold(orc, cam):
    case = index_cases.build("veto_chain", cam)
    ora = index_cases.oracle_tail(orc, cam, "veto_chain")
    kp, desc, depth, boxes = case["frames"][2]
    veto, dist, nocreate = index_cases.oracle_veto(orc, ora[2][4], boxes, case["frames"][1][0], kp)
    print("epipolar distances", dist[0, 0], dist[1, 1], dist[2, 1], dist[3, 2])
    assert dist[1, 1] > 1.0 and max(dist[0, 0], dist[2, 1], dist[3, 2]) < 0.01
    assert np.array_equal(nocreate, case["fiat"][2][1]) and ora[2][5] == 1
    assert np.isfinite(dist).any(axis=0).sum() == 4          # the four chain columns, and only they, lie in the padded box


@pytest.mark.parametrize("name", [n for n in SMALL if n != "veto_chain"])      # (the round restatement takes no veto)
def test_rounds_equal_the_sequential_scan(cam, name):
    """The round scheme (rank-aware claims, finality rule) restated on full rows gives the sequential result."""
    case = index_cases.build(name, cam)
    got = run_ref(case, rounds=True)
    assert signature(got) == signature(case["ref"])
    print(name, "rounds per frame (pass 1, pass 2):", [r["rounds"] for r in got])


MUTANTS = [dict(ratio_ge=True), dict(global_second=True), dict(last_tie=True), dict(claimed_blocks=True), dict(reverse=True),
           dict(rank_blind=True), dict(keep_observed=True), dict(thr1=14), dict(thr1=16), dict(thr2=29), dict(thr2=31),
           dict(cull_age=3), dict(cull_age=5), dict(drop_referenced=True)]


@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda m: "-".join("%s=%s" % kv for kv in m.items()))
def test_mutant_changes_an_expected_output(cam, mutant):
    killers = []
    for name in SMALL:
        case = index_cases.build(name, cam)
        if mutant.get("rank_blind") and case["fiat"]:
            continue
        if signature(run_ref(case, **mutant)) != signature(case["ref"]):
            killers.append(name)
            if len(killers) == 3:
                break
    print(mutant, "changes", killers)
    assert killers
