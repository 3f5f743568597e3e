"""Bag of words without a GPU: the symbols, every argument check and loader refusal, the text round trip through the library, the
library's loader against the twin's, the twin on hand-computed examples, the training's properties, and the mutant table: every
rule of the contract (DESIGN.md section 8 "Bag of words") has a named case that tells it from its neighbour."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import bow_cases as Cs
import bow_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1

BOW_SYMBOLS = ["svo_bow_create_from_text", "svo_bow_create", "svo_bow_save_text", "svo_bow_describe", "svo_bow_destroy", "svo_bow_sync",
               "svo_bow_stream", "svo_bow_last_error", "svo_bow_transform_dev", "svo_bow_transform", "svo_bow_score_dev",
               "svo_bow_query_dev", "svo_bow_assign_dev"]


# ---- symbols ------------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "svo.h")).read()
    lib = pkg.load_library()
    for name in BOW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in pkg.ABI_SYMBOLS and hasattr(lib, name), name
    assert lib.svo_abi_version() == 8
    for name in ("from_text", "from_arrays", "save_text", "describe", "transform", "transform_dev", "score_dev", "query_dev",
                 "assign_dev", "sync", "stream"):
        assert hasattr(pkg.Vocabulary, name), name
    assert pkg.BOW_ENTRY_DTYPE == R.ENTRY and pkg.BOW_FEATURE_DTYPE == R.FEATURE and pkg.BOW_CAND_DTYPE == R.CAND
    assert pkg.BOW_ENTRY_DTYPE.itemsize == 16 and pkg.BOW_FEATURE_DTYPE.itemsize == 8 and pkg.BOW_CAND_DTYPE.itemsize == 16


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _tiny_lines():
    return open(Cs.TINY).read().split("\n")


def _refused(pkg, text, tmp_path, needle, **kw):
    p = tmp_path / "voc.txt"
    p.write_text(text)
    with pytest.raises(pkg.SvoError) as e:
        pkg.Vocabulary.from_text(str(p), **kw)
    assert "bad argument" in str(e.value) or "invalid" in str(e.value).lower(), str(e.value)
    assert needle in str(e.value), str(e.value)
    with pytest.raises(ValueError):        # the twin's loader refuses the same files
        R.parse_text(text)


def test_loader_refusals_name_the_line(pkg, tmp_path):
    L = _tiny_lines()

    def swap(i, new):
        return "\n".join(L[:i] + [new] + L[i + 1:])
    _refused(pkg, swap(0, "4 3  1 0"), tmp_path, "line 1: scoring")
    _refused(pkg, swap(0, "4 3  0 4"), tmp_path, "line 1: weighting")
    _refused(pkg, swap(0, "4 3  0 -1"), tmp_path, "line 1: weighting")
    _refused(pkg, swap(0, "1 3  0 0"), tmp_path, "line 1: k")
    _refused(pkg, swap(0, "21 3  0 0"), tmp_path, "line 1: k")
    _refused(pkg, swap(0, "4 0  0 0"), tmp_path, "line 1: L")
    _refused(pkg, swap(0, "4 11  0 0"), tmp_path, "line 1: L")
    # node 3 (line 4) names parent 3: not defined yet; node 9 (line 10) names parent 12
    _refused(pkg, swap(3, "3 " + L[3].split(" ", 1)[1]), tmp_path, "line 4: parent 3 is not defined yet")
    _refused(pkg, swap(9, "12 " + L[9].split(" ", 1)[1]), tmp_path, "line 10: parent 12 is not defined yet")
    # node 13 (line 14) is inner; without its three children (lines 15 .. 17) it has none
    _refused(pkg, "\n".join(L[:14] + L[17:]), tmp_path, "line 14: an inner node without children")
    # node 4 (line 5) is a leaf: a child of it
    _refused(pkg, "\n".join(L[:20] + ["4 1 " + " ".join(["9"] * 32) + " 1"]) + "\n", tmp_path, "line 21: parent 4 is marked a leaf")
    # a fifth child of the root with k = 4
    _refused(pkg, "\n".join(L[:20] + ["0 1 " + " ".join(["9"] * 32) + " 1"]) + "\n", tmp_path, "more than k children")
    _refused(pkg, swap(5, L[5].replace(" 3 3 ", " 3 256 ", 1)), tmp_path, "line 6")
    _refused(pkg, swap(5, " ".join(L[5].split()[:-1])), tmp_path, "line 6")
    _refused(pkg, "", tmp_path, "header")
    with pytest.raises(pkg.SvoError) as e:
        pkg.Vocabulary.from_text(str(tmp_path / "absent.txt"))
    assert "cannot open" in str(e.value)


def test_constructor_argument_checks(pkg, tmp_path):
    v = Cs.tiny()
    for kw, needle in ((dict(max_kp=0), "max_kp"), (dict(max_kp=2049), "max_kp"), (dict(max_frames=0), "max_frames"),
                       (dict(max_frames=65536), "max_frames"), (dict(device=-1), "device")):
        with pytest.raises(pkg.SvoError) as e:
            pkg.Vocabulary.from_text(Cs.TINY, **kw)
        assert needle in str(e.value)
    ok = dict(k=v.k, L=v.L, weighting=0, parents=v.parent, descriptors=v.desc, weights=v.weight)
    for change, needle in ((dict(k=1), "k must"), (dict(k=21), "k must"), (dict(L=0), "L must"), (dict(L=11), "L must"),
                           (dict(weighting=4), "weighting"), (dict(weighting=-1), "weighting"), (dict(k=3), "more than k children"),
                           (dict(parents=np.r_[v.parent[:5], 7, v.parent[6:]]), "node 5: parent 7 is not defined yet"),
                           (dict(parents=v.parent[:1], descriptors=v.desc[:1], weights=v.weight[:1]), "needs the root")):
        with pytest.raises(pkg.SvoError) as e:
            pkg.Vocabulary.from_arrays(**dict(ok, **change))
        assert needle in str(e.value), str(e.value)
    lib = pkg.load_library()
    pkg.Vocabulary._bind()
    h = C.c_void_p()
    assert lib.svo_bow_create(0, 4, 3, 0, 20, None, None, None, 500, 1, C.byref(h)) == E_INVALID
    assert lib.svo_bow_create_from_text(0, None, 500, 1, C.byref(h)) == E_INVALID
    assert lib.svo_bow_create_from_text(0, Cs.TINY.encode(), 500, 1, None) == E_INVALID
    assert b"out is NULL" in lib.svo_bow_last_error(None)


def test_entry_argument_checks_answer_without_a_device(pkg):
    """Every check of the device entries answers SVO_E_INVALID with its message before a device is touched: pointers are never
    followed, so made-up addresses do."""
    voc = pkg.Vocabulary.from_text(Cs.TINY, max_kp=64, max_frames=4)
    lib, h = voc.lib, voc.h
    P, Q = 0x1000, 0x2000

    def bad(rc, needle):
        assert rc == E_INVALID
        assert needle in lib.svo_bow_last_error(h).decode(), lib.svo_bow_last_error(h)
    t = lib.svo_bow_transform_dev
    bad(t(h, None, P, 64, 1, 0, None, None, None, None, None, None), "d_desc is NULL")
    bad(t(h, P, None, 64, 1, 0, None, None, None, None, None, None), "d_n is NULL")
    bad(t(h, P + 2, P, 64, 1, 0, None, None, None, None, None, None), "4-byte aligned")
    bad(t(h, P, P, 0, 1, 0, None, None, None, None, None, None), "kp_stride")
    bad(t(h, P, P, 65, 1, 0, None, None, None, None, None, None), "kp_stride")
    bad(t(h, P, P, 64, 0, 0, None, None, None, None, None, None), "B must")
    bad(t(h, P, P, 64, 5, 0, None, None, None, None, None, None), "B must")
    bad(t(h, P, P, 64, 1, -1, None, None, None, None, None, None), "levelsup")
    assert t(None, P, P, 64, 1, 0, None, None, None, None, None, None) == E_INVALID
    assert b"bow is NULL" in lib.svo_bow_last_error(None)
    d = np.zeros((4, 32), np.uint8)
    n1 = C.c_int32(0)
    one = lib.svo_bow_transform
    bad(one(h, d.ctypes.data, 65, 0, None, None, None, None, None), "n must")
    bad(one(h, d.ctypes.data, -1, 0, None, None, None, None, None), "n must")
    bad(one(h, None, 4, 0, None, None, None, None, None), "desc is NULL")
    bad(one(h, d.ctypes.data, 4, -1, None, None, None, None, None), "levelsup")
    bad(one(h, d.ctypes.data, 4, 0, None, P, None, None, None), "vec and vec_n")
    bad(one(h, d.ctypes.data, 4, 0, None, None, None, None, C.addressof(n1)), "fv and fv_n")
    s = lib.svo_bow_score_dev
    bad(s(h, None, P, 1, P, P, 1, 64, P), "NULL")
    bad(s(h, P, P, 1, P, P, 1, 64, None), "NULL")
    bad(s(h, P + 4, P, 1, P, P, 1, 64, P), "8-byte aligned")
    bad(s(h, P, P, 0, P, P, 1, 64, P), "QA must")
    bad(s(h, P, P, 65536, P, P, 1, 64, P), "QA must")
    bad(s(h, P, P, 1, P, P, 0, 64, P), "NB must")
    bad(s(h, P, P, 1, P, P, 1, 0, P), "stride")
    bad(s(h, P, P, 1, P, P, 1, 65, P), "stride")
    q = lib.svo_bow_query_dev
    bad(q(h, None, P, 64, 10, 0, 1, 0, 0.0, 4, P, P), "NULL")
    bad(q(h, P, P, 64, 10, 0, 1, 0, 0.0, 4, None, P), "NULL")
    bad(q(h, P, P, 64, 10, 0, 1, 0, 0.0, 4, P + 4, P), "8-byte aligned")
    bad(q(h, P, P, 65, 10, 0, 1, 0, 0.0, 4, P, P), "stride")
    bad(q(h, P, P, 64, 0, 0, 1, 0, 0.0, 4, P, P), "N must")
    bad(q(h, P, P, 64, 10, -1, 1, 0, 0.0, 4, P, P), "queries")
    bad(q(h, P, P, 64, 10, 0, 0, 0, 0.0, 4, P, P), "queries")
    bad(q(h, P, P, 64, 10, 8, 3, 0, 0.0, 4, P, P), "queries")
    bad(q(h, P, P, 64, 10, 0, 1, -1, 0.0, 4, P, P), "gap")
    bad(q(h, P, P, 64, 10, 0, 1, 0, math.nan, 4, P, P), "min_score")
    bad(q(h, P, P, 64, 10, 0, 1, 0, 0.0, 0, P, P), "top_k")
    bad(q(h, P, P, 64, 10, 0, 1, 0, 0.0, 17, P, P), "top_k")
    a = lib.svo_bow_assign_dev
    bad(a(h, None, 1, Q, 2, P, P), "NULL")
    bad(a(h, P, 1, None, 2, P, P), "NULL")
    bad(a(h, P + 1, 1, Q, 2, P, P), "4-byte aligned")
    bad(a(h, P, 0, Q, 2, P, P), "n must")
    bad(a(h, P, 1, Q, 0, P, P), "k must")
    bad(a(h, P, 1, Q, 21, P, P), "k must")
    assert lib.svo_bow_sync(h) == 0 and lib.svo_bow_sync(None) == E_INVALID
    assert lib.svo_bow_save_text(h, None) == E_INVALID and lib.svo_bow_describe(None, None, None, None, None, None) == E_INVALID
    voc.close()


# ---- text format ----------------------------------------------------------------------------------------------------------------------
def _trained():
    rng = np.random.default_rng(3)
    docs = [Cs.near(100 + i, Cs.rand_desc(2, 12), int(rng.integers(5, 40)), flips=int(rng.integers(2, 30))) for i in range(12)]
    return docs, R.train(docs, 4, 3, R.TF_IDF, seed=5)


@pytest.fixture(scope="module")
def trained():
    return _trained()


def test_text_round_trip_is_byte_identical(pkg, tmp_path, trained):
    for name, text in (("tiny", open(Cs.TINY).read()), ("trained", R.format_text(trained[1])),
                       ("shuffled", R.format_text(Cs.walk_ragged(True)["voc"]))):
        a, b = tmp_path / (name + "_a.txt"), tmp_path / (name + "_b.txt")
        a.write_text(text)
        voc = pkg.Vocabulary.from_text(str(a))
        voc.save_text(str(b))
        assert b.read_bytes() == text.encode(), name
        voc.close()


def test_library_loader_against_twin_loader(pkg, tmp_path, trained):
    for v in (Cs.tiny(), trained[1]):
        p = tmp_path / "v.txt"
        p.write_text(R.format_text(v))
        voc = pkg.Vocabulary.from_text(str(p))
        assert voc.describe() == v.describe()
        arr = pkg.Vocabulary.from_arrays(v.k, v.L, v.weighting, v.parent, v.desc, v.weight)
        assert arr.describe() == v.describe()
        q = tmp_path / "w.txt"
        arr.save_text(str(q))
        w = R.parse_text(q.read_text())
        assert np.array_equal(w.parent, v.parent) and np.array_equal(w.desc[1:], v.desc[1:])
        assert w.weight.tobytes() == v.weight.tobytes() and np.array_equal(w.word, v.word)
        voc.close(), arr.close()


def test_blank_lines_and_ragged_text(pkg, tmp_path):
    """A file may end in blank lines (DBoW2's own loop reads one); a blank line between nodes would shift the ids: refused."""
    text = open(Cs.TINY).read()
    p = tmp_path / "v.txt"
    p.write_text(text + "\n  \n")
    assert pkg.Vocabulary.from_text(str(p)).describe() == Cs.tiny().describe()
    L = text.split("\n")
    p.write_text("\n".join(L[:5] + [""] + L[5:]))
    with pytest.raises(pkg.SvoError) as e:
        pkg.Vocabulary.from_text(str(p))
    assert "line 7: an empty line between nodes" in str(e.value)


# ---- the twin on hand-computed examples (tests/golden/bow_tiny_voc.txt: every centre is one byte 32 times) ------------------------------
def test_twin_walk_by_hand():
    v = Cs.tiny()
    assert v.describe() == dict(k=4, L=3, nodes=20, words=15, weighting=0)
    assert v.word_node.tolist() == [3, 4, 5, 6, 7, 9, 10, 11, 12, 14, 15, 16, 17, 18, 19]
    # 0x07: 96, 160, 32 and 32 from the root's children 1, 2, 4, 17: the tie keeps 4, a leaf at level 1 (word 1, weight 1.25)
    assert [R.walk(v, Cs.flat(0x07), ls)[:3] for ls in (0, 1, 2, 3, 4)] == [(1, 1.25, 4)] * 3 + [(1, 1.25, 0)] * 2
    # 0x30: node 1 (64 against 192, 192, 192), node 13 (96, 128, 160, 32), node 15 (64, 0, 64)
    assert [R.walk(v, Cs.flat(0x30), ls)[2] for ls in (0, 1, 2, 3)] == [15, 13, 1, 0]
    assert R.walk(v, Cs.flat(0x30))[:2] == (10, 0.125) and R.walk(v, Cs.flat(0x30))[3] == [1, 13, 15]
    # 0x11 below node 1: 32 from node 3 and from node 13: the earlier child, a leaf at level 2; nid at level 3 is that leaf
    assert [R.walk(v, Cs.flat(0x11), ls)[:3] for ls in (0, 1, 2)] == [(0, 0.5, 3), (0, 0.5, 3), (0, 0.5, 1)]
    # 0x03: a tie of 64 between the root's children 1 and 4 keeps 1; node 5 at distance 0 is a stop word
    assert R.walk(v, Cs.flat(0x03))[:3] == (2, 0.0, 5)


def test_twin_vectors_by_hand():
    v = Cs.tiny()
    descs = np.stack([Cs.flat(b) for b in (0x30, 0x07, 0x03, 0x07, 0x01, 0x07, 0x11)])
    words, vec, fv = R.transform(v, descs, levelsup=1)
    assert words.tolist() == [10, 1, -1, 1, 0, 1, 0]
    # word 0: 0.5 + 0.5, word 1: 1.25 three times, word 10: 0.125; norm = 1.0 + 3.75 + 0.125 (all exact)
    assert vec["word"].tolist() == [0, 1, 10] and vec["value"].tolist() == [1.0 / 4.875, 3.75 / 4.875, 0.125 / 4.875]
    assert [tuple(x) for x in fv.tolist()] == [(3, 4), (3, 6), (4, 1), (4, 3), (4, 5), (13, 0)]
    v.weighting = R.IDF
    vec = R.transform(v, descs)[1]
    assert vec["value"].tolist() == [0.5 / 1.875, 1.25 / 1.875, 0.125 / 1.875]


def test_twin_score_and_query_by_hand():
    a = np.array([(1, 0, 0.5), (4, 0, 0.25), (9, 0, 0.25)], R.ENTRY)
    b = np.array([(0, 0, 0.5), (4, 0, 0.5)], R.ENTRY)
    assert R.score(a, b) == -((abs(0.25 - 0.5) - 0.25 - 0.5) / 2.0) == 0.25
    assert R.score(a, a) == 1.0 and R.score(a[:1], b[:1]) == 0.0 and np.signbit(R.score(a[:1], b[:1]))
    assert np.signbit(R.score(a[:0], b))
    row = np.array([0.3, 0.5, 0.3, 0.1, 0.5, 0.9])
    c, n = R.select(row, 5, 0, 0.1, 3)
    assert n == 3 and c["frame"].tolist() == [1, 4, 0] and c["score"].tolist() == [0.5, 0.5, 0.3]
    c, n = R.select(row, 5, 1, 0.1, 16)
    assert n == 3 and c["frame"].tolist()[:4] == [1, 0, 2, -1] and c["score"][3] == 0.0
    assert R.select(row, 5, 5, 0.0, 4)[1] == 0 and R.select(row, 5, 9, 0.0, 4)[1] == 0
    assert R.select(row, 5, 4, 0.0, 4)[0]["frame"].tolist() == [0, -1, -1, -1]


# ---- training ---------------------------------------------------------------------------------------------------------------------------
def test_training_properties(trained):
    docs, v = trained
    feats = np.concatenate(docs)
    assert any(0 < len(c) < v.k for c in v.children) or any(v.level(int(n)) < v.L for n in v.word_node), "not a ragged tree"
    # every descriptor's leaf is the leaf the walk finds (of two equal centres under one parent the walk takes the earlier: equal
    # features of a trivial step), and idf = log(NDocs / Ni) with Ni counted once per document; a word no walk reaches keeps 0
    ni = np.zeros(v.n_words, int)
    at = 0
    for d in docs:
        leaf = np.array([R.walk(v, x)[3][-1] for x in d])
        want = v.train_leaf[at:at + len(d)]
        at += len(d)
        assert np.array_equal(v.desc[leaf], v.desc[want]) and (leaf <= want).all() and (leaf == want).mean() > 0.9
        assert np.array_equal(v.parent[leaf], v.parent[want])
        w = v.word[leaf]
        assert np.array_equal(w, R.leaf_words(v, d))
        ni[np.unique(w)] += 1
    for w in range(v.n_words):
        assert v.weight[v.word_node[w]] == (math.log(float(len(docs)) / float(ni[w])) if ni[w] else 0.0)
    assert all(v.weight[i] == 0.0 for i in range(len(v.parent)) if v.children[i])
    # a leaf above level L holds one feature (or several equal ones would have been split: their mean is themselves)
    words = R.leaf_words(v, feats)
    for w in range(v.n_words):
        node = int(v.word_node[w])
        if v.level(node) < v.L:
            held = feats[words == w]
            assert len(held) >= 1 and (held == held[0]).all() and np.array_equal(v.desc[node], held[0])
    assert R.format_text(R.train(docs, 4, 3, R.TF_IDF, seed=5)) == R.format_text(v)
    assert R.format_text(R.train(docs, 4, 3, R.TF_IDF, seed=6)) != R.format_text(v)


def test_training_trivial_case_and_weightings():
    d = Cs.rand_desc(1, 3)
    v = R.train([d[:2], d[2:]], 5, 2, R.TF_IDF, seed=0)          # n <= k: one child per feature, in feature order
    assert v.parent.tolist() == [-1, 0, 0, 0] and np.array_equal(v.desc[1:], d)
    assert v.weight.tolist() == [0.0] + [math.log(2.0)] * 3
    assert R.train([d[:2], d[2:]], 5, 2, R.BINARY, seed=0).weight.tolist() == [0.0, 1.0, 1.0, 1.0]
    v = R.train([np.concatenate([d, d[:1]])], 5, 2, R.IDF, seed=0)
    assert v.weight.tolist() == [0.0, 0.0, 0.0, 0.0, 0.0]         # one document: ln(1 / 1), every word a stop word
    assert len(v.parent) == 5


def test_mean_value_by_hand():
    a, b, c = Cs.flat(0b11110000), Cs.flat(0b11001100), Cs.flat(0b10101010)
    assert np.array_equal(R.mean_value([a]), a)
    assert np.array_equal(R.mean_value([a, b]), Cs.flat(0b11111100))          # N2 = 1: a bit one of two has
    assert np.array_equal(R.mean_value([a, b, c]), Cs.flat(0b11101000))       # N2 = 2
    assert np.array_equal(R.mean_value([a, b, c, c]), Cs.flat(0b11101010))    # N2 = 2 of four


# ---- the mutant table: each neighbour of a rule is told apart by a named case --------------------------------------------------------------
def _vec_bytes(case, rules, levelsup=0):
    w, vec, fv = R.transform(case["voc"], case["descs"], levelsup, rules)
    return w.tobytes() + vec.tobytes() + fv.tobytes()


def _weighting_case():
    v = Cs.vec_voc(R.IDF)
    return dict(voc=v, descs=Cs.vec_frames(v, [120], seed=91, dup=0.5)[0])


def _query_bytes(case, rules, gap=3):
    vecs = case["vecs"]
    c, n = R.query(vecs, len(vecs) - 4, 4, gap, -1.0, 16, rules)
    return c.tobytes() + n.tobytes()


MUTANTS = [
    ("tie to the last child", dict(tie_last=True), lambda r: _vec_bytes(Cs.walk_ties("first"), r)),
    ("tie to the last child (last two)", dict(tie_last=True), lambda r: _vec_bytes(Cs.walk_ties("last"), r)),
    ("c * w instead of repeated addition", dict(multiply=True), lambda r: _vec_bytes(Cs.vec_repeat500(), r)),
    ("norm summed in feature order", dict(norm_feature_order=True), lambda r: _vec_bytes(Cs.vec_norm_order(), r)),
    ("stop words kept", dict(keep_stop=True), lambda r: _vec_bytes(Cs.vec_stop_mixed(), r)),
    ("addWeight where addIfNotExist belongs", dict(add_always=True), lambda r: _vec_bytes(_weighting_case(), r)),
    ("levelsup off by one (+)", dict(levelsup_off=1), lambda r: _vec_bytes(Cs.walk_ragged(), r, 1)),
    ("levelsup off by one (-)", dict(levelsup_off=-1), lambda r: _vec_bytes(Cs.walk_ragged(), r, 1)),
    ("majority with n / 2", dict(majority_half=True), lambda r: R.format_text(R.train(_trained()[0], 4, 3, R.TF_IDF, 5, rules=r)).encode()),
    ("score without the sign of zero", dict(drop_zero_sign=True), lambda r: R.scores(Cs.score_sets()["A"], Cs.score_sets()["B"], r).tobytes()),
    ("candidate ties by descending j", dict(cand_desc_j=True), lambda r: _query_bytes(Cs.query_db(), r)),
    ("gap off by one (+)", dict(gap_off=1), lambda r: _query_bytes(Cs.query_db(), r, gap=30)),
    ("gap off by one (-)", dict(gap_off=-1), lambda r: _query_bytes(Cs.query_db(), r, gap=30)),
]


@pytest.mark.parametrize("name,kw,run", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_mutant_is_killed(name, kw, run):
    assert run(R.CONTRACT) != run(R.Rules(**kw)), name
    assert run(R.CONTRACT) == run(R.Rules()), "the case is not deterministic"


def test_every_case_has_its_edge():
    for c in (Cs.walk_random(3, 3), Cs.walk_random(10, 6, 0.6), Cs.walk_ties("first"), Cs.walk_ties("last"), Cs.walk_ties("all"),
              Cs.walk_ragged(False), Cs.walk_ragged(True), Cs.vec_repeat500(), Cs.vec_all_different(), Cs.vec_all_stopped(),
              Cs.vec_stop_mixed(), Cs.vec_norm_order(), Cs.score_sets(), Cs.query_db()):
        c["prove"]()


def test_repeated_addition_is_not_a_product():
    s, first = 0.0, None
    for c in range(1, 501):
        s += Cs.W73
        if first is None and s != c * Cs.W73:
            first = c
    assert first == 6


def test_restatement_pins():
    """counts and digests of the twin's results on the named cases (tools/make_bow_pins.py wrote them)"""
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_bow_pins
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "bow_restatement_pins.json")))
    got = make_bow_pins.pins()
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
