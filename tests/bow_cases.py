"""Named, seeded cases for the bag-of-words tests.  Every builder returns a dict; its `prove` checks, on the twin's own
intermediates, that the case has the edge its name promises (a case that lost its edge fails there, not silently).
Vocabularies come from bow_ref.random_tree in milliseconds; tests/golden/bow_tiny_voc.txt is the one hand-written file."""
import math
import os

import numpy as np

import bow_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
TINY = os.path.join(HERE, "golden", "bow_tiny_voc.txt")
W73 = math.log(7.0 / 3.0)       # a weight for which w added c times differs from c * w (from c = 6 on)


def tiny():
    return R.parse_text(open(TINY).read())


def flat(byte):
    return np.full(32, byte, np.uint8)


def rand_desc(seed, n):
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)


def near(seed, centres, n, flips=6):
    """n descriptors, each a random centre with `flips` random bits turned."""
    rng = np.random.default_rng(seed)
    out = centres[rng.integers(0, len(centres), n)].copy()
    for d in out:
        for b in rng.integers(0, 256, flips):
            d[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


# ---- walk ------------------------------------------------------------------------------------------------------------------------
def walk_random(k, L, ragged=0.0, seed=11):
    """Random descriptors, copies of centres (distance 0) and complements of centres (distance 256) through a full tree, or
    (ragged > 0: the deep trees of a large k) through a sparse one that still reaches level L."""
    for s in range(50 if ragged else 1):      # (a sparse tree of a useful size: the first seed that gives one)
        v = R.random_tree(seed + 100 * k + L + 1000 * s, k, L, ragged=ragged)
        first = np.asarray(v.children[0])
        descs = np.concatenate([rand_desc(seed, 40), v.desc[first[:2]], ~v.desc[first[-1:]], near(seed + 1, v.desc[v.word_node], 40)])
        if not ragged or (500 < len(v.parent) < 20000 and max(len(R.walk(v, x)[3]) for x in descs) == L):
            break

    def prove():
        d = R.hamming(descs[:, None, :], v.desc[first][None])
        assert (d == 0).any() and (d == 256).any()
        if ragged:
            assert max(len(R.walk(v, x)[3]) for x in descs) == L and max(len(c) for c in v.children) == k
        else:
            assert all(len(c) in (0, k) for c in v.children)
    return dict(voc=v, descs=descs, prove=prove)


def walk_ties(which, k=5):
    """One level of k children with equal centres: 'first' child 0 and child 2, 'last' the last two, 'all' every child."""
    rng = np.random.default_rng(5)
    c = rng.integers(0, 256, (k, 32), dtype=np.uint8)
    if which == "first":
        c[2] = c[0]
        probe, want = c[0], 0
    elif which == "last":
        c[k - 1] = c[k - 2]
        probe, want = c[k - 2], k - 2
    else:
        c[:] = c[0]
        probe, want = c[0], 0
    parent = np.array([-1] + [0] * k, np.int32)
    v = R.Voc(k, 1, R.TF, parent, np.concatenate([np.zeros((1, 32), np.uint8), c]), np.array([0.0] + [1.0] * k))
    descs = np.concatenate([probe[None], near(9, probe[None], 7, flips=3)])

    def prove():
        for d in descs:
            dist = R.hamming(d[None], c)
            assert (dist == dist.min()).sum() >= 2 and int(np.argmin(dist)) == want
            assert R.walk(v, d)[0] == want
            assert R.walk(v, d, rules=R.Rules(tie_last=True))[0] != want
    return dict(voc=v, descs=descs, prove=prove)


def walk_ragged(shuffle=False):
    """A ragged tree (k = 6, L = 4): a leaf at level 1 beside leaves at level L, nodes with fewer than k children."""
    for seed in range(200):
        v = R.random_tree(1000 + seed, 6, 4, ragged=0.35, shuffle_ids=shuffle, stop=0.2)
        lv = [v.level(int(nd)) for nd in v.word_node]
        if 1 in lv and 4 in lv and any(0 < len(c) < 6 for c in v.children) and len(v.parent) > 60:
            break
    else:
        raise AssertionError("no ragged tree among the seeds")
    descs = np.concatenate([rand_desc(3, 60), near(4, v.desc[v.word_node], 60)])

    def prove():
        ends = {v.level(R.walk(v, d)[3][-1]) for d in descs}
        assert 1 in ends and 4 in ends, ends
        if shuffle:     # some node's children are not contiguous by id
            assert any(c and c[-1] - c[0] != len(c) - 1 for c in v.children)
        w = [R.walk(v, d)[1] for d in descs]
        assert any(x > 0 for x in w) and any(not x > 0 for x in w)
    return dict(voc=v, descs=descs, prove=prove)


# ---- vectors -----------------------------------------------------------------------------------------------------------------------
def vec_voc(weighting=R.TF_IDF, stop=0.0, seed=21):
    return R.random_tree(seed, 10, 3, weighting=weighting, stop=stop)


def vec_frames(v, counts, seed=31, dup=0.3):
    """Frames of the given lengths near the vocabulary's words, a share of them repeated so that words occur more than once."""
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(counts):
        d = near(seed + i, v.desc[v.word_node], n, flips=4)
        if n > 1 and dup:
            src = rng.integers(0, n, n)
            rep = rng.random(n) < dup
            d[rep] = d[src[rep]]
        out.append(d)
    return out


def vec_repeat500():
    """500 features in one word of weight ln(7/3) and 3 in another: the repeated addition shows in the normalised values."""
    c = rand_desc(77, 2)
    v = R.Voc(2, 1, R.TF_IDF, [-1, 0, 0], np.concatenate([np.zeros((1, 32), np.uint8), c]), [0.0, W73, 1.0])
    descs = np.concatenate([np.repeat(c[:1], 500, axis=0), np.repeat(c[1:], 3, axis=0)])

    def prove():
        s = 0.0
        for _ in range(500):
            s += W73
        assert s != 500 * W73
        a = R.transform(v, descs)[1]
        b = R.transform(v, descs, rules=R.Rules(multiply=True))[1]
        assert len(a) == 2 and a.tobytes() != b.tobytes()
    return dict(voc=v, descs=descs, prove=prove)


def vec_all_different():
    v = R.random_tree(41, 20, 2)
    descs = v.desc[v.word_node][::7][:50].copy()

    def prove():
        w, vec, fv = R.transform(v, descs)
        assert len(vec) == len(descs) == len(set(w.tolist())) == len(fv)
    return dict(voc=v, descs=descs, prove=prove)


def vec_all_stopped():
    v = vec_voc(stop=1.0)
    descs = rand_desc(8, 70)

    def prove():
        w, vec, fv = R.transform(v, descs)
        assert (w == -1).all() and len(vec) == 0 and len(fv) == 0
    return dict(voc=v, descs=descs, prove=prove)


def vec_stop_mixed():
    v = vec_voc(stop=0.4)
    descs = vec_frames(v, [200], seed=51)[0]

    def prove():
        w, vec, fv = R.transform(v, descs)
        assert 0 < (w == -1).sum() < len(w) and len(fv) == (w >= 0).sum()
        assert R.transform(v, descs, rules=R.Rules(keep_stop=True))[1].tobytes() != vec.tobytes()
    return dict(voc=v, descs=descs, prove=prove)


def vec_norm_order():
    """Three words whose |values| sum differently in word order and in feature order."""
    c = rand_desc(78, 3)
    for a, b, d in ((1e16, 1.0, 1.0), (0.1, 0.2, 0.3)):
        if (a + b) + d != (d + b) + a:
            break
    v = R.Voc(3, 1, R.TF_IDF, [-1, 0, 0, 0], np.concatenate([np.zeros((1, 32), np.uint8), c]), [0.0, a, b, d])
    descs = c[::-1].copy()          # feature order: word 2, 1, 0

    def prove():
        x = R.transform(v, descs)[1]
        y = R.transform(v, descs, rules=R.Rules(norm_feature_order=True))[1]
        assert x.tobytes() != y.tobytes()
    return dict(voc=v, descs=descs, prove=prove)


# ---- scores and queries ------------------------------------------------------------------------------------------------------------
def make_vec(rng, n, n_words=5000, words=None):
    """A normalised vector of n entries over random ascending words."""
    if words is None:
        words = np.sort(rng.choice(n_words, n, replace=False))
    v = np.zeros(len(words), R.ENTRY)
    v["word"] = words
    x = rng.random(len(words)) + 0.01
    norm = 0.0
    for t in x:
        norm += t
    v["value"] = x / norm if len(words) else x
    return v


def score_sets():
    """Two sets of vectors: lengths 0, 1, 63, 64, 65, 500, disjoint pairs, a common word only at the first / only at the last entry."""
    rng = np.random.default_rng(61)
    A = [make_vec(rng, n, 700) for n in (0, 1, 63, 64, 65, 500)]
    B = [make_vec(rng, n, 700) for n in (500, 65, 64, 63, 1, 0)]
    lo = make_vec(rng, 0, words=np.arange(10, 60))
    hi = make_vec(rng, 0, words=np.arange(1000, 1070))
    first = make_vec(rng, 0, words=np.concatenate([[10], np.arange(2000, 2040)]))      # shares only its first entry with lo
    last = make_vec(rng, 0, words=np.concatenate([np.arange(0, 5), [59]]))              # shares only its last entry with lo
    one = make_vec(rng, 0, words=np.array([lo["word"][7]]))
    A += [lo, hi, first, last, one]
    B += [lo, hi, first, last, one]

    def prove():
        assert np.signbit(R.score(lo, hi)) and R.score(lo, hi) == 0.0
        assert set(lo["word"]) & set(first["word"]) == {first["word"][0]}
        assert set(lo["word"]) & set(last["word"]) == {last["word"][-1]}
        assert R.score(lo, hi, R.Rules(drop_zero_sign=True)).hex() != R.score(lo, hi).hex()
    return dict(A=A, B=B, prove=prove)


def query_db(n=40, seed=71):
    """A database with planted duplicates (equal scores) and near duplicates, over few words so that most pairs share some."""
    rng = np.random.default_rng(seed)
    vecs = [make_vec(rng, int(rng.integers(20, 90)), 300) for _ in range(n)]
    for dst, src in ((9, 2), (17, 2), (25, 2), (30, 11), (12, 11)):
        vecs[dst] = vecs[src].copy()
    vecs[5] = make_vec(rng, 0, words=np.arange(100000, 100010))     # shares nothing: -0.0 against everything
    vecs[n - 1] = make_vec(rng, 0, words=vecs[2]["word"])            # the last frame sees the place of 2, 9, 17 and 25 again

    def prove():
        row = np.array([R.score(vecs[n - 1], vecs[j]) for j in range(n - 1)])
        assert row[2] == row[9] == row[17] == row[25] and row[2] > 0
        a = R.select(row, n - 1, 0, -1.0, 16)[0]
        b = R.select(row, n - 1, 0, -1.0, 16, R.Rules(cand_desc_j=True))[0]
        assert a.tobytes() != b.tobytes() and a["frame"][:4].tolist() == [2, 9, 17, 25]
    return dict(vecs=vecs, prove=prove)


def pack(vecs, stride):
    """The device layout: (len(vecs), stride) entries and the counts; the unused entries hold a pattern that must not matter."""
    out = np.zeros((len(vecs), stride), R.ENTRY)
    out["word"] = 0xFFFFFFF0
    out["value"] = np.nan
    n = np.zeros(len(vecs), np.int32)
    for i, v in enumerate(vecs):
        out[i, :len(v)] = v
        n[i] = len(v)
    return out, n
