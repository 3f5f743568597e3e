"""numpy twin of the bag-of-words contract (DESIGN.md section 8 "Bag of words"): DBoW2's vocabulary tree, text format, word walk,
BowVector / FeatureVector, L1 score, the query's selection and the training, restated from the reference's Thirdparty/DBoW2.

Every rule the contract fixes is a switch of `Rules`, so a test can show that a case tells the rule from its neighbour (the
mutant table of tests/test_bow_cpu.py).  The defaults are the contract."""
import math

import numpy as np

TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3

ENTRY = np.dtype([("word", "<u4"), ("reserved", "<u4"), ("value", "<f8")])
FEATURE = np.dtype([("node", "<u4"), ("feature", "<u4")])
CAND = np.dtype([("frame", "<i4"), ("reserved", "<i4"), ("score", "<f8")])

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


class Rules:
    """The contract's rules; each keyword names the neighbour a mutant takes instead."""

    def __init__(self, **kw):
        self.tie_last = False          # `<=` in the walk and the assignment: a tie goes to the last child
        self.multiply = False          # c * w instead of w added c times
        self.norm_feature_order = False   # the norm summed in the order the words first occur
        self.keep_stop = False         # stop words (weight not > 0) kept
        self.add_always = False        # addWeight where addIfNotExist belongs (IDF, BINARY)
        self.levelsup_off = 0          # nid taken at level L - levelsup + this
        self.majority_half = False     # n / 2 instead of n / 2 + n % 2
        self.drop_zero_sign = False    # 0.0 where the score is -0.0
        self.cand_desc_j = False       # equal scores by descending frame
        self.gap_off = 0               # frames 0 .. q - gap - 1 + this
        for k, v in kw.items():
            if not hasattr(self, k):
                raise TypeError("no rule %r" % k)
            setattr(self, k, v)


CONTRACT = Rules()


class Voc:
    """A tree by node id: node 0 is the root.  parent (n,), desc (n, 32) uint8, weight (n,) float64; children and word ids follow."""

    def __init__(self, k, L, weighting, parent, desc, weight, scoring=0):
        self.k, self.L, self.weighting, self.scoring = int(k), int(L), int(weighting), int(scoring)
        self.parent = np.asarray(parent, np.int32).copy()
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32).copy()
        self.weight = np.asarray(weight, np.float64).copy()
        n = len(self.parent)
        self.parent[0] = -1
        self.children = [[] for _ in range(n)]
        for i in range(1, n):
            p = int(self.parent[i])
            if not 0 <= p < i:
                raise ValueError("node %d: parent %d is not defined yet" % (i, p))
            self.children[p].append(i)
        self.word = np.full(n, -1, np.int32)      # createWords (TemplatedVocabulary.h:901-921): the leaves in node-id order
        w = 0
        for i in range(1, n):
            if not self.children[i]:
                self.word[i] = w
                w += 1
        self.n_words = w
        self.word_node = np.flatnonzero(self.word >= 0).astype(np.int32)

    def describe(self):
        return dict(k=self.k, L=self.L, nodes=len(self.parent), words=self.n_words, weighting=self.weighting)

    def level(self, node):
        lv = 0
        while node != 0:
            node = int(self.parent[node])
            lv += 1
        return lv


# ---- text format (TemplatedVocabulary.h:1338-1449) ---------------------------------------------------------------------------
def parse_text(text):
    """loadFromTextFile, with the contract's refusals (ValueError naming the line)."""
    lines = text.split("\n")
    header = None
    parent, desc, weight, leaf = [-1], [np.zeros(32, np.uint8)], [0.0], [False]
    line0 = None
    for no, s in enumerate(lines, 1):
        if not s.strip():
            continue
        tok = s.split()
        if header is None:
            if len(tok) != 4:
                raise ValueError("line %d: the header is `k L scoring weighting`" % no)
            k, L, scoring, weighting = (int(t) for t in tok)
            if not 2 <= k <= 20:
                raise ValueError("line %d: k must be 2 .. 20" % no)
            if not 1 <= L <= 10:
                raise ValueError("line %d: L must be 1 .. 10" % no)
            if scoring != 0:
                raise ValueError("line %d: scoring must be 0 (L1_NORM)" % no)
            if not 0 <= weighting <= 3:
                raise ValueError("line %d: weighting must be 0 .. 3" % no)
            header = (k, L, weighting)
            continue
        if line0 is None:
            line0 = no
        if len(tok) != 35:
            raise ValueError("line %d: a node is `parent is_leaf b0 .. b31 weight`" % no)
        p = int(tok[0])
        if not 0 <= p < len(parent):
            raise ValueError("line %d: parent %d is not defined yet" % (no, p))
        b = [int(t) for t in tok[2:34]]
        if min(b) < 0 or max(b) > 255:
            raise ValueError("line %d: a descriptor byte must be 0 .. 255" % no)
        parent.append(p)
        leaf.append(int(tok[1]) > 0)
        desc.append(np.array(b, np.uint8))
        weight.append(float(tok[34]))
    if header is None:
        raise ValueError("line 1: the header is `k L scoring weighting`")
    if len(parent) < 2:
        raise ValueError("a vocabulary needs the root and at least one node")
    v = Voc(header[0], header[1], header[2], parent, np.stack(desc), weight)
    for i in range(1, len(parent)):
        ln = line0 + i - 1
        if leaf[int(v.parent[i])]:
            raise ValueError("line %d: parent %d is marked a leaf" % (ln, v.parent[i]))
    for i in range(len(parent)):
        if len(v.children[i]) > v.k:
            raise ValueError("line %d: parent %d has more than k children" % (line0 + v.children[i][v.k] - 1, i))
    for i in range(1, len(parent)):
        if not leaf[i] and not v.children[i]:
            raise ValueError("line %d: an inner node without children" % (line0 + i - 1))
    return v


def format_text(v):
    """saveToTextFile with 17 significant digits for the weights (DBoW2's stream prints 6)."""
    out = ["%d %d  %d %d" % (v.k, v.L, v.scoring, v.weighting)]
    for i in range(1, len(v.parent)):
        out.append("%d %d %s %s" % (v.parent[i], 0 if v.children[i] else 1, " ".join(str(int(b)) for b in v.desc[i]),
                                    "%.17g" % v.weight[i]))
    return "\n".join(out) + "\n"


# ---- distance, assignment, walk ------------------------------------------------------------------------------------------------
def hamming(a, b):
    """FORB::distance / pnpmatch::DescriptorDistance: differing bits of 32-byte descriptors (broadcasts over leading axes)."""
    return _POP[np.bitwise_xor(a, b)].sum(axis=-1)


def assign(desc, centres, rules=CONTRACT):
    """Each descriptor's nearest centre: strict `<` in centre order, so the earliest among equals (:736-746).  (index, distance)"""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    centres = np.asarray(centres, np.uint8).reshape(-1, 32)
    d = hamming(desc[:, None, :], centres[None, :, :]).astype(np.int32)
    if rules.tie_last:
        idx = d.shape[1] - 1 - np.argmin(d[:, ::-1], axis=1)
    else:
        idx = np.argmin(d, axis=1)
    return idx.astype(np.int32), d[np.arange(len(d)), idx].astype(np.int32)


def walk(v, d, levelsup=0, rules=CONTRACT):
    """transform(feature, id, weight, nid, levelsup) (:1218-1259) -> (word, weight, nid, path).
    nid: the node at level L - levelsup; the root when that is <= 0.  When the walk ends on a leaf above that level the reference
    never writes *nid (its caller's local keeps an indeterminate value): the contract takes the leaf."""
    nid_level = v.L - levelsup + rules.levelsup_off
    nid = 0 if nid_level <= 0 else None
    node, level, path = 0, 0, []
    while True:
        level += 1
        ch = v.children[node]
        idx, _ = assign(d, v.desc[ch], rules)
        node = ch[int(idx[0])]
        path.append(node)
        if nid is None and level == nid_level:
            nid = node
        if not v.children[node]:
            break
    if nid is None:
        nid = node
    return int(v.word[node]), float(v.weight[node]), nid, path


# ---- vectors -------------------------------------------------------------------------------------------------------------------
def transform(v, descs, levelsup=0, rules=CONTRACT):
    """transform(features, BowVector, FeatureVector, levelsup) (:1127-1194) with BowVector.cpp:34-84.
    -> (words (n,) int32 with -1 for a stopped feature, vec ENTRY, fv FEATURE)."""
    descs = np.asarray(descs, np.uint8).reshape(-1, 32)
    words = np.full(len(descs), -1, np.int32)
    bow, order, fvl = {}, [], []
    once = v.weighting in (IDF, BINARY) and not rules.add_always
    count = {}
    for i, d in enumerate(descs):
        word, w, nid, _ = walk(v, d, levelsup, rules)
        if not (w > 0) and not rules.keep_stop:
            continue
        words[i] = word
        if word not in bow:
            bow[word] = w
            order.append(word)
            count[word] = 1
        elif not once:
            bow[word] += w                      # addWeight: one double addition per occurrence, in feature order
            count[word] += 1
        fvl.append((nid, i))
    if rules.multiply:
        for word in bow:
            bow[word] = count[word] * float(v.weight[v.word_node[word]])
    norm = 0.0
    for word in (order if rules.norm_feature_order else sorted(bow)):
        norm += abs(bow[word])                  # BowVector::normalize, L1: in the map's (ascending word) order
    vec = np.zeros(len(bow), ENTRY)
    for j, word in enumerate(sorted(bow)):
        vec[j] = (word, 0, bow[word] / norm if norm > 0.0 else bow[word])
    fv = np.zeros(len(fvl), FEATURE)
    for j, (nid, i) in enumerate(sorted(fvl)):
        fv[j] = (nid, i)
    return words, vec, fv


def score(a, b, rules=CONTRACT):
    """L1Scoring::score (ScoringObject.cpp:23-68): vi from a, wi from b, the common words in ascending order."""
    s = 0.0
    wb = {int(w): float(x) for w, x in zip(b["word"], b["value"])}
    for w, vi in zip(a["word"], a["value"]):
        wi = wb.get(int(w))
        if wi is not None:
            vi = float(vi)
            s += abs(vi - wi) - abs(vi) - abs(wi)
    s = -s / 2.0
    if rules.drop_zero_sign and s == 0.0:
        s = 0.0
    return s


def scores(vecs_a, vecs_b, rules=CONTRACT):
    return np.array([[score(a, b, rules) for b in vecs_b] for a in vecs_a], np.float64).reshape(len(vecs_a), len(vecs_b))


def select(row, q, gap, min_score, top_k, rules=CONTRACT):
    """The query's selection from a query's scores against every frame: frames 0 .. q - gap - 1 with score > min_score, by
    descending score, equal scores by ascending frame.  -> (cand (top_k,) CAND, count)"""
    last = q - gap + rules.gap_off
    c = [(float(row[j]), j) for j in range(max(last, 0)) if row[j] > min_score]
    c.sort(key=lambda t: (-t[0], -t[1] if rules.cand_desc_j else t[1]))
    c = c[:top_k]
    out = np.zeros(top_k, CAND)
    out["frame"] = -1
    for i, (s, j) in enumerate(c):
        out[i] = (j, 0, s)
    return out, len(c)


def query(vecs, q0, Q, gap, min_score, top_k, rules=CONTRACT):
    cand = np.zeros((Q, top_k), CAND)
    cnt = np.zeros(Q, np.int32)
    for i in range(Q):
        q = q0 + i
        row = np.array([score(vecs[q], vecs[j], rules) for j in range(q)], np.float64)
        cand[i], cnt[i] = select(row, q, gap, min_score, top_k, rules)
    return cand, cnt


# ---- training (create / HKmeansStep / initiateClustersKMpp / FORB::meanValue / setNodeWeights, :558-996, FORB.cpp:28-77) ----------
def mean_value(descs, rules=CONTRACT):
    """FORB::meanValue: of one descriptor, that descriptor; otherwise bit j is set when at least N2 = n / 2 + n % 2 have it."""
    descs = np.asarray(descs, np.uint8).reshape(-1, 32)
    n = len(descs)
    if n == 1:
        return descs[0].copy()
    s = np.unpackbits(descs, axis=1).astype(np.int64).sum(axis=0)
    n2 = n // 2 + (0 if rules.majority_half else n % 2)
    return np.packbits(s >= n2)


def _kmpp(descs, k, rng, assign_fn):
    """initiateClustersKMpp (:829-897).  The one departure: the draws come from `rng` (a seeded numpy Generator), not rand()."""
    n = len(descs)
    centres = [descs[int(rng.integers(0, n))].copy()]
    min_d = assign_fn(descs, centres[-1][None])[1].astype(np.float64)
    while len(centres) < k:
        if len(centres) > 1:
            d = assign_fn(descs, centres[-1][None])[1].astype(np.float64)
            upd = (min_d > 0) & (d < min_d)
            min_d[upd] = d[upd]
        total = float(min_d.sum())          # std::accumulate over whole numbers below 2^53: exact in any order
        if not total > 0:
            break
        while True:
            cut = float(rng.uniform(0.0, total))
            if cut != 0.0:
                break
        cum = np.cumsum(min_d)
        hit = np.flatnonzero(cum >= cut)
        centres.append(descs[int(hit[0]) if len(hit) else n - 1].copy())
    return np.stack(centres)


def train(docs, k, L, weighting, seed, assign_fn=None, rules=CONTRACT):
    """create(training_features, k, L, weighting, L1_NORM).  docs: a list of (n_i, 32) uint8 arrays, one per document.
    assign_fn(descs, centres) -> (index, distance): the assignment step (the twin's `assign`, or the device's)."""
    if assign_fn is None:
        def assign_fn(d, c):
            return assign(d, c, rules)
    rng = np.random.Generator(np.random.PCG64(seed))
    feats = np.concatenate([np.asarray(d, np.uint8).reshape(-1, 32) for d in docs])
    parent, desc = [-1], [np.zeros(32, np.uint8)]
    leaf_of = np.zeros(len(feats), np.int64)   # per training feature the leaf its group became (a probe for the tests)

    def step(parent_id, idxs, level):
        n = len(idxs)
        if n == 0:
            return
        sub = feats[idxs]
        if n <= k:                           # the trivial case: one cluster per feature
            centres = sub.copy()
            groups = [[i] for i in range(n)]
        else:
            centres = _kmpp(sub, k, rng, assign_fn)
            last = None
            while True:
                cur = assign_fn(sub, centres)[0]
                groups = [np.flatnonzero(cur == c) for c in range(len(centres))]
                if last is not None and np.array_equal(cur, last):
                    break
                last = cur
                # a cluster that lost its features keeps its centre (the reference's mean of none is an empty matrix)
                centres = np.stack([mean_value(sub[g], rules) if len(g) else centres[c] for c, g in enumerate(groups)])
        ids = []
        for c in centres:
            ids.append(len(parent))
            parent.append(parent_id)
            desc.append(c)
        for nid, g in zip(ids, groups):
            if level < L and len(g) > 1:     # a child holding one feature stays a leaf
                step(nid, idxs[np.asarray(g)], level + 1)
            else:
                leaf_of[idxs[np.asarray(g, np.int64)]] = nid

    step(0, np.arange(len(feats)), 1)
    v = Voc(k, L, weighting, parent, np.stack(desc), np.zeros(len(parent)))
    v.train_leaf = leaf_of
    if weighting in (TF, BINARY):
        v.weight[v.word_node] = 1.0
    else:                                    # setNodeWeights: Ni counts a word once per document
        ni = np.zeros(v.n_words, np.int64)
        words = leaf_words(v, feats, assign_fn)
        at = 0
        for d in docs:
            ni[np.unique(words[at:at + len(d)])] += 1
            at += len(d)
        for w in range(v.n_words):
            if ni[w] > 0:
                v.weight[v.word_node[w]] = math.log(float(len(docs)) / float(ni[w]))
    return v


def leaf_words(v, descs, assign_fn=None):
    """The word of every descriptor, stop words included: the walk level by level over all descriptors at once."""
    if assign_fn is None:
        assign_fn = assign
    descs = np.asarray(descs, np.uint8).reshape(-1, 32)
    node = np.zeros(len(descs), np.int64)
    active = np.arange(len(descs))
    inner = np.array([len(c) > 0 for c in v.children], bool)
    while len(active):
        cur = node[active]
        for p in np.unique(cur):
            sel = active[cur == p]
            ch = np.asarray(v.children[int(p)])
            node[sel] = ch[assign_fn(descs[sel], v.desc[ch])[0]]
        active = active[inner[node[active]]]
    return v.word[node].astype(np.int32)


# ---- seeded material for the cases -----------------------------------------------------------------------------------------------
def random_tree(seed, k, L, weighting=TF_IDF, ragged=0.0, shuffle_ids=False, stop=0.0):
    """A random vocabulary: every inner node has k children (fewer, and early leaves, with probability `ragged`), random centres,
    weights ln(N / Ni) of random counts (0.0 with probability `stop`: ln(N / N)).  shuffle_ids: node ids interleave siblings."""
    rng = np.random.default_rng(seed)
    nodes = [(-1, 0)]                         # (parent, level)
    frontier = [0]
    while frontier:                           # breadth first
        nxt = []
        for p in frontier:
            lv = nodes[p][1]
            nc = k if rng.random() >= ragged else int(rng.integers(1, k + 1))
            for _ in range(nc):
                nodes.append((p, lv + 1))
                if lv + 1 < L and not (ragged and rng.random() < ragged):
                    nxt.append(len(nodes) - 1)
        frontier = nxt
    n = len(nodes)
    parent = np.array([p for p, _ in nodes], np.int32)
    if shuffle_ids:                           # renumber so that siblings' ids interleave, parents still first
        level = np.array([lv for _, lv in nodes])
        key = level * 1.0 + rng.random(n) * 0.999
        order = np.argsort(key, kind="stable")
        new = np.empty(n, np.int64)
        new[order] = np.arange(n)
        parent2 = np.full(n, -1, np.int32)
        for old in range(1, n):
            parent2[new[old]] = new[parent[old]]
        parent = parent2
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for i in range(1, n):                     # below level 1 a centre is its parent's with 40 / level bits turned: walks go deep
        lv, p = 1, int(parent[i])
        while parent[p] >= 0:
            lv, p = lv + 1, int(parent[p])
        if lv > 1:
            desc[i] = desc[parent[i]]
            for b in rng.integers(0, 256, 40 // lv):
                desc[i, b >> 3] ^= np.uint8(1 << (b & 7))
    v = Voc(k, L, weighting, parent, desc, np.zeros(n))
    for node in v.word_node:
        if weighting in (TF, BINARY):
            w = 1.0
        else:
            w = math.log(50.0 / float(rng.integers(1, 50)))
        if stop and rng.random() < stop:
            w = 0.0
        v.weight[node] = w
    return v
