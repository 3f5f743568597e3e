#!/usr/bin/env python3
"""make_bow_pins.py - counts and digests of the twin's results on the named cases of tests/bow_cases.py, for
tests/golden/bow_restatement_pins.json (tests/test_bow_cpu.py compares: a change of the twin or of a case shows there).

    python tools/make_bow_pins.py > tests/golden/bow_restatement_pins.json"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(a.tobytes())
    return h.hexdigest()[:32]


def pins():
    import bow_cases as Cs
    import bow_ref as R
    out = {}
    named = {"walk_k3_L3": Cs.walk_random(3, 3), "walk_k10_L6": Cs.walk_random(10, 6, 0.6), "walk_k20_L3": Cs.walk_random(20, 3),
             "ties_first": Cs.walk_ties("first"), "ties_last": Cs.walk_ties("last"), "ties_all": Cs.walk_ties("all"),
             "ragged": Cs.walk_ragged(False), "ragged_interleaved": Cs.walk_ragged(True), "repeat500": Cs.vec_repeat500(),
             "all_different": Cs.vec_all_different(), "all_stopped": Cs.vec_all_stopped(), "stop_mixed": Cs.vec_stop_mixed(),
             "norm_order": Cs.vec_norm_order()}
    for name, c in named.items():
        w, vec, fv = R.transform(c["voc"], c["descs"], 1)
        out[name] = dict(c["voc"].describe(), features=len(w), stopped=int((w < 0).sum()), entries=len(vec), pairs=len(fv),
                         vocabulary=digest(c["voc"].parent, c["voc"].desc, c["voc"].weight), result=digest(w, vec, fv))
    s = Cs.score_sets()
    out["scores"] = dict(a=len(s["A"]), b=len(s["B"]), result=digest(R.scores(s["A"], s["B"])))
    q = Cs.query_db()
    n = len(q["vecs"])
    cand, cnt = R.query(q["vecs"], n - 4, 4, 3, -1.0, 16)
    out["query"] = dict(frames=n, candidates=[int(x) for x in cnt], result=digest(cand, cnt))
    tiny = Cs.tiny()
    out["tiny"] = dict(tiny.describe(), text=hashlib.sha256(R.format_text(tiny).encode()).hexdigest()[:32])
    return out


if __name__ == "__main__":
    print(json.dumps(pins(), indent=1, sort_keys=True))
