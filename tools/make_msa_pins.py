#!/usr/bin/env python3
"""make_msa_pins.py - counts and digests of the twin's results (tests/msa_ref.py) on the named cases of tests/msa_cases.py, for
tests/golden/msa_restatement_pins.json (tests/test_msa_cpu.py compares: a change of the twin or of a case shows there).

    python tools/make_msa_pins.py > tests/golden/msa_restatement_pins.json

The whole-solve cases need the product's host-side tree builder (svo_msa_tree), so the library must be built; no GPU."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(a.tobytes())
    return h.hexdigest()


def pins():
    import msa_cases as Cs
    import msa_ref as R
    out = {}
    for name, c in Cs.tree_cases().items():
        out["tree/" + name] = dict(nodes=c.N, D=c.D, levels=c.levels, maxw=c.maxw, max_children=c.max_children, lds=c.lds, bfs=c.expect_bfs,
                                   tree=digest(c.seq, c.cp, c.ch, c.cc, c.cost),
                                   result=digest(*[R.tree_dp(*c.args(), R.exp_table(o)) for o in c.os]))
    for W, H in Cs.INIT_SIZES:
        for disp in Cs.INIT_DISPS:
            o = Cs.init_twin(W, H, disp)
            out["init/%dx%d_disp%d" % (W, H, disp)] = dict(pair=digest(*Cs.init_pair(W, H)), result=digest(*[o[k] for k in sorted(o)]))
    for W, H in Cs.WTA_SIZES:
        A, kind = Cs.wta_volume(W, H)
        out["wta/%dx%d" % (W, H)] = dict(kinds=np_counts(kind), result=digest(R.wta(A, H, W)))
    for W in (256, 257):
        d1, d2, named = Cs.lr_maps(W)
        vol, mask = R.lrcheck(d1, d2, 256)
        out["lrcheck/w%d" % W] = dict(named=len(named), stable=int(mask.sum()), result=digest(vol, mask))
    for shape in Cs.CTMF_SHAPES:
        a = Cs.ctmf_image(shape)
        out["ctmf/" + "x".join(map(str, shape))] = dict(result=digest(*[R.median_clamped(a, r) for r in (1, 2)]))
    for name, W, H, d, shift, scales, bfs in Cs.SOLVE_CASES:
        s = Cs.solved(name)
        out["solve/" + name] = dict(stable=int(s["mask"].sum()), nonzero=int((s["disp0"] != 0).sum()), bfs=bfs,
                                    result=digest(*[s[k] for k in sorted(s) if k != "out" and hasattr(s[k], "tobytes")], *[R.output(s["disp0"], sc) for sc in scales]))
    for d in (255, 0):
        out["batch/d%d" % d] = dict(result=digest(*Cs.batch_twin_maps(d)))
    return out


def np_counts(a):
    import numpy as np
    return [int(x) for x in np.bincount(a.reshape(-1))]


if __name__ == "__main__":
    print(json.dumps(pins(), indent=1, sort_keys=True))
