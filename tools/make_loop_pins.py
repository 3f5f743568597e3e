#!/usr/bin/env python3
"""make_loop_pins.py - what tests/test_loop_cpu.py pins of the twin of loop verification (tests/loop_ref.py), for
tests/golden/loop_restatement_pins.json: the sigma2 table, the first samples, the measured worst difference between the twin's Horn
and a Kabsch solve through numpy.linalg.svd, and digests of the twin's results on named cases of tests/loop_cases.py (a change of
the twin or of a case shows there).

    python tools/make_loop_pins.py > tests/golden/loop_restatement_pins.json"""
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


def case_pins():
    import loop_cases as Cs
    import loop_ref as R
    out = {}
    for name, c in (("planted", Cs.planted(1)), ("root500", Cs.root(2, 500))):
        m, mn, res, inl = R.verify(c["scene"], c["pairs"], Cs.CAM, c["P"])
        out[name] = dict(matches=int(mn[0]), status=int(res[0]["status"]), inliers=int(res[0]["n_inliers"]), result=digest(m, mn, res, inl))
    for name, c in (("solve500", Cs.solve_case(7, 500, n_out=150)), ("refit", Cs.solve_case(13, 120, n_out=50, P=R.params(refine=1))),
                    ("winner_last", Cs.winner_last()), ("rejected_equal", Cs.rejected_equal())):
        r, inl, _ = Cs.run_solve(c)
        out[name] = dict(status=int(r["status"]), winner=int(r["winner"]), inliers=int(r["n_inliers"]), seed=int(c["P"]["seed"]),
                         result=digest(r, inl))
    return out


def pins():
    import loop_ref as R
    import test_loop_cpu as T
    return {"sigma2_scale_1.2": R.sigma2_table(1.2),
            "samples_seed_default_N20": [R.sample(R.PARAMS["seed"], i, 20) for i in range(4)],
            "horn_vs_kabsch_worst": float(T.horn_vs_kabsch()),
            "horn_vs_kabsch_note": "max |R - R_svd|, |t - t_svd| over 200 seeded sets (3 points, spread; 4 .. 59 points); the test allows 10 x",
            "cases": case_pins()}


if __name__ == "__main__":
    print(json.dumps(pins(), indent=1, sort_keys=True))
