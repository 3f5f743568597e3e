"""Pins of the Lucas-Kanade restatement (tests/lk_ref.py), the oracle of both GPU suites: SHA-256 digests of the raw bytes of
every array it returns - next points, status, err, exits, iterations, for colour the window sums and their level, every level
image and derivative plane of both frames - on the inputs the GPU suites compare the device against.  The digests in
tests/golden/lk_restatement_pins.json were recorded once, from the two separate restatements (gray and colour) that stood
before they were merged into one; this test only reads them.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import lk_bgr_cases
import lk_cases
import lk_ref
import test_lk_bgr_gpu as colour_suite
import test_lk_gpu as gray_suite

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lk_restatement_pins.json")
RESULT_KEYS = ("next_pts", "status", "err", "exits", "iterations", "sums", "sums_level")
PLANE_KEYS = ("levels_prev", "derivs_prev", "levels_next", "derivs_next")


def _digest(a):
    a = np.ascontiguousarray(a)
    return "%s%s:%s" % (a.dtype, list(a.shape), hashlib.sha256(a.tobytes()).hexdigest())


def _of_result(out):
    d = {k: _digest(out[k]) for k in RESULT_KEYS if k in out}
    d["top"] = out["top"]
    for k in PLANE_KEYS:
        for level, a in enumerate(out[k]):
            d["%s/%d" % (k, level)] = _digest(a)
    return d


def _of_stage(mod, prev, nxt):
    planes = dict(zip(PLANE_KEYS, mod.build_pyramid(prev) + mod.build_pyramid(nxt)))
    return {"%s/%d" % (k, level): _digest(a) for k in PLANE_KEYS for level, a in enumerate(planes[k])}


def _faint():
    prev, nxt = lk_bgr_cases.faint_pair()
    pts = np.concatenate([[lk_bgr_cases.SPLIT_POINT], lk_cases.inner_grid(64, 64, 12, 8)]).astype(np.float32)
    return prev, nxt, pts


def _faint_replicated():
    prev, nxt, pts = _faint()
    return lk_bgr_cases.replicate(prev), lk_bgr_cases.replicate(nxt), pts


def _iso_as_gray():
    prev, nxt = lk_bgr_cases.isoluminant_pair()
    return lk_bgr_cases.gray_of(prev), lk_bgr_cases.gray_of(nxt), lk_cases.inner_grid(*lk_bgr_cases.ISO_SIZE)


def cases(gray, colour):
    """{pin name: function returning its digests}, `gray` and `colour` the modules that restate the two contracts (here the same
    one; when the pins were recorded, the two modules of that time)."""
    c = {}
    for kind, suite, mod in (("gray", gray_suite, gray), ("colour", colour_suite, colour)):
        for name in suite.STAGE_CASES:
            c["%s/stage/%s" % (kind, name)] = lambda suite=suite, mod=mod, name=name: _of_stage(mod, *suite._stage_case(name))
        for name in suite.RESULT_CASES:
            c["%s/result/%s" % (kind, name)] = lambda suite=suite, mod=mod, name=name: _of_result(mod.track(*suite._result_case(name)))

        def level0(suite=suite, mod=mod):
            prev, nxt, pts = suite._result_case("planted120x50")
            return _of_result(mod.track(prev, nxt, pts[:16], max_level=0))
        c["%s/max_level0/planted120x50" % kind] = level0
    c["gray/faint64x64"] = lambda: _of_result(gray.track(*_faint()))
    c["colour/faint64x64_replicated"] = lambda: _of_result(colour.track(*_faint_replicated()))
    c["gray/isoluminant200x180_as_gray"] = lambda: _of_result(gray.track(*_iso_as_gray()))
    return c


CASES = cases(lk_ref, lk_ref)


def test_the_pin_file_names_exactly_these_cases():
    with open(PINS) as f:
        assert sorted(json.load(f)) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_restatement_returns_the_pinned_bytes(name):
    with open(PINS) as f:
        want = json.load(f)[name]
    got = CASES[name]()
    assert set(want) <= set(got), sorted(set(want) - set(got))
    bad = [k for k in sorted(want) if got[k] != want[k]]
    assert not bad, (name, bad[:4], [got[k] for k in bad[:2]], [want[k] for k in bad[:2]])
