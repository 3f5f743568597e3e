"""Inputs of the MODE_HH suites of the semi-global block matcher: stage cases reused by name from tests/sgbm_cases.py (gray) and
tests/sgbm_bgr_cases.py (colour), the eight-direction restatement tests/sgbm_hh_ref.py of each computed once per session, and
the hashes that pin it (tests/golden/sgbm_hh_restatement_pins.json).

These are the smallest cases at which the mode's code can go wrong:

  gray    minimal25x2d16     H = 2: every reverse path has one predecessor row
          noise83x37         general D = 16 case
          portrait41x90d16   H > W - D: bottom-up diagonals enter at the side columns
          noise120x30d32     D = 32
          urban200x26        D = 48: groups of 64 with idle lanes
          noise150x20d64     D = 64
          saturated120x30    the second pass's sum of three directions passes int16
          bars64x8s29        tied bids on the right-image columns
          binary64x8s5348    winners at both ends of the disparity range
  colour  minimal25x2d16     smallest admitted size
          wrap80x12d16       carried steps wrap in every new direction
          noise120x24d48     D = 48
          portrait28x60d16   H > W - D
          replicated64x20d16 low-side saturation of sum8
"""
import hashlib
import json
import os

import numpy as np

import sgbm_bgr_cases
import sgbm_cases
import sgbm_hh_ref

GRAY_CASES = ("minimal25x2d16", "noise83x37", "portrait41x90d16", "noise120x30d32", "urban200x26", "noise150x20d64",
              "saturated120x30", "bars64x8s29", "binary64x8s5348")
BGR_CASES = ("minimal25x2d16", "wrap80x12d16", "noise120x24d48", "portrait28x60d16", "replicated64x20d16")
WRAP_CASE, GRAY_REPLICATED_CASE = sgbm_bgr_cases.WRAP_CASE, sgbm_bgr_cases.GRAY_CASE
PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sgbm_hh_restatement_pins.json")

_refs = {}


def ref(name):
    """(L, R, D, MODE_HH restatement) of a gray case, computed once per session and never modified."""
    key = ("gray", name)
    if key not in _refs:
        L, R, D = sgbm_cases.case(name)
        _refs[key] = (L, R, D, sgbm_hh_ref.sgbm_hh(L, R, D))
    return _refs[key]


def ref_bgr(name):
    """(L, R, D, MODE_HH restatement) of a colour case (L and R are H x W x 3 uint8)."""
    key = ("bgr", name)
    if key not in _refs:
        L, R, D = sgbm_bgr_cases.case(name)
        _refs[key] = (L, R, D, sgbm_hh_ref.sgbm_hh_bgr(L, R, D))
    return _refs[key]


def stage_hashes(out):
    """sha256 of every stage of a restatement, made the way sgbm_bgr_cases.stage_hashes makes them (a gray restatement has no
    Ctrue)."""
    return {k: hashlib.sha256(np.ascontiguousarray(out[k]).astype(out[k].dtype.newbyteorder("<")).tobytes()).hexdigest()
            for k in sgbm_bgr_cases.STAGE_KEYS if k in out}


def all_hashes():
    pins = {"gray/" + name: stage_hashes(ref(name)[3]) for name in GRAY_CASES}
    pins.update({"bgr/" + name: stage_hashes(ref_bgr(name)[3]) for name in BGR_CASES})
    return pins


if __name__ == "__main__":      # prints the pins file
    print(json.dumps(all_hashes(), indent=1, sort_keys=True))
