"""Writes tests/golden/rect_restatement_pins.json: the SHA-256 of what the numpy restatement of the rectification contract
(tests/rect_ref.py, DESIGN.md section 8 "Rectification") gives on its cases - iR, both float maps, the fixed-point coordinates and the gray and BGR
outputs of one raw pair, per case and side.  tests/test_rect_cpu.py checks the restatement against this file, so a change to the
restatement shows up as a change to this file.
    python tools/make_rect_pins.py            (no GPU needed)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rect_ref  # noqa: E402

if __name__ == "__main__":
    path = os.path.join(ROOT, "tests", "golden", "rect_restatement_pins.json")
    with open(path, "w") as f:
        json.dump(rect_ref.pins(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)
