"""Writes tests/golden/pnp_rule_margins.json: over all pairs 5 <= g <= n, 6 <= n <= 512 of RANSACUpdateNumIters(0.99, (n - g) / n, 5, .),
the closest the quotient log(0.01) / log(1 - (g / n)^5) - evaluated with 200 bits - comes to a tie of its rounding and to an integer
bound 1 .. 100 of the comparison in front of it, relative to the quotient, with the arguments (tests/pnp_rule_ref.py margin_study;
tests/test_pnp_rule_cpu.py recomputes and compares).  Needs mpmath, no GPU:  python tools/make_pnp_rule_margins.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pnp_rule_ref as ref


def main():
    s = ref.margin_study()
    out = {"pairs": int(len(s["g"])), "pairs_with_g_equal_n": int((s["g"] == s["n"]).sum()),
           "tie": {"relative_margin": s["tie"][0], "at": list(s["tie"][1])},
           "cmp": {"relative_margin": s["cmp"][0], "at": list(s["cmp"][1])}}
    with open(ref.MARGINS_PATH, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
