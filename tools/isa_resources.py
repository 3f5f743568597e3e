#!/usr/bin/env python3
"""Per-kernel resources and mnemonic histogram of translation units, for comparing two trees kernel by kernel.

    python tools/isa_resources.py [--root OTHER_TREE] [--diff OTHER_LISTING] unit.hip ... > listing.txt

Every named `csrc/` unit of the tree (this one, or `--root`) is compiled to gfx950 assembly with `tools/isa_mix.py`'s flags (the
library's own) and split per kernel with its `kernels_of`.  Per kernel three lines: the ISA metadata (VGPRs, AGPRs, SGPRs, spill
counts, private segment, static LDS, code bytes), the `.amdhsa_` directives behind it, and the count of every mnemonic.
`--diff` compares against a listing made earlier (another tree's): kernels whose metadata or histogram differ, with the difference.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

import isa_mix

INFO = ["codeLenInByte", "TotalNumSgprs", "NumVgprs", "NumAgprs", "TotalNumVgprs", "ScratchSize", "LDSByteSize", "Occupancy"]
DIRECTIVES = ["next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size", "group_segment_fixed_size"]


def listing(root, units):
    out = []
    with tempfile.TemporaryDirectory() as td:
        for u in units:
            s = os.path.join(td, u + ".s")
            subprocess.check_call(["/opt/rocm/bin/hipcc"] + isa_mix.FLAGS + ["-o", s, os.path.join(root, "stereo-semantic-vo_amd", "csrc", u)],
                                  stderr=subprocess.DEVNULL)
            txt = open(s).read()
            direct, info, cur = {}, {}, None
            for m in re.finditer(r"\.amdhsa_kernel\s+(\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
                direct[m.group(1)] = {k: v for k in DIRECTIVES for v in re.findall(r"\.amdhsa_%s\s+(\S+)" % k, m.group(2))[:1]}
            for line in txt.splitlines():      # the "; Kernel info:" comment block behind each kernel
                m = re.match(r"^([A-Za-z_][\w$.]*):", line)
                if m and m.group(1) in direct:
                    cur = m.group(1)
                    info[cur] = {}
                m = re.match(r"^; (\w+):? =? ?(\d+)", line)
                if m and cur and m.group(1) in INFO:
                    info[cur].setdefault(m.group(1), m.group(2))
            for blk in re.split(r"\n  - \.agpr_count", txt)[1:]:      # the code object's metadata: spill counts
                name = re.search(r"\.symbol:\s+(\S+)\.kd", blk).group(1)
                for k in ("sgpr_spill_count", "vgpr_spill_count"):
                    info[name][k] = re.search(r"\.%s:\s+(\d+)" % k, blk).group(1)
            for name, body in isa_mix.kernels_of(txt):
                hist = collections.Counter(l.split()[0] for l in body)
                out.append("%s  [%s]" % (isa_mix.demangle(name), u))
                out.append("  " + "  ".join("%s=%s" % kv for kv in info[name].items()))
                out.append("  " + "  ".join("%s=%s" % kv for kv in direct[name].items()))
                out.append("  instructions=%d  " % len(body) + " ".join("%s:%d" % kv for kv in sorted(hist.items())))
    return out


def parse(lines):
    return {lines[i]: lines[i + 1:i + 4] for i in range(0, len(lines) - 3, 4)}


def diff(ours, theirs):
    for k, a in parse(theirs).items():
        b = parse(ours).get(k)
        if b is None:
            print("%s: not in this tree" % k)
            continue
        meta = lambda r: [re.sub(r"codeLenInByte=\d+\s+", "", r[0]), r[1]]
        ha, hb = (dict(x.rsplit(":", 1) for x in r[2].split()[1:]) for r in (a, b))
        d = {m: int(hb.get(m, 0)) - int(ha.get(m, 0)) for m in sorted(set(ha) | set(hb)) if ha.get(m, 0) != hb.get(m, 0)}
        if meta(a) == meta(b) and not d:
            continue
        print("%s: metadata %s; histogram %s" % (k, "equal" if meta(a) == meta(b) else "DIFFERS", " ".join("%s%+d" % kv for kv in d.items()) or "equal"))
        if meta(a) != meta(b):
            print("    other: %s\n    this:  %s" % (" | ".join(meta(a)), " | ".join(meta(b))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=isa_mix.ROOT)
    ap.add_argument("--diff")
    ap.add_argument("units", nargs="+")
    a = ap.parse_args()
    lines = listing(a.root, a.units)
    if a.diff:
        diff(lines, [l.rstrip("\n") for l in open(a.diff) if not l.startswith("#")])
    else:
        sys.stdout.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
