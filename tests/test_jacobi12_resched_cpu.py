"""The M = 12 step loop with its step body rescheduled around the dependent chain (EO_JACOBI_ASM_12 of tools/gen_jacobi_asm.py) against
the block it replaces (EO_JACOBI_ASM_12_PREV), without a GPU: a wave64 interpreter of the mnemonics the two blocks use runs both on
every matrix of tests/golden/jacobi12_cases.npy (tools/make_jacobi12_cases.py) and on 20 seeded random M^T M; the committed state - the
lane's row x0..x2, chg, flag, the exchange area in LDS - and the number of steps must be bit-equal.

What the interpreter is: float64 multiply and add are IEEE (numpy); v_fma_f64 is a compensated product-and-sum (two-product, two-sum:
the exact result in all but double-rounding cases, deterministic); v_rcp_f64 / v_rsq_f64 are 1 / x and 1 / sqrt(x) - stand-ins, both
blocks go through the same ones, the comparison is between the blocks, not with the device; the 4x4x4 DMFMA with A = 1.0 is the
ordered sum ((((C + b0) + b1) + b2) + b3) over the four lane groups.  LDS reads are checked against the block's own s_waitcnt: a
register an outstanding ds_read will fill must not be read before the wait."""
import functools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

FULL = (1 << 64) - 1
LANES = np.arange(64, dtype=np.uint64)
XCH, TAB = 0, 2048            # LDS byte addresses: the exchange [16 rows][4 lane groups][4 doubles], the 12-row schedule table
EPS = 2.220446049250313e-16 * 10
EPS2 = EPS * EPS
OPERANDS = {"x0": "v[0:1]", "x1": "v[2:3]", "x2": "v[4:5]", "chg": "v6", "flag": "v7", "tper": "v8", "lane": "v9", "base": "v10", "act": "v11",
            "pm": "v12", "eps": "v[14:15]", "eps2hi": "v[16:17]", "eps2lo": "v[18:19]", "amine": "v20", "axch": "v21"}


@pytest.fixture(scope="module")
def gen():
    env = {k: os.environ.pop(k) for k in ("JACOBI_LOOP_ALIGN", "JACOBI_LOOP_NOPS", "JACOBI12_ITEMS") if k in os.environ}   # default settings
    try:
        import gen_jacobi_asm
    finally:
        os.environ.update(env)
    return gen_jacobi_asm


@pytest.fixture(scope="module")
def cases():
    return np.load(os.path.join(ROOT, "tests", "golden", "jacobi12_cases.npy"))


# ---- arithmetic ------------------------------------------------------------------------------------------------------------
def _split(a):
    t = a * 134217729.0
    hi = t - (t - a)
    return hi, a - hi


def fma(a, b, c):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    s = p + c
    bb = s - p
    t = (p - (s - bb)) + (c - bb)
    return s + (t + e)


def to_mask(b):
    return int((b.astype(np.uint64) << LANES).sum())


def to_lanes(m):
    return ((np.uint64(m) >> LANES) & np.uint64(1)).astype(bool)


# ---- the interpreter ---------------------------------------------------------------------------------------------------------
class Wave:
    def __init__(self, lines):
        self.lines = [re.sub(r"%\[(\w+)\]", lambda m: OPERANDS[m.group(1)], l) for l in lines]
        self.label = {l[:-1]: i for i, l in enumerate(self.lines) if l.endswith(":")}
        self.prog = [self._parse(l) for l in self.lines]
        # the copy an instruction belongs to: the step t of the next L_skip_<t>_ label
        self.copy_of, t = [None] * len(self.lines), None
        for i in range(len(self.lines) - 1, -1, -1):
            m = re.match(r"L_skip_(\d+)_%=:", self.lines[i])
            if m:
                t = int(m.group(1))
            self.copy_of[i] = t

    @staticmethod
    def _parse(line):
        if line.endswith(":") or line.startswith("."):
            return None
        mn, _, rest = line.partition(" ")
        offs = {k: int(x) for k, x in re.findall(r"\b(offset\d?):(\d+)", rest)}
        rest = re.sub(r"\s+offset\d?:\d+", "", rest)
        ops = [o.strip() for o in rest.split(",")] if rest.strip() else []
        return mn, ops, offs

    # operands (parsed once per spelling)
    @staticmethod
    @functools.lru_cache(maxsize=None)
    def _vregs(op):
        m = re.search(r"v\[(\d+):(\d+)\]", op)
        if m:
            return tuple(range(int(m.group(1)), int(m.group(2)) + 1))
        m = re.fullmatch(r"-?\|?v(\d+)\|?", op)
        return (int(m.group(1)),) if m else ()

    def vregs(self, op):
        return self._vregs(op)

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def _f64op(op):
        neg = op.startswith("-")
        o = op[1:] if neg else op
        ab = o.startswith("|")
        o = o.strip("|")
        m = re.fullmatch(r"v\[(\d+):(\d+)\]", o)
        return (int(m.group(1)) if m else None, None if m else float(o), neg, ab)

    def f64(self, op):
        lo, lit, neg, ab = self._f64op(op)
        if lo is not None:
            x = (self.V[lo].astype(np.uint64) | (self.V[lo + 1].astype(np.uint64) << np.uint64(32))).view(np.float64)
        else:
            x = np.full(64, lit)
        if ab:
            x = np.abs(x)
        return -x if neg else x

    def set64(self, op, x):
        lo = int(re.fullmatch(r"v\[(\d+):(\d+)\]", op).group(1))
        b = np.ascontiguousarray(x, np.float64).view(np.uint64)
        self.setv(lo, (b & np.uint64(0xffffffff)).astype(np.uint32))
        self.setv(lo + 1, (b >> np.uint64(32)).astype(np.uint32))

    def setv(self, n, val):
        if self.exec == FULL:
            self.V[n] = val
        else:
            self.V[n] = np.where(to_lanes(self.exec), val, self.V[n])

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def _u32op(op):
        m = re.fullmatch(r"([vs])(\d+)", op)
        return (m.group(1), int(m.group(2))) if m else ("l", int(op, 0) & 0xffffffff)

    def u32(self, op):
        kind, n = self._u32op(op)
        if kind == "v":
            return self.V[n]
        return np.full(64, self.S[n] if kind == "s" else n, np.uint32)

    def s64(self, op):
        if op == "vcc":
            return self.vcc
        if op == "exec":
            return self.exec
        m = re.fullmatch(r"s\[(\d+):(\d+)\]", op)
        if m:
            lo = int(m.group(1))
            return self.S[lo] | (self.S[lo + 1] << 32)
        return int(op, 0)

    def set_s64(self, op, val):
        val &= FULL
        if op == "vcc":
            self.vcc = val
        elif op == "exec":
            self.exec = val
        else:
            lo = int(re.fullmatch(r"s\[(\d+):(\d+)\]", op).group(1))
            self.S[lo], self.S[lo + 1] = val & 0xffffffff, val >> 32

    def s32(self, op):
        m = re.fullmatch(r"s(\d+)", op)
        return self.S[int(m.group(1))] if m else int(op, 0)

    # LDS (words)
    def lds_read(self, addr, words):
        a = (addr.astype(np.int64) >> 2)
        assert np.all(addr % 4 == 0) and a.min() >= 0 and a.max() + words <= len(self.lds), "LDS read out of bounds"
        return [self.lds[a + k] for k in range(words)]

    def lds_write(self, addr, vals):
        a = (addr.astype(np.int64) >> 2)
        on = to_lanes(self.exec)
        assert a[on].size == 0 or (a[on].min() >= XCH // 4 and a[on].max() + len(vals) <= (XCH + 2048) // 4), "LDS write outside the exchange"
        for k, val in enumerate(vals):
            self.lds[a[on] + k] = val[on]

    def run(self, At, u, max_steps=2000):
        """At: the 12 x 12 matrix (row i = row i of S.jr).  Returns the committed state and the counters."""
        self.V = np.zeros((256, 64), np.uint32)
        self.S = [0] * 104
        self.vcc, self.exec, self.scc = 0, FULL, 0
        self.lds = np.zeros(4096, np.uint32)
        self.pending = set()
        lane = np.arange(64)
        r, g = lane & 15, lane >> 4
        live = r < 12
        jr = np.zeros((16, 16))
        jr[:12, :12] = At
        self.set64("v[0:1]", jr[r, g]); self.set64("v[2:3]", jr[r, 4 + g]); self.set64("v[4:5]", jr[r, 8 + g])
        xch = np.zeros((16, 4, 4))
        xch[r, g, 0], xch[r, g, 1], xch[r, g, 2] = jr[r, g], jr[r, 4 + g], jr[r, 8 + g]
        self.lds[XCH // 4:XCH // 4 + 512] = xch.reshape(-1).view(np.uint32)
        tab = np.array([[(e & ~16) | ((e & 16) << 27) for e in row] for row in u.tab], np.uint32)
        self.lds[TAB // 4:TAB // 4 + tab.size] = tab.reshape(-1)
        self.V[8] = np.where(live, TAB + 4 * (u.pro * 12 + r), TAB)                 # tper (n = 0: the table's first word)
        self.V[9] = lane
        self.V[10] = np.where(live, 0, r)                                           # base
        self.V[11] = live.astype(np.uint32)                                         # act
        self.V[12] = np.where(live, 0xfff, 0)                                       # pm
        self.set64("v[14:15]", np.full(64, EPS))
        self.set64("v[16:17]", np.full(64, EPS2 * (1.0 + 9.094947017729282e-13)))
        self.set64("v[18:19]", np.full(64, EPS2 * (1.0 - 9.094947017729282e-13)))
        self.V[20] = XCH + 128 * r + 32 * g                                         # amine
        self.V[21] = XCH + 32 * g                                                   # axch
        steps, undecided, no_rotation = 0, [], 0
        pc = 0
        with np.errstate(all="ignore"):
            while pc < len(self.prog):
                ins, here = self.prog[pc], pc
                pc += 1
                if ins is None:
                    continue
                mn, ops, offs = ins
                if mn.startswith("v_") or mn.startswith("ds_"):
                    for o in (ops if mn.startswith("ds_write") else ops[1:]):
                        assert not self.pending.intersection(self.vregs(o)), "read of a register an outstanding ds_read fills: " + self.lines[here]
                if mn in ("s_nop",):
                    pass
                elif mn == "s_waitcnt":
                    assert ops == ["lgkmcnt(0)"]
                    self.pending.clear()
                elif mn == "v_mul_f64":
                    self.set64(ops[0], self.f64(ops[1]) * self.f64(ops[2]))
                    if ops[0] == ops[1] == "v[202:203]":      # THR *= eps: the exact threshold of an undecided pair
                        undecided.append(self.copy_of[here])
                elif mn == "v_add_f64":
                    self.set64(ops[0], self.f64(ops[1]) + self.f64(ops[2]))
                elif mn == "v_fma_f64":
                    self.set64(ops[0], fma(self.f64(ops[1]), self.f64(ops[2]), self.f64(ops[3])))
                elif mn == "v_rcp_f64":
                    self.set64(ops[0], 1.0 / self.f64(ops[1]))
                elif mn == "v_rsq_f64":
                    self.set64(ops[0], 1.0 / np.sqrt(self.f64(ops[1])))
                elif mn == "v_mfma_f64_4x4x4_4b_f64":
                    assert np.all(self.f64(ops[1]) == 1.0)
                    b, acc = self.f64(ops[2]).reshape(4, 16), self.f64(ops[3]).copy().reshape(4, 16)
                    for k in range(4):
                        acc = acc + b[k][None, :]
                    self.set64(ops[0], acc.reshape(64))
                elif mn == "v_mov_b64":
                    self.set64(ops[0], self.f64(ops[1]))
                elif mn == "v_mov_b32":
                    self.setv(self.vregs(ops[0])[0], self.u32(ops[1]))
                elif mn in ("v_and_b32", "v_or_b32", "v_xor_b32", "v_add_u32", "v_sub_u32", "v_lshlrev_b32", "v_lshrrev_b32"):
                    a, b = self.u32(ops[1]), self.u32(ops[2])
                    res = {"v_and_b32": lambda: a & b, "v_or_b32": lambda: a | b, "v_xor_b32": lambda: a ^ b, "v_add_u32": lambda: a + b,
                           "v_sub_u32": lambda: a - b, "v_lshlrev_b32": lambda: b << (a & np.uint32(31)),
                           "v_lshrrev_b32": lambda: b >> (a & np.uint32(31))}[mn]()
                    self.setv(self.vregs(ops[0])[0], res.astype(np.uint32))
                elif mn == "v_lshl_add_u32":
                    self.setv(self.vregs(ops[0])[0], ((self.u32(ops[1]) << self.u32(ops[2])) + self.u32(ops[3])).astype(np.uint32))
                elif mn == "v_bfe_u32":
                    self.setv(self.vregs(ops[0])[0], (self.u32(ops[1]) >> self.u32(ops[2])) & np.uint32((1 << int(ops[3])) - 1))
                elif mn in ("v_cmp_ne_u32", "v_cmp_eq_u32"):
                    a, b = self.u32(ops[1]), self.u32(ops[2])
                    self.set_s64(ops[0], to_mask((a != b) if mn == "v_cmp_ne_u32" else (a == b)) & self.exec)
                elif mn in ("v_cmp_gt_f64", "v_cmp_lt_f64", "v_cmp_nle_f64"):
                    a, b = self.f64(ops[1]), self.f64(ops[2])
                    res = (a > b) if mn == "v_cmp_gt_f64" else ((a < b) if mn == "v_cmp_lt_f64" else ~(a <= b))
                    self.set_s64(ops[0], to_mask(res) & self.exec)
                    if mn == "v_cmp_lt_f64":
                        steps += 1
                        assert steps <= max_steps, "the loop does not end"
                elif mn in ("v_cndmask_b32", "v_cndmask_b32_e64"):
                    m = to_lanes(self.s64(ops[3]))
                    self.setv(self.vregs(ops[0])[0], np.where(m, self.u32(ops[2]), self.u32(ops[1])))
                elif mn in ("s_and_b64", "s_or_b64", "s_andn2_b64"):
                    a, b = self.s64(ops[1]), self.s64(ops[2])
                    res = a & b if mn == "s_and_b64" else (a | b if mn == "s_or_b64" else a & ~b & FULL)
                    self.set_s64(ops[0], res)
                    self.scc = int(res != 0)
                elif mn == "s_and_b32":
                    res = self.s32(ops[1]) & self.s32(ops[2])
                    self.S[int(ops[0][1:])] = res
                    self.scc = int(res != 0)
                elif mn == "s_mov_b64":
                    self.set_s64(ops[0], self.s64(ops[1]))
                elif mn == "s_cmp_lg_u64":
                    self.scc = int(self.s64(ops[0]) != self.s64(ops[1]))
                elif mn in ("s_cbranch_scc0", "s_cbranch_scc1"):
                    if self.scc == int(mn[-1]):
                        pc = self.label[ops[0]]
                        if ops[0].startswith("L_skip_"):
                            no_rotation += 1
                elif mn == "ds_read_b32":
                    dst = self.vregs(ops[0])
                    self.V[dst[0]] = self.lds_read(self.u32(ops[1]) + np.uint32(offs.get("offset", 0)), 1)[0]
                    self.pending.update(dst)
                elif mn in ("ds_read_b64", "ds_read_b128"):
                    dst = self.vregs(ops[0])
                    for n, w in zip(dst, self.lds_read(self.u32(ops[1]) + np.uint32(offs.get("offset", 0)), len(dst))):
                        self.V[n] = w
                    self.pending.update(dst)
                elif mn == "ds_write_b64":
                    src = self.vregs(ops[1])
                    self.lds_write(self.u32(ops[0]) + np.uint32(offs.get("offset", 0)), [self.V[n] for n in src])
                elif mn == "ds_write2_b64":
                    for o, k in ((ops[1], offs.get("offset0", 0)), (ops[2], offs.get("offset1", 0))):
                        self.lds_write(self.u32(ops[0]) + np.uint32(8 * k), [self.V[n] for n in self.vregs(o)])
                else:
                    raise AssertionError("mnemonic not interpreted: " + self.lines[here])
        assert self.exec == FULL
        return {"x": self.V[0:6].copy(), "chg": self.V[6].copy(), "flag": self.V[7].copy(), "xch": self.lds[XCH // 4:XCH // 4 + 512].copy(),
                "steps": steps, "undecided": undecided, "no_rotation": no_rotation}


@pytest.fixture(scope="module")
def waves(gen):
    u = gen.Unrolled()
    return u, Wave(gen.program12()), Wave(gen.program12(prev=True))


def random_mtm(seed):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((10, 12)) * np.exp(rng.uniform(-2, 2, 12))[None, :]
    A = M.T @ M
    return (A + A.T) / 2


def _doubles(res, k):
    if k == "xch":
        return res[k].view(np.float64)
    x = res[k]
    return (x[0::2].astype(np.uint64) | (x[1::2].astype(np.uint64) << np.uint64(32))).view(np.float64)


def same(a, b, nan_ok=False):
    """The committed state and the step count, bit for bit.  nan_ok (the fixture's NaN matrix): NaN payloads are nobody's contract -
    where one block holds a NaN the other must hold one too, everything else bit for bit."""
    for k in ("x", "chg", "flag", "xch"):
        if nan_ok and k in ("x", "xch"):
            xf, yf = _doubles(a, k), _doubles(b, k)
            nx, ny = np.isnan(xf), np.isnan(yf)
            if not np.array_equal(nx, ny) or not np.array_equal(xf[~nx].view(np.uint64), yf[~ny].view(np.uint64)):
                return False
        elif not np.array_equal(a[k], b[k]):
            return False
    return a["steps"] == b["steps"]


@pytest.fixture(scope="module")
def results(waves, cases):
    u, new, prev = waves
    mats = [(c["group"].decode(), c["At"], int(c["sweeps"])) for c in cases] + [("r", random_mtm(s), None) for s in range(20)]
    return [(grp, At, sw, new.run(At, u), prev.run(At, u)) for grp, At, sw in mats]


def test_both_blocks_commit_the_same_bits(waves, results):
    u = waves[0]
    assert len(results) >= 60
    for k, (grp, At, sw, a, b) in enumerate(results):
        assert same(a, b, nan_ok=bool(np.isnan(At).any())), (k, grp)
        assert a["undecided"] == b["undecided"] and a["no_rotation"] == b["no_rotation"], (k, grp)
        assert (a["steps"] - u.pro) % u.per == 0 and a["steps"] >= u.pro + u.per
        # idle rows (12..15 of every lane group) commit nothing
        idle = (np.arange(64) & 15) >= 12
        assert not a["chg"][idle].any() and not a["flag"][idle].any()


def test_paths_the_fixture_is_there_for(waves, results):
    """Group f reaches the undecided path in both blocks - in a copy of the prologue and in copies of the period -, groups b and c never
    rotate (every step takes the no-rotation branch and drops its speculative prefix), group e rotates in exactly one step a sweep."""
    u = waves[0]
    f_copies = set()
    for grp, At, sw, a, b in results:
        for res in (a, b):
            if grp == "f":
                assert res["undecided"], "a pair inside the margin did not take the exact path"
            if grp in ("b", "c"):
                assert res["steps"] == u.pro + u.per and res["no_rotation"] == res["steps"] and not res["chg"].any()
            if grp == "e":
                assert res["steps"] == u.pro + 2 * u.per and res["no_rotation"] == res["steps"] - 1
        if grp == "f":
            f_copies |= set(a["undecided"])
    assert any(t < u.pro for t in f_copies) and any(t >= u.pro for t in f_copies), f_copies
    # the stand-in arithmetic converges like the real one: the samples leave after a handful of sweeps, not at the bound
    sw = [(a["steps"] - u.pro) // u.per for grp, At, s, a, b in results if grp in ("a", "r")]
    assert 3 <= min(sw) and max(sw) <= 12 and len(set(sw)) >= 2
    # a NaN runs into the 25-sweep bound with the flag set; nothing else does
    for grp, At, s, a, b in results:
        assert bool(a["flag"].any()) == bool(np.isnan(At).any())


def test_a_planted_mutant_is_seen(gen, waves):
    """The first reciprocal of a rotation fed with the unselected operand (|LO| for |HI|): the comparison above fails."""
    u, new, prev = waves
    lines = gen.program12()
    good = "v_rcp_f64 %s, |%s|" % (gen.pair(gen.RCP), gen.pair(gen.HI))
    assert sum(1 for l in lines if l == good) == u.pro + u.per
    mutant = Wave([("v_rcp_f64 %s, |%s|" % (gen.pair(gen.RCP), gen.pair(gen.LO))) if l == good else l for l in lines])
    At = random_mtm(0)
    assert same(new.run(At, u), prev.run(At, u))
    assert not same(mutant.run(At, u), prev.run(At, u))


def test_registers_and_layout(gen):
    """The rescheduled block stays inside v140..v255 / s60..s71, keeps the alignment in front of L_loop and one backward branch, and
    leaves P alone until the undecided path has read |P| (2p lives in a register of its own)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_jacobi3_regs import _parse, _regs
    lines = gen.program12()
    used = set()
    for l in lines:
        p = _parse(l)
        if p:
            for o in p[1] + p[2]:
                used |= _regs(o)
    vs = {r[1] for r in used if r[0] == "v"}
    ss = {r[1] for r in used if r[0] == "s"}
    assert min(vs) >= 140 and max(vs) <= 255 and min(ss) >= 60 and max(ss) <= 71
    assert lines[lines.index("L_loop_%=:") - 1] == ".p2align %d" % gen.LOOP_ALIGN
    assert sum(1 for l in lines if l.startswith("s_cbranch_scc1 L_loop_")) == 1
    writes_p = [l for l in lines if _parse(l) and _parse(l)[1] and _parse(l)[1][0] == gen.pair(gen.P) and not l.startswith("v_mfma")]
    assert writes_p == [] or 2 not in gen.ITEMS12
