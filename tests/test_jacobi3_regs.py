"""The three-row Jacobi block with the rows in registers (EO_JACOBI_ASM_3R of tools/gen_jacobi_asm.py), checked without a GPU:
its three copies visit the pairs of JacobiSVDImpl_'s cyclic order and close the sweep where the table-driven walk does, problems
side by side leave the loop independently (the block's own scalar bookkeeping is interpreted), its registers stay in the block's
window clear of the fixed ones, and every block of the generator keeps the wait states its docstring states (hazard lint)."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo-semantic-vo_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def gen():
    env = {k: os.environ.pop(k) for k in ("JACOBI_LOOP_ALIGN", "JACOBI_LOOP_NOPS") if k in os.environ}   # default settings
    try:
        import gen_jacobi_asm
    finally:
        os.environ.update(env)
    return gen_jacobi_asm


# ---- the pair sequence ------------------------------------------------------------------------------------------------
def _tab3():
    with open(os.path.join(CSRC, "svo_epnp_ord_tab.h")) as f:
        text = f.read()
    body = re.search(r"c_tab3\[EO_TAB3_STEPS\]\[3\] = \{(.*?)\n\};", text, re.S).group(1)
    rows = [[int(x, 16) for x in re.findall(r"0x[0-9a-f]+", line)] for line in body.strip().splitlines()]
    pro = int(re.search(r"#define EO_TAB3_PROLOGUE (\d+)", text).group(1))
    return rows, pro


def _table_walk3(nsteps):
    """(i, j, closes) per step as the table-driven loop decodes the committed three-row schedule."""
    tab, pro = _tab3()
    tt, out = 0, []
    for _ in range(nsteps):
        pairs = set()
        for r in range(3):
            e = tab[tt][r]
            if (e & 15) != r:
                i, j = ((e & 15), r) if e & 16 else (r, e & 15)      # bit 4: r is the pair's second row
                pairs.add((i, j))
        assert len(pairs) == 1
        (i, j), = pairs
        out.append((i, j, bool(tab[tt][0] & 0x80)))
        tt += 1
        if tt == len(tab):
            tt = pro
    return out


def test_copies_visit_the_cyclic_order(gen):
    """32 sweeps: JacobiSVDImpl_'s `for i < n - 1: for j in i + 1 .. n - 1` for n = 3, the committed table and the block's copies give the
    same pairs in the same order, and the sweep closes behind the same step."""
    n, sweeps = 3, 32
    cv = [(i, j, (i, j) == (n - 2, n - 1)) for _ in range(sweeps) for i in range(n - 1) for j in range(i + 1, n)]
    copies = [(i, j, k == len(gen.R3_PAIRS) - 1) for _ in range(sweeps) for k, (i, j) in enumerate(gen.R3_PAIRS)]
    assert cv == copies == _table_walk3(3 * sweeps)


# ---- the emitted block, parsed -------------------------------------------------------------------------------------------
def _lines(gen, which):
    return {"12": gen.program12, "6": lambda: gen.program(6), "3": lambda: gen.program(3), "3R": gen.program3r}[which]()


def _regs(op):
    """Registers an operand names: ('v', n) / ('s', n) / ('vcc',)."""
    out = set()
    for lo, hi in re.findall(r"\bv\[(\d+):(\d+)\]", op):
        out |= {("v", k) for k in range(int(lo), int(hi) + 1)}
    for lo, hi in re.findall(r"\bs\[(\d+):(\d+)\]", op):
        out |= {("s", k) for k in range(int(lo), int(hi) + 1)}
    out |= {("v", int(k)) for k in re.findall(r"\bv(\d+)\b", op)}
    out |= {("s", int(k)) for k in re.findall(r"\bs(\d+)\b", op)}
    if re.search(r"\bvcc\b", op):
        out.add(("vcc",))
    return out


def _parse(line):
    """(mnemonic, destination operands, source operands) of an instruction line; None for labels and directives."""
    line = line.strip()
    if line.endswith(":") or line.startswith("."):
        return None
    mn, _, rest = line.partition(" ")
    ops = [o.strip() for o in rest.split(",")] if rest else []
    ops = [re.sub(r"\s+offset\d?:\d+", "", o) for o in ops]
    if mn.startswith(("s_nop", "s_waitcnt", "s_cbranch", "s_branch")):
        return mn, [], []
    if mn.startswith("s_cmp"):
        return mn, [], ops
    if mn.startswith("ds_write"):
        return mn, [], ops
    ndst = 2 if "_co_" in mn else 1
    return mn, ops[:ndst], ops[ndst:]


def _mask_operand(mn, srcs):
    """The operand a VALU instruction reads as a lane mask (None: it reads none)."""
    if mn.startswith("v_cndmask"):
        return srcs[2]
    if mn.startswith("v_addc_co"):
        return srcs[2]
    return None


def lint(lines):
    """Walks the instruction list in program order and returns the violations of the distances of the generator's docstring.  A wait
    state is one instruction or one count of an s_nop; a register's entry holds what last wrote it and how many wait states ago."""
    last = {}          # register -> (kind of the writer, wait states issued since)
    bad = []

    def need(reg, kinds, n, what, idx, line):
        w = last.get(reg)
        if w and w[0] in kinds and w[1] < n:
            bad.append("%d: %s  [%s: %d < %d on %s]" % (idx, line.strip(), what, w[1], n, reg))

    for idx, line in enumerate(lines):
        p = _parse(line)
        if p is None:
            continue
        mn, dsts, srcs = p
        src_regs = set().union(*[_regs(o) for o in srcs]) if srcs else set()
        valu = mn.startswith("v_") and not mn.startswith("v_mfma")
        if mn.startswith("v_mfma"):
            for r in _regs(srcs[0]) | _regs(srcs[1]):
                need(r, {"valu", "trans"}, 2, "VALU write -> DMFMA read", idx, line)
                need(r, {"mfma"}, 4, "DMFMA -> dependent DMFMA", idx, line)
            for r in _regs(srcs[2]):
                need(r, {"valu", "trans"}, 2, "VALU write -> DMFMA read", idx, line)
                need(r, {"mfma"}, 4, "DMFMA -> dependent DMFMA (SrcC)", idx, line)
        elif valu:
            for r in src_regs:
                need(r, {"trans"}, 1, "transcendental -> read", idx, line)
                need(r, {"mfma"}, 6, "DMFMA -> VALU read", idx, line)
            m = _mask_operand(mn, srcs)
            if m is not None:
                for r in _regs(m):
                    need(r, {"valu", "trans"}, 2, "VALU write of a lane mask -> its use", idx, line)
        elif mn.startswith("ds_"):
            for r in src_regs:
                need(r, {"mfma"}, 9, "DMFMA -> LDS read", idx, line)
        # time passes
        ws = int(line.split()[1]) + 1 if mn == "s_nop" else 1
        for r in list(last):
            last[r] = (last[r][0], last[r][1] + ws)
        kind = "mfma" if mn.startswith("v_mfma") else ("trans" if mn.startswith(("v_rcp_f64", "v_rsq_f64")) else ("valu" if valu else "other"))
        for o in dsts:
            for r in _regs(o):
                last[r] = (kind, 0)
    return bad


@pytest.mark.parametrize("which", ["12", "6", "3", "3R"])
def test_hazard_lint(gen, which):
    """1 after v_rcp_f64 / v_rsq_f64, 2 from a VALU write to a DMFMA read, 4 between dependent DMFMAs, 6 before a VALU read and 9 before
    an LDS read of a DMFMA result, 2 from a VALU write of VCC / an SGPR to its use as a lane mask.  The three older blocks are proven
    by bit parity on the GPU: the lint has to pass on them as they stand."""
    lines = _lines(gen, which)
    assert sum(1 for l in lines if l.startswith("v_mfma")) >= 3
    assert lint(lines) == []


def test_hazard_lint_sees_a_missing_wait_state(gen):
    """The lint is not vacuous: with the wait states in front of decide() shortened by one, it reports the early read of a DMFMA sum,
    and without the s_nop behind a v_rcp_f64 the read of the reciprocal."""
    lines = _lines(gen, "3R")
    k = lines.index("s_nop 4")
    assert any("DMFMA -> VALU read" in b for b in lint(lines[:k] + ["s_nop 3"] + lines[k + 1:]))
    k = next(i for i, l in enumerate(lines) if l.startswith("v_rcp_f64"))
    assert lines[k + 1] == "s_nop 0"
    assert any("transcendental" in b for b in lint(lines[:k + 1] + lines[k + 2:]))
    k = next(i for i, l in enumerate(lines) if l.startswith("v_cmp_gt_f64 vcc, |"))
    assert lines[k + 1] == "s_nop 1"
    assert any("lane mask" in b for b in lint(lines[:k + 1] + ["s_nop 0"] + lines[k + 2:]))


# ---- registers --------------------------------------------------------------------------------------------------------------
def test_registers_in_the_window(gen):
    lines = _lines(gen, "3R")
    used = set()
    for l in lines:
        p = _parse(l)
        if p:
            for o in p[1] + p[2]:
                used |= _regs(o)
    vs = {r[1] for r in used if r[0] == "v"}
    ss = {r[1] for r in used if r[0] == "s"}
    assert vs and min(vs) >= 140 and max(vs) <= 255
    assert ss and min(ss) >= 60 and max(ss) <= 71
    own = set()
    for row in gen.R3:
        for lo in row:
            own |= {lo, lo + 1}
    own |= {gen.R3_QI, gen.R3_TMP}
    assert len(own) == 14
    fixed = set()
    for lo in (gen.X0, gen.X1, gen.X2, gen.WW, gen.RCP, gen.ERR, gen.REM, gen.QQ, gen.TA, gen.TB, gen.TC, gen.ONE, gen.T0, gen.T1, gen.T2, gen.AB,
               gen.Y, gen.G, gen.H, gen.RR, gen.D, gen.P, gen.THR, gen.PLO, gen.PLO + 2, gen.P2, gen.WP, gen.BETA, gen.HI, gen.LO, gen.GAM, gen.R1,
               gen.R2, gen.CC, gen.SS, gen.N0, gen.N1, gen.N2, gen.U0, gen.U1, gen.U2, gen.V0, gen.V1, gen.V2):
        fixed |= {lo, lo + 1}
    assert not own & fixed
    # the temporaries of the row update are distinct pairs, and none of them is a rotation input still to be read (CC, SS)
    tmp = [lo for grp in (gen.R3_N, gen.R3_T) for row in grp for lo in row]
    assert len(set(tmp)) == 8 and not {gen.CC, gen.SS} & set(tmp)
    # no exec change, no LDS traffic behind the set-up, no sign register, no table
    loop = lines[lines.index("L_loop_%=:"):]
    assert not any("exec" in l or l.startswith("ds_") or "v_xor_b32" in l for l in loop)
    assert sum(1 for l in lines if l.startswith("ds_")) == 3
    assert sum(1 for l in lines if l.startswith("s_cbranch_scc1 L_loop_")) == 1      # one backward branch
    assert lines[lines.index("L_loop_%=:") - 1] == ".p2align %d" % gen.LOOP_ALIGN


# ---- the sweep bookkeeping, interpreted ------------------------------------------------------------------------------------
FULL = (1 << 64) - 1


def _lanes(problem):
    """The lanes of problem p of the three side by side (rows 5 p .. 5 p + 2 in every lane group)."""
    return sum(1 << (16 * g + 5 * problem + q) for g in range(4) for q in range(3))


def _run(gen, rotates, max_steps=400):
    """Interprets the scalar skeleton of the emitted block (masks, counter, branches, the flag's two VALU instructions); the arithmetic
    is replaced by `rotates(problem, sweep, copy)`.  Returns (per problem: sweeps it took part in, flag per problem, sweeps run)."""
    lines = _lines(gen, "3R")
    label = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    act_lanes = sum(_lanes(p) for p in range(3))
    S = {"s[60:61]": 0, "s[64:65]": 0, "s[68:69]": 0, "s[70:71]": 0, "vcc": 0, "s66": 0}
    scc, flag, tmpv = 0, 0, 0
    took = [0, 0, 0]
    copy, pc, steps = 0, 0, 0

    def val(o):
        return S[o] if o in S else int(o, 0)

    while pc < len(lines):
        l = lines[pc]
        pc += 1
        if l.endswith(":") or l.startswith("."):
            continue
        mn, _, rest = l.partition(" ")
        ops = [o.strip() for o in rest.split(",")]
        if mn == "v_cmp_ne_u32" and ops[0] == "s[60:61]":
            S["s[60:61]"] = act_lanes
        elif mn == "v_cmp_gt_f64" and ops[0] == "vcc" and ops[1].startswith("v[%d" % gen.G):      # decide(): p^2 well above
            steps += 1
            assert steps <= max_steps, "the loop does not end"
            sweep = S["s66"]
            rot = sum(_lanes(p) for p in range(3) if rotates(p, sweep, copy))
            for p in range(3):
                if copy == 0 and S["s[60:61]"] & _lanes(p):
                    took[p] += 1
            S["vcc"] = rot
            S["_lt"] = FULL & ~rot
            copy = (copy + 1) % 3
        elif mn == "v_cmp_lt_f64":
            S[ops[0]] = S.pop("_lt")
        elif mn in ("s_and_b64", "s_or_b64", "s_andn2_b64"):
            a, b = val(ops[1]), val(ops[2])
            r = a & b if mn == "s_and_b64" else (a | b if mn == "s_or_b64" else a & ~b & FULL)
            S[ops[0]] = r
            scc = int(r != 0)
        elif mn in ("s_mov_b64", "s_mov_b32"):
            S[ops[0]] = val(ops[1])
        elif mn == "s_add_u32":
            S[ops[0]] = val(ops[1]) + val(ops[2])
        elif mn == "s_cmp_lt_u32":
            scc = int(val(ops[0]) < val(ops[1]))
        elif mn == "s_cmp_lg_u64":
            scc = int(val(ops[0]) != val(ops[1]))
        elif mn in ("s_cbranch_scc0", "s_cbranch_scc1"):
            if scc == int(mn[-1]):
                pc = label[ops[0]]
        elif mn == "v_cndmask_b32_e64" and ops[1:3] == ["0", "1"]:
            tmpv = val(ops[3])
        elif mn == "v_or_b32" and ops[0] == "%[flag]":
            flag |= tmpv
        else:
            assert not mn.startswith("s_") or mn in ("s_nop", "s_waitcnt"), l      # nothing scalar goes uninterpreted
    flags = [bool(flag & _lanes(p)) for p in range(3)]
    for p in range(3):
        assert (flag & _lanes(p)) in (0, _lanes(p))
    return took, flags, S["s66"]


def test_problems_leave_independently(gen):
    """Problem p rotates (somewhere) in its first stop[p] sweeps: it runs stop[p] + 1 sweeps - the last one finds nothing to rotate - and
    the loop ends with the slowest problem.  Which copy of a sweep rotates makes no difference."""
    for stop, where in (((1, 4, 2), 0), ((3, 0, 7), 1), ((2, 2, 5), 2), ((0, 0, 0), 0)):
        took, flags, sweeps = _run(gen, lambda p, s, c: s < stop[p] and c == where)
        assert took == [s + 1 for s in stop]
        assert flags == [False, False, False]
        assert sweeps == max(stop) + 1


def test_sweep_bound(gen):
    """A problem that never stops rotating is cut off after 25 sweeps with its flag set - and so is one that stops exactly in the 25th,
    as in the table-driven block; a problem that left earlier keeps a clear flag."""
    took, flags, sweeps = _run(gen, lambda p, s, c: c == 2 and (p == 0 or (p == 1 and s < 24) or (p == 2 and s < 3)))
    assert sweeps == gen.R3_MAX_SWEEPS == 25
    assert took == [25, 25, 4]
    assert flags == [True, True, False]
