"""The unrolled 12-row step loop of the wave Jacobi engine (tools/gen_jacobi_asm.py -> csrc/svo_epnp_ord_asm.h), checked without a GPU:
the committed header is the generator's output, the per-copy constants of the unrolled program visit the same (pair, sweep) items
per lane as the table walk they replace, and the two table-driven macros (M = 6, M = 3) are the ones of the commit before."""
import contextlib
import hashlib
import io
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo-semantic-vo_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

# SHA-256 of the macro texts ("#define EO_JACOBI_ASM_<M> \" up to and including the macro's last line) as they were before the
# M = 12 loop was unrolled: M = 6 and M = 3 stay table-driven
TABLE_DRIVEN_SHA256 = {
    6: "7c25e4717dbad785e70ea53cc2222cb6971b8d37f35a9784f3ddfd7523c82503",
    3: "a50f709544eb8cda2686103133fe41d786bd801af9e5de797b0aaebee136bdec",
}


@pytest.fixture(scope="module")
def gen():
    env = {k: os.environ.pop(k) for k in ("JACOBI_LOOP_ALIGN", "JACOBI_LOOP_NOPS") if k in os.environ}   # default settings
    try:
        import gen_jacobi_asm
    finally:
        os.environ.update(env)
    return gen_jacobi_asm


def _header():
    with open(os.path.join(CSRC, "svo_epnp_ord_asm.h")) as f:
        return f.read()


def test_committed_header_is_the_generators_output(gen):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        gen.main()
    assert out.getvalue() == _header()


def test_committed_table_is_the_schedule_the_generator_unrolls(gen):
    """csrc/svo_epnp_ord_tab.h (what the block reads from LDS at run time) holds the entries the generator took its constants from."""
    with open(os.path.join(CSRC, "svo_epnp_ord_tab.h")) as f:
        text = f.read()
    u = gen.Unrolled()
    body = re.search(r"c_tab12\[EO_TAB12_STEPS\]\[12\] = \{(.*?)\n\};", text, re.S).group(1)
    rows = [[int(x, 16) for x in re.findall(r"0x[0-9a-f]+", line)] for line in body.strip().splitlines()]
    assert rows == u.tab
    assert int(re.search(r"#define EO_TAB12_PROLOGUE (\d+)", text).group(1)) == u.pro
    assert int(re.search(r"#define EO_TAB12_STEPS (\d+)", text).group(1)) == u.pro + u.per


def _table_walk(u, nsteps):
    """What the table-driven loop decodes, step by step (TT, TP, the wrap to PRO, the sweep base's carry): per step a list over the
    64 lanes of (partner row, valid, second row of the pair, sweep) and the sweep the step closes (or None)."""
    steps, pro, n = u.pro + u.per, u.pro, 12
    tt, sb, out = 0, 0, []
    for _ in range(nsteps):
        lanes = []
        for lane in range(64):
            r = lane & 15
            if r >= n:                              # n = 0: the row idles (ACT is clear), it reads its own row
                lanes.append((r, False, None, None))
                continue
            e = u.tab[tt][r]
            valid = (e & 15) != r
            lanes.append(((e & 15) if valid else r, valid, (e >> 4) & 1 if valid else None, sb + ((e >> 5) & 3) if valid else None))
        e0 = u.tab[tt][0]
        out.append((lanes, sb + ((e0 >> 8) & 3) if e0 & 0x80 else None))
        tt += 1
        if tt == steps:
            tt, sb = pro, sb + 1
    return out


def _unrolled_walk(u, nsteps):
    """The same from the unrolled program's constants: the copies in execution order, the base bit doubled behind a closing copy."""
    t, base, out = 0, 0, []
    for _ in range(nsteps):
        lanes = []
        for lane in range(64):
            partner, valid, second, srel, closes = u.lane_constants(t, lane)
            lanes.append((partner, valid, second if valid else None, base + srel if valid else None))
        closes = u.closes(t)
        out.append((lanes, base + closes if closes is not None else None))
        if closes is not None:
            base += 1
        t = u.next_copy(t)
    return out


def test_unrolled_constants_visit_what_the_table_walk_visits(gen):
    """Every lane, every step of 32 sweeps: partner row, valid bit, sign (second row of the pair), sweep index and closing flag.
    (Sign and sweep are compared where the lane has a pair: nothing reads them elsewhere.)"""
    u = gen.Unrolled()
    u.check()
    nsteps = u.pro + 32 * u.per
    a, b = _table_walk(u, nsteps), _unrolled_walk(u, nsteps)
    closed = [c for _, c in a if c is not None]
    assert closed == list(range(len(closed))) and len(closed) >= 30
    for step, (x, y) in enumerate(zip(a, b)):
        assert x[1] == y[1], ("closing flag", step)
        for lane in range(64):
            assert x[0][lane] == y[0][lane], (step, lane, x[0][lane], y[0][lane])


def test_unrolled_layout(gen):
    """One exit: the only closing copy is the last one of the period (the backward branch sits behind it), so a solve that stops
    after s + 1 sweeps has run PRO + (s + 1) PER steps.  Slots and registers are one to one."""
    u = gen.Unrolled()
    assert [t for t in u.copies() if u.closes(t) is not None] == [u.pro + u.per - 1]
    assert sorted(u.slot(t) for t in range(u.pro, u.pro + u.per)) == list(range(u.per))
    regs = gen.U_AP + gen.U_K + [gen.U_SGN, gen.U_TMP, gen.U_BB, gen.U_TMP2]
    assert len(set(regs)) == len(regs) and all(140 <= r <= 255 for r in regs)
    fixed = set()
    for lo in (gen.X0, gen.X1, gen.X2, gen.WW, gen.RCP, gen.ERR, gen.REM, gen.QQ, gen.TA, gen.TB, gen.TC, gen.ONE, gen.T0, gen.T1, gen.T2, gen.AB,
               gen.Y, gen.G, gen.H, gen.RR, gen.D, gen.P, gen.THR, gen.PLO, gen.PLO + 2, gen.P2, gen.WP, gen.BETA, gen.HI, gen.LO, gen.GAM, gen.R1,
               gen.R2, gen.CC, gen.SS, gen.N0, gen.N1, gen.N2, gen.U0, gen.U1, gen.U2, gen.V0, gen.V1, gen.V2):
        fixed |= {lo, lo + 1}
    assert not fixed & set(regs)


@pytest.mark.parametrize("M", [6, 3])
def test_table_driven_macros_are_untouched(M):
    m = re.search(r'(#define EO_JACOBI_ASM_%d \\\n(?:  ".*\n)+)' % M, _header())
    assert hashlib.sha256(m.group(1).encode()).hexdigest() == TABLE_DRIVEN_SHA256[M]
