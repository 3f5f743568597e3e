"""Generates csrc/svo_epnp_ord_asm.h: the step loop of the wave Jacobi engine (jacobi_rows of svo_epnp_ord_dev.h) as ONE
inline-assembly block per column count M in {12, 6, 3}, plus the block jacobi_rows<3> uses (3R) - the compiler's version of the same loop spends more than half of a
step on copies of the loop-carried rows, lane-mask bookkeeping and branches (measured: 675 of 1200 ticks per step with the
arithmetic and the LDS traffic removed).

What a step does is documented where it is used (svo_epnp_ord_dev.h); this file only fixes registers and instruction order.
Wait states follow LLVM's GCNHazardRecognizer for gfx940/gfx950: 1 after a transcendental (v_rcp_f64 / v_rsq_f64) before its
result is read, 2 between a VALU write of an SGPR / VCC and a VALU read of it as a lane mask, 2 between a VALU write of a VGPR
and a DMFMA read of it, 4 between dependent 4x4x4 DMFMAs (SrcC), 6 before a VALU read and 9 before an LDS read of a DMFMA
result.

Three layouts:
  M = 6, M = 3 (program): ONE copy of the step body that walks the schedule table in LDS - the entry of step t + 2 is read while
    step t computes (TT / TP / SB, wrap to the prologue's end), decode() turns an entry into the partner's address, the lane mask
    VALID, the sign and the sweep bit, and every step tests the entry's closing bit.  Three problems of different sizes share
    one schedule there, with per-problem closing bits.
  M = 12 (program12, class Unrolled): one problem, so everything decode() derives depends on the lane and the step only.  The
    schedule (tools/gen_jacobi_schedule.py: PRO prologue steps, then PER steps that repeat with the sweep base one higher) is
    unrolled: one copy of the step body per step - the PRO prologue copies, then, behind .p2align, the PER copies of the period
    with ONE backward branch.  Before the first step the block reads the lane's PER table entries of the period from LDS and
    turns them into two registers per slot (partner row's address; sign | relative sweep); VALID of a copy is a 16-bit constant
    of that copy & ACT; the sweep bookkeeping and the exit test are emitted only in the copy that closes a sweep (the period's
    last), where the base bit U_BB is doubled.  No table read, no walk, no decode and no closing test per step.  The commit and
    the write-back are the same instruction sequences as in the table-driven layout; the sums, the decision and the rotation are
    the same operations in an order that follows the step's dependent chain (pair_test12 / decide_rotate12 below).  The block
    with pair_test, decide and rotation in the table-driven layout's order stays as EO_JACOBI_ASM_12_PREV (--prev; -DEO_JACOBI12_PREV).

  M = 3, rows in registers (program3r, EO_JACOBI_ASM_3R): three-row problems only - what every caller of jacobi_rows<3> passes.  Each
    lane holds columns g and 4 + g of all three rows of its problem, so a step needs no partner row from LDS: three copies of the
    step body for the pairs (0, 1), (0, 2), (1, 2) behind .p2align with ONE backward branch, both rows updated in the lane, scalar
    sweep bookkeeping in the third copy only.  pair_test's, decide's and the rotation's instruction sequences as in the other layouts.
    The table-driven M = 3 block stays (jacobi_rows<3> with -DEO_JACOBI3_TABLE; its text is pinned by tests/test_jacobi_unrolled.py).

Registers: the block owns v140..v255 and s60..s71 (clobbers); the row (x0, x1, x2) lives in v150..v155 while the loop runs.
  v140..v149, v174..v175  U0..U2, V0..V2 (squares for the DMFMA chains)       v150..v157  X0..X2, WW
  v160..v173  division / square-root temporaries, QQ, TA..TC                  v180..v199  ONE, T0..T2, AB, Y, G, H, RR, D
  v200..v233  P, THR, PLO (partner row, 4 + 2 registers with P2), WP, BETA, HI, LO, GAM, R1, R2, CC, SS, N0..N2
  table-driven: v234..v253  E, E1, E2, TT, TP, SB, SBE, SBE1, SGN, SWBIT, AP, AW, TMP, TMP2, ROW, QI, ONEI, STEPS, PRO, TSTEP
  unrolled:     v234..v245  U_AP[0..11] partner addresses per slot; v158, v159, v176..v179, v246..v251  U_K[0..11] sign | sweep
                v252 U_SGN, v253 U_TMP, v254 U_BB (1 << sweep base), v255 U_TMP2; N0 / N1 hold the row and its index during set-up
  rows in registers: v234..v245  R3[row][column group], v246 R3_QI (row index in the problem), v247 R3_TMP; the rotated rows go through
                N0..N2, V0 and T0..T2, U0
  s[60:61] ACT, s[62:63] VALID, s[64:65] ROT, s[66:67] SAVE (exec), s[68:69] CL, s[70:71] ST
  (rows in registers: ACT stands for VALID, CL collects the lanes that rotated in the sweep under way, s66 counts sweeps)
"""

import os
LOOP_ALIGN = int(os.environ.get("JACOBI_LOOP_ALIGN", "6"))    # log2 bytes
LOOP_NOPS = int(os.environ.get("JACOBI_LOOP_NOPS", "0"))      # 4-byte s_nops between the alignment and the loop's first instruction


# ---- fixed registers -------------------------------------------------------------------------------------------------
def pair(lo):
    return "v[%d:%d]" % (lo, lo + 1)


X0, X1, X2, WW = 150, 152, 154, 156
RCP, ERR, REM, QQ, TA, TB, TC = 160, 162, 164, 166, 168, 170, 172
ONE, T0, T1, T2, AB, Y, G, H, RR, D = 180, 182, 184, 186, 188, 190, 192, 194, 196, 198
P, THR, PLO, P2, WP, BETA, HI, LO, GAM, R1, R2, CC, SS, N0, N1, N2 = 200, 202, 204, 208, 210, 212, 214, 216, 218, 220, 222, 224, 226, 228, 230, 232
Q0, Q1 = PLO, PLO + 2
U0, U1, U2, V0, V1, V2 = 140, 142, 144, 146, 148, 174
E, E1, E2, TT, TP, SB, SBE, SBE1, SGN, SWBIT, AP, AW, TMP, TMP2, ROW, QI, ONEI, STEPS, PRO, TSTEP = range(234, 254)
ACT, VALID, ROT, SAVE, CL, ST = "s[60:61]", "s[62:63]", "s[64:65]", "s[66:67]", "s[68:69]", "s[70:71]"


def v(n):
    return "v%d" % n


def ndiv(dst, a, b):
    """dst = a / b, the compiler's IEEE division without range scaling / fix-up (see ndiv in svo_epnp_ord_dev.h)."""
    r, e, rem = pair(RCP), pair(ERR), pair(REM)
    return [
        "v_rcp_f64 %s, %s" % (r, b),
        "s_nop 0",
        "v_fma_f64 %s, -%s, %s, 1.0" % (e, b, r),
        "v_fma_f64 %s, %s, %s, %s" % (r, r, e, r),
        "v_fma_f64 %s, -%s, %s, 1.0" % (e, b, r),
        "v_fma_f64 %s, %s, %s, %s" % (r, r, e, r),
        "v_mul_f64 %s, %s, %s" % (dst, a, r),
        "v_fma_f64 %s, -%s, %s, %s" % (rem, b, dst, a),
        "v_fma_f64 %s, %s, %s, %s" % (dst, rem, r, dst),
    ]


def nsqrt(dst, x):
    """dst = sqrt(x), x > 0, the compiler's IEEE square root without range scaling (see nsqrt in svo_epnp_ord_dev.h)."""
    y, h, r, d = pair(Y), pair(H), pair(RR), pair(D)
    return [
        "v_rsq_f64 %s, %s" % (y, x),
        "s_nop 0",
        "v_mul_f64 %s, %s, %s" % (dst, x, y),
        "v_mul_f64 %s, %s, 0.5" % (h, y),
        "v_fma_f64 %s, -%s, %s, 0.5" % (r, h, dst),
        "v_fma_f64 %s, %s, %s, %s" % (dst, dst, r, dst),
        "v_fma_f64 %s, %s, %s, %s" % (h, h, r, h),
        "v_fma_f64 %s, -%s, %s, %s" % (d, dst, dst, x),
        "v_fma_f64 %s, %s, %s, %s" % (dst, d, h, dst),
        "v_fma_f64 %s, -%s, %s, %s" % (d, dst, dst, x),
        "v_fma_f64 %s, %s, %s, %s" % (dst, d, h, dst),
    ]


def mfma(dst, b, c):
    return "v_mfma_f64_4x4x4_4b_f64 %s, %s, %s, %s" % (dst, pair(ONE), b, c)


def pair_test(M, wait=1):
    """P = sum_k mine[k] theirs[k], WW = sum_k mine[k]^2 (= W of my row), WP = sum_k theirs[k]^2 (= W of the partner row) over the A
    columns: three interleaved DMFMA chains (dependent DMFMAs end up 4 wait states apart)."""
    p, wa, wb = pair(P), pair(WW), pair(WP)
    regs = ((T0, U0, V0, X0, Q0), (T1, U1, V1, X1, Q1), (T2, U2, V2, X2, P2))
    nq = {12: 3, 6: 2, 3: 1}[M]
    out = []
    for q in range(nq):      # the squares of my own row need no partner: they go in front of the wait for its arrival
        t, u, w, x, y = regs[q]
        out.append("v_mul_f64 %s, %s, %s" % (pair(u), pair(x), pair(x)))
    out.append("s_waitcnt lgkmcnt(%d)" % wait)     # the partner's row (requested at the end of the previous step; table-driven loop:
                                                   # the table read issued after it may still be on its way)
    for q in range(nq):
        t, u, w, x, y = regs[q]
        out += ["v_mul_f64 %s, %s, %s" % (pair(t), pair(x), pair(y)), "v_mul_f64 %s, %s, %s" % (pair(w), pair(y), pair(y))]
    if M != 12:          # the partly filled column group: V columns count as +0.0
        t, u, w, x, y = regs[nq - 1]
        out += ["v_mul_f64 %s, %s, %%[mk]" % (pair(r), pair(r)) for r in (t, u, w)]
        out.append("s_nop 0")
    for q in range(nq):
        t, u, w, x, y = regs[q]
        c = (lambda r: "0") if q == 0 else (lambda r: r)
        if q:
            out.append("s_nop 1")
        out += [mfma(wa, pair(u), c(wa)), mfma(wb, pair(w), c(wb)), mfma(p, pair(t), c(p))]
    out.append("s_nop 4")     # 6 wait states between a chain's last DMFMA and the VALU read of its sum: decide() reads WW and WP
                              # first (5 + the DMFMA into P), then P (5 + one VALU instruction)
    return out


def decide(tag="", valid=None):
    """ROT = VALID & !(|p| <= eps sqrt(W[i] W[j])) (`valid`: the lane mask that stands for VALID; the register layout has none of its own).  Decided on the squares with a margin of 2^-40 (the roundings of either side are
    of the order 2^-52); a pair inside the margin - or with a NaN - takes the exact expression for the whole wave."""
    valid = valid or VALID
    return [
        "v_mul_f64 %s, %s, %s" % (pair(AB), pair(WW), pair(WP)),
        "v_mul_f64 %s, %s, %s" % (pair(G), pair(P), pair(P)),
        "v_mul_f64 %s, %s, %%[eps2hi]" % (pair(H), pair(AB)),
        "v_mul_f64 %s, %s, %%[eps2lo]" % (pair(RR), pair(AB)),
        "v_cmp_gt_f64 vcc, %s, %s" % (pair(G), pair(H)),            # p^2 well above: rotates
        "v_cmp_lt_f64 %s, %s, %s" % (ST, pair(G), pair(RR)),        # well below: does not
        "s_or_b64 %s, vcc, %s" % (ST, ST),
        "s_andn2_b64 %s, %s, %s" % (ST, valid, ST),                 # undecided (valid pairs only)
        "s_cbranch_scc0 L_decided_%s%%=" % tag,
    ] + nsqrt(pair(THR), pair(AB)) + [
        "v_mul_f64 %s, %s, %%[eps]" % (pair(THR), pair(THR)),
        "v_cmp_nle_f64 vcc, |%s|, %s" % (pair(P), pair(THR)),
        "L_decided_%s%%=:" % tag,
        "s_and_b64 %s, vcc, %s" % (ROT, valid),
    ]


def rotation_cs(sgn):
    """(c, s) of the pair by OpenCV's formulas, into CC and SS; `sgn`: the register that holds 0x80000000 in the lanes of the pair's
    second (j) row (there WW / WP are W[j] / W[i] and the lane gets -s), or None: every lane is on the first row's side."""
    o = []
    a = o.append
    a("v_add_f64 %s, %s, %s" % (pair(P), pair(P), pair(P)))
    a("v_add_f64 %s, %s, -%s" % (pair(BETA), pair(WW), pair(WP)))
    if sgn is not None:
        a("v_xor_b32 %s, %s, %s" % (v(BETA + 1), v(BETA + 1), v(sgn)))
    a("v_cmp_gt_f64 vcc, |%s|, |%s|" % (pair(P), pair(BETA)))
    a("s_nop 1")
    a("v_cndmask_b32 %s, %s, %s, vcc" % (v(HI), v(BETA), v(P)))
    a("v_cndmask_b32 %s, %s, %s, vcc" % (v(HI + 1), v(BETA + 1), v(P + 1)))
    a("v_cndmask_b32 %s, %s, %s, vcc" % (v(LO), v(P), v(BETA)))
    a("v_cndmask_b32 %s, %s, %s, vcc" % (v(LO + 1), v(P + 1), v(BETA + 1)))
    o += ndiv(pair(QQ), "|%s|" % pair(LO), "|%s|" % pair(HI))
    a("v_mul_f64 %s, %s, %s" % (pair(TA), pair(QQ), pair(QQ)))
    a("v_add_f64 %s, %s, 1.0" % (pair(TA), pair(TA)))
    o += nsqrt(pair(TB), pair(TA))
    a("v_mul_f64 %s, |%s|, %s" % (pair(GAM), pair(HI), pair(TB)))
    a("v_add_f64 %s, %s, |%s|" % (pair(TA), pair(GAM), pair(BETA)))
    a("v_add_f64 %s, %s, %s" % (pair(TC), pair(GAM), pair(GAM)))
    o += ndiv(pair(QQ), pair(TA), pair(TC))
    o += nsqrt(pair(R1), pair(QQ))
    a("v_mul_f64 %s, %s, %s" % (pair(TA), pair(GAM), pair(R1)))
    a("v_add_f64 %s, %s, %s" % (pair(TA), pair(TA), pair(TA)))
    o += ndiv(pair(R2), pair(P), pair(TA))
    a("v_cmp_gt_f64 vcc, 0, %s" % pair(BETA))
    a("s_nop 1")
    a("v_cndmask_b32 %s, %s, %s, vcc" % (v(SS), v(R2), v(R1)))
    a("v_cndmask_b32 %s, %s, %s, vcc" % (v(SS + 1), v(R2 + 1), v(R1 + 1)))
    a("v_cndmask_b32 %s, %s, %s, vcc" % (v(CC), v(R1), v(R2)))
    a("v_cndmask_b32 %s, %s, %s, vcc" % (v(CC + 1), v(R1 + 1), v(R2 + 1)))
    if sgn is not None:
        a("v_xor_b32 %s, %s, %s" % (v(SS + 1), v(SS + 1), v(sgn)))
    return o


def rotation(sgn):
    """(c, s) and the rotated row N0..N2 = c mine + (+-s) theirs."""
    o = rotation_cs(sgn)
    a = o.append
    for n_, x_, q_, t_ in ((N0, X0, Q0, T0), (N1, X1, Q1, T1), (N2, X2, P2, T2)):
        a("v_mul_f64 %s, %s, %s" % (pair(n_), pair(CC), pair(x_)))
        a("v_mul_f64 %s, %s, %s" % (pair(t_), pair(SS), pair(q_)))
    for n_, t_ in ((N0, T0), (N1, T1), (N2, T2)):
        a("v_add_f64 %s, %s, %s" % (pair(n_), pair(n_), pair(t_)))
    return o


def commit():
    """The rows that rotate take the rotated row."""
    o = []
    a = o.append
    for x_, n_ in ((X0, N0), (X1, N1), (X2, N2)):
        a("v_cndmask_b32_e64 %s, %s, %s, %s" % (v(x_), v(x_), v(n_), ROT))
        a("v_cndmask_b32_e64 %s, %s, %s, %s" % (v(x_ + 1), v(x_ + 1), v(n_ + 1), ROT))
    return o


def write_back():
    """The rotated rows go back to the exchange (lanes of ROT only)."""
    return [
        "s_mov_b64 %s, exec" % SAVE,
        "s_mov_b64 exec, %s" % ROT,
        "ds_write2_b64 %%[amine], %s, %s offset1:1" % (pair(X0), pair(X1)),
        "ds_write_b64 %%[amine], %s offset:16" % pair(X2),
        "s_mov_b64 exec, %s" % SAVE,
    ]


def decode(e, sbe):
    """The pair of the step whose entry is in `e` (sweep base `sbe`): lane mask VALID, partner addresses, sign, sweep bit;
    then the partner's row and W are requested."""
    return [
        "v_and_b32 %s, 15, %s" % (v(TMP), v(e)),
        "v_cmp_ne_u32 vcc, %s, %s" % (v(TMP), v(QI)),
        "s_and_b64 %s, vcc, %s" % (VALID, ACT),
        "v_add_u32 %s, %s, %%[base]" % (v(TMP), v(TMP)),
        "v_cndmask_b32_e64 %s, %s, %s, %s" % (v(TMP), v(ROW), v(TMP), VALID),
        "v_lshl_add_u32 %s, %s, 7, %%[axch]" % (v(AP), v(TMP)),
        "v_and_b32 %s, 0x80000000, %s" % (v(SGN), v(e)),
        "v_bfe_u32 %s, %s, 5, 2" % (v(TMP2), v(e)),
        "v_add_u32 %s, %s, %s" % (v(TMP2), v(TMP2), v(sbe)),
        "v_lshlrev_b32 %s, %s, %s" % (v(SWBIT), v(TMP2), v(ONEI)),
        "ds_read_b128 v[%d:%d], %s" % (PLO, PLO + 3, v(AP)),
        "ds_read_b64 %s, %s offset:16" % (pair(P2), v(AP)),
    ]


def program(M):
    o = []
    a = o.append
    # ---- set-up
    for dst, src in ((X0, "%[x0]"), (X1, "%[x1]"), (X2, "%[x2]")):
        a("v_mov_b64 %s, %s" % (pair(dst), src))
    a("v_mov_b64 %s, 1.0" % pair(ONE))
    a("v_mov_b32 %s, 1" % v(ONEI))
    a("v_mov_b32 %s, %%[e0]" % v(E))
    a("v_mov_b32 %s, %%[e1]" % v(E1))
    a("v_mov_b32 %s, %%[e1]" % v(E2))
    a("v_mov_b32 %s, %%[tt]" % v(TT))
    a("v_mov_b32 %s, %%[tp]" % v(TP))
    a("v_mov_b32 %s, %%[sb]" % v(SB))
    a("v_mov_b32 %s, 0" % v(SBE))
    a("v_mov_b32 %s, %%[sb]" % v(SBE1))
    a("v_and_b32 %s, 0xff, %%[cfg]" % v(STEPS))
    a("v_bfe_u32 %s, %%[cfg], 8, 8" % v(PRO))
    a("v_lshrrev_b32 %s, 16, %%[cfg]" % v(TSTEP))
    a("v_and_b32 %s, 15, %%[lane]" % v(ROW))
    a("v_sub_u32 %s, %s, %%[base]" % (v(QI), v(ROW)))
    a("v_cmp_ne_u32 %s, 0, %%[act]" % ACT)
    a("s_nop 1")
    o += decode(E, SBE)
    a("s_cmp_lg_u64 %s, 0" % ACT)
    a("s_cbranch_scc0 L_done_%=")
    # ---- the step loop
    a(".p2align %d" % LOOP_ALIGN)                    # the loop's address relative to the fetch lines must not depend on the code in front of it
    for _ in range(LOOP_NOPS):
        a("s_nop 0")
    a("L_loop_%=:")
    a("s_waitcnt lgkmcnt(2)")                      # the entry requested a step ago has arrived
    a("v_mov_b32 %s, %s" % (v(E1), v(E2)))
    a("v_add_u32 %s, 1, %s" % (v(TT), v(TT)))
    a("v_add_u32 %s, %s, %s" % (v(TP), v(TP), v(TSTEP)))
    a("v_cmp_eq_u32 vcc, %s, %s" % (v(TT), v(STEPS)))
    a("s_nop 1")
    a("v_cndmask_b32 %s, %s, %s, vcc" % (v(TT), v(TT), v(PRO)))
    a("v_cndmask_b32 %s, %s, %%[twrap], vcc" % (v(TP), v(TP)))
    a("v_addc_co_u32 %s, vcc, 0, %s, vcc" % (v(SB), v(SB)))
    a("ds_read_b32 %s, %s" % (v(E2), v(TP)))
    o += pair_test(M)
    o += decide()
    a("s_cbranch_scc0 L_skip_%=")
    o += rotation(SGN)
    o += commit()
    a("v_cndmask_b32_e64 %s, 0, %s, %s" % (v(TMP), v(SWBIT), ROT))
    a("v_or_b32 %%[chg], %%[chg], %s" % v(TMP))
    o += write_back()
    a("L_skip_%=:")
    # the next step's pair (requested before the bookkeeping: more instructions between the request and the use)
    o += decode(E1, SBE1)
    # sweep bookkeeping
    a("v_and_b32 %s, 0x80, %s" % (v(TMP), v(E)))
    a("v_cmp_ne_u32 vcc, 0, %s" % v(TMP))
    a("s_and_b64 %s, vcc, %s" % (CL, ACT))
    a("s_cbranch_scc0 L_open_%=")
    a("v_bfe_u32 %s, %s, 8, 2" % (v(TMP), v(E)))
    a("v_add_u32 %s, %s, %s" % (v(TMP), v(TMP), v(SBE)))          # the sweep that is complete
    a("v_lshrrev_b32 %s, %s, %%[chg]" % (v(TMP2), v(TMP)))
    a("v_and_b32 %s, 1, %s" % (v(TMP2), v(TMP2)))
    a("v_cmp_ne_u32 vcc, 0, %s" % v(TMP2))
    a("s_and_b64 %s, vcc, %s" % (ST, CL))                        # rows (of closing problems) that rotated in it
    a("v_mov_b32 %s, s70" % v(TMP2))
    a("v_and_b32 %s, %s, %%[pm]" % (v(TMP2), v(TMP2)))
    a("v_cmp_eq_u32 vcc, 0, %s" % v(TMP2))                       # no row of my problem did: JacobiSVDImpl_ stops
    a("v_cmp_le_u32 %s, 24, %s" % (ST, v(TMP)))                   # 25 sweeps: not reproduced here (flag)
    a("s_or_b64 vcc, vcc, %s" % ST)
    a("s_and_b64 vcc, vcc, %s" % CL)
    a("s_andn2_b64 %s, %s, vcc" % (ACT, ACT))
    a("s_and_b64 %s, %s, %s" % (ST, ST, CL))
    a("v_cndmask_b32_e64 %s, 0, 1, %s" % (v(TMP), ST))
    a("v_or_b32 %%[flag], %%[flag], %s" % v(TMP))
    a("s_and_b64 %s, %s, %s" % (VALID, VALID, ACT))      # a problem that has just stopped takes no part in the next step
    a("L_open_%=:")
    a("v_mov_b32 %s, %s" % (v(E), v(E1)))
    a("v_mov_b32 %s, %s" % (v(SBE), v(SBE1)))
    a("v_mov_b32 %s, %s" % (v(SBE1), v(SB)))
    a("s_cmp_lg_u64 %s, 0" % ACT)
    a("s_cbranch_scc1 L_loop_%=")
    a("L_done_%=:")
    a("s_waitcnt lgkmcnt(0)")
    for dst, src in (("%[x0]", X0), ("%[x1]", X1), ("%[x2]", X2)):
        a("v_mov_b64 %s, %s" % (dst, pair(src)))
    return [l.replace('%%[', '%[') for l in o]


# ---- M = 12: the schedule unrolled ------------------------------------------------------------------------------------
# The 12-row schedule (tools/gen_jacobi_schedule.py) is PRO prologue steps followed by PER steps that repeat with the sweep base
# one higher each time.  What a step's table entry says depends on the lane and the step only, so the loop is emitted as one copy
# of the step body per step: the prologue copies, then - aligned, L_loop - the copies of the period.
#   slot j = the j-th step of the period.  Per lane and slot two registers are filled ONCE per solve, before the first step, from
#   the table in LDS: U_AP[j] the address of the partner's row in the exchange (the lane's own row where it idles or its row belongs
#   to no problem) and U_K[j] = bit 31: the lane's row is the pair's second row | bits 0-1: the pair's sweep relative to the base.
#   A prologue step is the slot PER - PRO steps further on with fewer pairs: its valid lanes have the same partner and sign there and
#   belong to sweep 0 (checked below), so prologue copies use that slot's registers and the constant sweep bit 1.
#   VALID of a step = its lanes with a partner (a 16-bit constant per step, the same in every lane group) & ACT.
#   U_BB = 1 << sweep base, doubled where a copy closes a sweep; only those copies carry the sweep bookkeeping and the exit test.
U_AP = list(range(234, 246))
U_K = [158, 159, 176, 177, 178, 179, 246, 247, 248, 249, 250, 251]
U_SGN, U_TMP, U_BB, U_TMP2 = 252, 253, 254, 255
U_ROW, U_QI = N0, N1                 # set-up only


class Unrolled:
    """The constants of the unrolled M = 12 program, from the schedule alone (tests/test_jacobi_unrolled.py walks them)."""

    def __init__(self):
        import gen_jacobi_schedule
        self.n = 12
        self.tab, self.pro, self.per = gen_jacobi_schedule.table(12, 12)
        self.steps = self.pro + self.per
        assert self.per == len(U_AP) == len(U_K)
        assert self.pro <= self.per

    # what the table says about (step, row)
    def partner(self, t, r):
        return self.tab[t][r] & 15

    def has_pair(self, t, r):
        return self.partner(t, r) != r

    def second(self, t, r):
        return (self.tab[t][r] >> 4) & 1

    def srel(self, t, r):
        return (self.tab[t][r] >> 5) & 3

    def closes(self, t):
        """None, or the sweep (relative to the base) that is complete after step t."""
        e = self.tab[t][0]
        return ((e >> 8) & 3) if e & 0x80 else None

    # what the unrolled program uses
    def copies(self):
        """Execution order: every step once, then the period again and again."""
        return list(range(self.steps))

    def next_copy(self, t):
        return t + 1 if t + 1 < self.steps else self.pro

    def slot(self, t):
        """The slot whose registers the copy of step t reads."""
        return t - self.pro if t >= self.pro else t + self.per - self.pro

    def slot_step(self, j):
        """The step whose table entries fill slot j."""
        return self.pro + j

    def valid16(self, t):
        """Bit r: row r has a partner in step t."""
        return sum(1 << r for r in range(self.n) if self.has_pair(t, r))

    def lane_constants(self, t, lane):
        """(partner row, valid, second row of the pair, sweep relative to the base of the copy's period, closing sweep or None) the
        copy of step t uses in `lane`; the base of the prologue's copies is that of the first period."""
        r = lane & 15
        if r >= self.n:
            return r, False, 0, 0, self.closes(t)
        ts = self.slot_step(self.slot(t))
        valid = bool(self.valid16(t) >> r & 1)
        srel = self.srel(ts, r) if t >= self.pro else 0
        return (self.partner(ts, r) if valid else r), valid, self.second(ts, r), srel, self.closes(t)

    def check(self):
        for t in range(self.pro):          # a prologue step = its slot with fewer pairs, all of sweep 0
            ts = self.slot_step(self.slot(t))
            assert self.closes(t) is None
            for r in range(self.n):
                if self.has_pair(t, r):
                    assert self.partner(t, r) == self.partner(ts, r) and self.second(t, r) == self.second(ts, r)
                    assert self.srel(t, r) == 0 and self.srel(ts, r) == 1
        for t in range(self.steps):
            assert self.closes(t) in (None, 0)     # U_BB is the bit of the sweep a closing copy completes
        assert self.closes(self.steps - 1) == 0    # the loop's backward branch sits behind a closing copy


def decode12(u, t):
    """VALID of step t; its partner rows are requested."""
    m = u.valid16(t)
    lit = "0x%08x" % (m | m << 16)
    ap = U_AP[u.slot(t)]
    return [
        "s_and_b32 s62, s60, %s" % lit,
        "s_and_b32 s63, s61, %s" % lit,
        "ds_read_b128 v[%d:%d], %s" % (PLO, PLO + 3, v(ap)),
        "ds_read_b64 %s, %s offset:16" % (pair(P2), v(ap)),
    ]


# ---- M = 12: the step body rescheduled around its dependent chain ---------------------------------------------------------
# A step is one dependent chain (sums -> decision -> two divisions and two square roots -> row update) and is bound by that chain,
# not by issue - and the chain has no idle issue slots to speak of: every instruction woven into it cost its own issue time when
# measured.  So the functions below emit the SAME floating-point operations on the same operands as pair_test / decide / rotation -
# no operation on a committed value is added, removed, reordered within a sum or rounded differently - in an order that takes work
# the chain does not need out of its way, WITHOUT adding instructions to the rotating path.  Three items (ITEMS12; each can be
# left out for measurements: JACOBI12_ITEMS=, =1, =12 ...; figures in docs/NEXT_ROUNDS.md):
#   1  the lane's own-row sum WW = sum x[k]^2 needs nothing from the partner: its three DMFMAs run in front of the wait for the
#      partner's row, in the shadow of the LDS round trip, and six DMFMAs instead of nine follow the wait.
#   2  2p, beta = WW - WP, the |2p| > |beta| select and the first reciprocal of the rotation need P, WW and WP only: they are
#      issued speculatively between decide()'s instructions, and decide()'s scalar mask logic and both branches sit behind the
#      reciprocal and its first refinement steps, whose latency they would otherwise wait out.  2p goes to a register of its own
#      (P2X): the undecided path still reads |P|.  The select's lane mask is CL (free between two sweep closings), the exact
#      threshold's nsqrt keeps Y / H / RR / D to itself (the prefix uses RCP / ERR / HI / LO / BETA / P2X).  Where no lane rotates
#      the prefix is dropped; lanes outside ROT compute garbage (rcp(0), 0/0) that reaches no committed register: commit, chg and
#      the write-back go by ROT as before.
#   3  c and s are R1 and R2 or R2 and R1 by the sign of beta, which is known from the start: the compare takes the wait state
#      behind the last division's reciprocal (an s_nop before) instead of standing, with two wait states of its own, between the
#      division and the row update.
ITEMS12 = frozenset(int(c) for c in os.environ.get("JACOBI12_ITEMS", "123"))
P2X = CC                             # 2p of the speculative prefix (CC / SS are written behind the last division)


def pair_test12(items):
    if 1 not in items:
        return pair_test(12, wait=0)
    wa, wb, p = pair(WW), pair(WP), pair(P)
    regs = ((T0, U0, V0, X0, Q0), (T1, U1, V1, X1, Q1), (T2, U2, V2, X2, P2))
    out = ["v_mul_f64 %s, %s, %s" % (pair(u), pair(x), pair(x)) for t, u, w, x, y in regs]
    out += [mfma(wa, pair(U0), "0"), "s_nop 3", mfma(wa, pair(U1), wa), "s_nop 3", mfma(wa, pair(U2), wa)]
    out.append("s_waitcnt lgkmcnt(0)")             # the partner's row (requested at the end of the previous step)
    for t, u, w, x, y in regs:
        out += ["v_mul_f64 %s, %s, %s" % (pair(t), pair(x), pair(y)), "v_mul_f64 %s, %s, %s" % (pair(w), pair(y), pair(y))]
    for q, (t, u, w, x, y) in enumerate(regs):
        c = (lambda r: "0") if q == 0 else (lambda r: r)
        if q:
            out.append("s_nop 2")
        out += [mfma(wb, pair(w), c(wb)), mfma(p, pair(t), c(p))]
    out.append("s_nop 4")     # 6 wait states between a chain's last DMFMA and the VALU read of its sum (WP first, P two instructions on)
    return out


def decide_rotate12(tag, items):
    """From the sums to the rotated row N0..N2 (rotating lanes: ROT; SCC clear at L_skip_<tag>: nobody rotates)."""
    p2 = P2X if 2 in items else P
    hi, lo = "|%s|" % pair(HI), "|%s|" % pair(LO)
    nd1 = ndiv(pair(QQ), lo, hi)

    def prefix(mask, e64):
        cm = (lambda d, f, t_: "v_cndmask_b32_e64 %s, %s, %s, %s" % (v(d), v(f), v(t_), mask)) if e64 else \
             (lambda d, f, t_: "v_cndmask_b32 %s, %s, %s, vcc" % (v(d), v(f), v(t_)))
        return [
            "v_add_f64 %s, %s, %s" % (pair(p2), pair(P), pair(P)),
            "v_add_f64 %s, %s, -%s" % (pair(BETA), pair(WW), pair(WP)),
            "v_xor_b32 %s, %s, %s" % (v(BETA + 1), v(BETA + 1), v(U_SGN)),
            "v_cmp_gt_f64 %s, |%s|, |%s|" % (mask, pair(p2), pair(BETA)),
        ], [cm(HI, BETA, p2), cm(HI + 1, BETA + 1, p2 + 1), cm(LO, p2, BETA), cm(LO + 1, p2 + 1, BETA + 1)]

    if 2 in items:
        (a2p, abeta, axor, acmp), sel = prefix(CL, True)
        d = decide(tag)
        k = d.index("s_cbranch_scc0 L_decided_%s%%=" % tag)
        dm, dcmp1, dcmp2, dsor, dsandn = d[0:4], d[4], d[5], d[6], d[7]
        assert k == 8 and d[-1].startswith("s_and_b64 %s" % ROT)
        o = [abeta, dm[0], a2p, dm[1], axor, dm[2], acmp, dm[3], dcmp1, dcmp2] + sel
        # (the two scalar instructions are the wait state behind the reciprocal)
        o += [nd1[0], dsor, dsandn, nd1[2], d[k]] + d[k + 1:-1] + [d[-1], nd1[3], "s_cbranch_scc0 L_skip_%s%%=" % tag] + nd1[4:]
    else:
        (a2p, abeta, axor, acmp), sel = prefix("vcc", False)
        o = decide(tag) + ["s_cbranch_scc0 L_skip_%s%%=" % tag, a2p, abeta, axor, acmp, "s_nop 1"] + sel + nd1
    o += ["v_mul_f64 %s, %s, %s" % (pair(TA), pair(QQ), pair(QQ)), "v_add_f64 %s, %s, 1.0" % (pair(TA), pair(TA))]
    o += nsqrt(pair(TB), pair(TA))
    o += ["v_mul_f64 %s, %s, %s" % (pair(GAM), hi, pair(TB)),
          "v_add_f64 %s, %s, |%s|" % (pair(TA), pair(GAM), pair(BETA)),
          "v_add_f64 %s, %s, %s" % (pair(TC), pair(GAM), pair(GAM))]
    o += ndiv(pair(QQ), pair(TA), pair(TC))
    o += nsqrt(pair(R1), pair(QQ))
    o += ["v_mul_f64 %s, %s, %s" % (pair(TA), pair(GAM), pair(R1)), "v_add_f64 %s, %s, %s" % (pair(TA), pair(TA), pair(TA))]
    last = ndiv(pair(R2), pair(p2), pair(TA))
    sign = "v_cmp_gt_f64 vcc, 0, %s" % pair(BETA)
    if 3 in items:
        assert last[1] == "s_nop 0"
        last[1] = sign
        o += last
    else:
        o += last + [sign, "s_nop 1"]
    o += ["v_cndmask_b32 %s, %s, %s, vcc" % (v(SS), v(R2), v(R1)), "v_cndmask_b32 %s, %s, %s, vcc" % (v(SS + 1), v(R2 + 1), v(R1 + 1)),
          "v_cndmask_b32 %s, %s, %s, vcc" % (v(CC), v(R1), v(R2)), "v_cndmask_b32 %s, %s, %s, vcc" % (v(CC + 1), v(R1 + 1), v(R2 + 1)),
          "v_xor_b32 %s, %s, %s" % (v(SS + 1), v(SS + 1), v(U_SGN))]
    rows = ((N0, X0, Q0, T0), (N1, X1, Q1, T1), (N2, X2, P2, T2))
    for n_, x_, q_, t_ in rows:
        o += ["v_mul_f64 %s, %s, %s" % (pair(n_), pair(CC), pair(x_)), "v_mul_f64 %s, %s, %s" % (pair(t_), pair(SS), pair(q_))]
    o += ["v_add_f64 %s, %s, %s" % (pair(n_), pair(n_), pair(t_)) for n_, x_, q_, t_ in rows]
    return o


def program12(prev=False, items=None):
    """prev: the block as it was before the step body was rescheduled (EO_JACOBI_ASM_12_PREV, built with -DEO_JACOBI12_PREV)."""
    items = ITEMS12 if items is None else frozenset(items)
    u = Unrolled()
    u.check()
    o = []
    a = o.append
    # ---- set-up
    for dst, src in ((X0, "%[x0]"), (X1, "%[x1]"), (X2, "%[x2]")):
        a("v_mov_b64 %s, %s" % (pair(dst), src))
    a("v_mov_b64 %s, 1.0" % pair(ONE))
    a("v_mov_b32 %s, 1" % v(U_BB))
    for j in range(u.per):                         # the lane's entries of the period's steps
        a("ds_read_b32 %s, %%[tper] offset:%d" % (v(U_K[j]), 4 * u.n * j))
    a("v_and_b32 %s, 15, %%[lane]" % v(U_ROW))
    a("v_sub_u32 %s, %s, %%[base]" % (v(U_QI), v(U_ROW)))
    a("v_cmp_ne_u32 %s, 0, %%[act]" % ACT)
    a("s_waitcnt lgkmcnt(0)")
    for j in range(u.per):
        e, ap = U_K[j], U_AP[j]
        a("v_and_b32 %s, 15, %s" % (v(U_TMP), v(e)))
        a("v_cmp_ne_u32 vcc, %s, %s" % (v(U_TMP), v(U_QI)))
        a("s_and_b64 %s, vcc, %s" % (VALID, ACT))
        a("v_add_u32 %s, %s, %%[base]" % (v(U_TMP), v(U_TMP)))
        a("v_cndmask_b32_e64 %s, %s, %s, %s" % (v(U_TMP), v(U_ROW), v(U_TMP), VALID))
        a("v_lshl_add_u32 %s, %s, 7, %%[axch]" % (v(ap), v(U_TMP)))
        a("v_bfe_u32 %s, %s, 5, 2" % (v(U_TMP), v(e)))
        a("v_and_b32 %s, 0x80000000, %s" % (v(e), v(e)))
        a("v_or_b32 %s, %s, %s" % (v(e), v(e), v(U_TMP)))
    o += decode12(u, 0)
    a("s_cmp_lg_u64 %s, 0" % ACT)
    a("s_cbranch_scc0 L_done_%=")
    # ---- the steps
    for t in u.copies():
        k = U_K[u.slot(t)]
        if t == u.pro:
            a(".p2align %d" % LOOP_ALIGN)            # the loop's address relative to the fetch lines must not depend on the code in front of it
            for _ in range(LOOP_NOPS):
                a("s_nop 0")
            a("L_loop_%=:")
        if prev:
            o += pair_test(12, wait=0)
            o += decide("%d_" % t)
            a("s_cbranch_scc0 L_skip_%d_%%=" % t)
            a("v_and_b32 %s, 0x80000000, %s" % (v(U_SGN), v(k)))
            o += rotation(U_SGN)
        else:
            a("v_and_b32 %s, 0x80000000, %s" % (v(U_SGN), v(k)))
            o += pair_test12(items)
            o += decide_rotate12("%d_" % t, items)
        o += commit()
        if t >= u.pro:
            a("v_lshlrev_b32 %s, %s, %s" % (v(U_TMP), v(k), v(U_BB)))      # 1 << (base + the pair's relative sweep)
            a("v_cndmask_b32_e64 %s, 0, %s, %s" % (v(U_TMP), v(U_TMP), ROT))
        else:
            a("v_cndmask_b32_e64 %s, 0, 1, %s" % (v(U_TMP), ROT))           # sweep 0
        a("v_or_b32 %%[chg], %%[chg], %s" % v(U_TMP))
        o += write_back()
        a("L_skip_%d_%%=:" % t)
        # the next step's pair (requested before the bookkeeping: more instructions between the request and the use)
        o += decode12(u, u.next_copy(t))
        if u.closes(t) is None:
            continue
        # sweep bookkeeping: the sweep of U_BB is complete
        a("s_mov_b64 %s, %s" % (CL, ACT))
        a("v_and_b32 %s, %%[chg], %s" % (v(U_TMP2), v(U_BB)))
        a("v_cmp_ne_u32 vcc, 0, %s" % v(U_TMP2))
        a("s_and_b64 %s, vcc, %s" % (ST, CL))                        # rows (of closing problems) that rotated in it
        a("v_mov_b32 %s, s70" % v(U_TMP2))
        a("v_and_b32 %s, %s, %%[pm]" % (v(U_TMP2), v(U_TMP2)))
        a("v_cmp_eq_u32 vcc, 0, %s" % v(U_TMP2))                     # no row of my problem did: JacobiSVDImpl_ stops
        a("v_lshrrev_b32 %s, 24, %s" % (v(U_TMP), v(U_BB)))
        a("v_cmp_ne_u32 %s, 0, %s" % (ST, v(U_TMP)))                  # 25 sweeps: not reproduced here (flag)
        a("s_or_b64 vcc, vcc, %s" % ST)
        a("s_and_b64 vcc, vcc, %s" % CL)
        a("s_andn2_b64 %s, %s, vcc" % (ACT, ACT))
        a("s_and_b64 %s, %s, %s" % (ST, ST, CL))
        a("v_cndmask_b32_e64 %s, 0, 1, %s" % (v(U_TMP), ST))
        a("v_or_b32 %%[flag], %%[flag], %s" % v(U_TMP))
        a("s_and_b64 %s, %s, %s" % (VALID, VALID, ACT))      # a problem that has just stopped takes no part in the next step
        a("v_lshlrev_b32 %s, 1, %s" % (v(U_BB), v(U_BB)))
        a("s_cmp_lg_u64 %s, 0" % ACT)
        a("s_cbranch_scc1 L_loop_%=" if u.next_copy(t) == u.pro else "s_cbranch_scc0 L_done_%=")
    a("L_done_%=:")
    a("s_waitcnt lgkmcnt(0)")
    for dst, src in (("%[x0]", X0), ("%[x1]", X1), ("%[x2]", X2)):
        a("v_mov_b64 %s, %s" % (dst, pair(src)))
    return [l.replace('%%[', '%[') for l in o]


# ---- M = 3, three-row problems only: the rows in registers --------------------------------------------------------------
# Every caller of jacobi_rows<3> passes three-row problems.  Their cyclic order is (0, 1), (0, 2), (1, 2) - one pair per step, the
# third closes the sweep - so the block is three copies of the step body with the pair fixed per copy.  Lane 16 g + r belongs to
# the problem row r belongs to and holds columns g and 4 + g of ALL THREE rows of that problem (R3[row][column group], read by the
# block from S.jr; the lanes of a problem hold identical copies and take identical decisions): both rows of a pair are in the
# lane, nothing goes through LDS between the first step and the last, no table, no exec change, no sign register.  The column
# sums work as in the other layouts (the DMFMA adds the four lane groups of a row; every row of the problem gets the same sum);
# columns 8 + g of the row are not rotated along - no caller reads a column >= 6 of a three-row problem.
#   s66: sweeps completed (uniform: the problems side by side run their sweeps in step), CL: lanes whose problem rotated in the
#   sweep under way, ACT: lanes whose problem is still iterating - stands for VALID as well.  Only copy 2 carries the bookkeeping.
R3 = [[234, 236], [238, 240], [242, 244]]      # [row][column group] -> register pair
R3_QI, R3_TMP = 246, 247
R3_N = [[N0, N1], [N2, V0]]                    # the rotated rows i, j of the pair per column group
R3_T = [[T0, T1], [T2, U0]]
R3_PAIRS = [(0, 1), (0, 2), (1, 2)]
R3_SWEEPS = "s66"
R3_MAX_SWEEPS = 25


def program3r():
    o = []
    a = o.append
    # ---- set-up
    a("v_mov_b64 %s, 1.0" % pair(ONE))
    for i in range(3):                             # the problem's three rows: columns g and 4 + g (row stride 16 doubles)
        a("ds_read2_b64 v[%d:%d], %%[ajr] offset0:%d offset1:%d" % (R3[i][0], R3[i][0] + 3, 16 * i, 16 * i + 4))
    a("v_and_b32 %s, 15, %%[lane]" % v(R3_QI))
    a("v_sub_u32 %s, %s, %%[base]" % (v(R3_QI), v(R3_QI)))
    a("v_cmp_ne_u32 %s, 0, %%[act]" % ACT)
    a("s_mov_b64 %s, 0" % CL)
    a("s_mov_b32 %s, 0" % R3_SWEEPS)
    a("s_waitcnt lgkmcnt(0)")
    a("s_cmp_lg_u64 %s, 0" % ACT)
    a("s_cbranch_scc0 L_done_%=")
    a(".p2align %d" % LOOP_ALIGN)
    a("L_loop_%=:")
    for k, (i, j) in enumerate(R3_PAIRS):
        ai, aj = R3[i], R3[j]
        # p = sum_k Ai[k] Aj[k], W[i], W[j] over the A columns (column group 0, V's column masked by mk): pair_test(3) with both rows at hand
        a("v_mul_f64 %s, %s, %s" % (pair(U0), pair(ai[0]), pair(ai[0])))
        a("v_mul_f64 %s, %s, %s" % (pair(T0), pair(ai[0]), pair(aj[0])))
        a("v_mul_f64 %s, %s, %s" % (pair(V0), pair(aj[0]), pair(aj[0])))
        for r in (T0, U0, V0):
            a("v_mul_f64 %s, %s, %%[mk]" % (pair(r), pair(r)))
        a("s_nop 0")
        o += [mfma(pair(WW), pair(U0), "0"), mfma(pair(WP), pair(V0), "0"), mfma(pair(P), pair(T0), "0")]
        a("s_nop 4")
        o += decide("%d_" % k, valid=ACT)
        a("s_cbranch_scc0 L_skip_%d_%%=" % k)
        o += rotation_cs(None)
        for c in range(2):                         # t0 = c Ai + s Aj
            a("v_mul_f64 %s, %s, %s" % (pair(R3_N[0][c]), pair(CC), pair(ai[c])))
            a("v_mul_f64 %s, %s, %s" % (pair(R3_T[0][c]), pair(SS), pair(aj[c])))
        for c in range(2):                         # t1 = -s Ai + c Aj
            a("v_mul_f64 %s, -%s, %s" % (pair(R3_T[1][c]), pair(SS), pair(ai[c])))
            a("v_mul_f64 %s, %s, %s" % (pair(R3_N[1][c]), pair(CC), pair(aj[c])))
        for c in range(2):
            a("v_add_f64 %s, %s, %s" % (pair(R3_N[0][c]), pair(R3_N[0][c]), pair(R3_T[0][c])))
        for c in range(2):
            a("v_add_f64 %s, %s, %s" % (pair(R3_N[1][c]), pair(R3_T[1][c]), pair(R3_N[1][c])))
        for row, regs in ((0, ai), (1, aj)):       # the problems that rotate take the rotated rows
            for c in range(2):
                for h in range(2):
                    a("v_cndmask_b32_e64 %s, %s, %s, %s" % (v(regs[c] + h), v(regs[c] + h), v(R3_N[row][c] + h), ROT))
        a("s_or_b64 %s, %s, %s" % (CL, CL, ROT))
        a("L_skip_%d_%%=:" % k)
    # sweep bookkeeping: a problem none of whose pairs rotated in the sweep stops; sweep 25 is not reproduced here (flag)
    a("s_mov_b64 %s, %s" % (ST, ACT))
    a("s_and_b64 %s, %s, %s" % (ACT, ACT, CL))
    a("s_mov_b64 %s, 0" % CL)
    a("s_add_u32 %s, %s, 1" % (R3_SWEEPS, R3_SWEEPS))
    a("s_cmp_lt_u32 %s, %d" % (R3_SWEEPS, R3_MAX_SWEEPS))
    a("s_cbranch_scc1 L_more_%=")
    a("v_cndmask_b32_e64 %s, 0, 1, %s" % (v(R3_TMP), ST))
    a("v_or_b32 %%[flag], %%[flag], %s" % v(R3_TMP))
    a("s_mov_b64 %s, 0" % ACT)
    a("L_more_%=:")
    a("s_cmp_lg_u64 %s, 0" % ACT)
    a("s_cbranch_scc1 L_loop_%=")
    a("L_done_%=:")
    # the lane's own row (row q = r - base of its problem) goes out as the table-driven block leaves it
    for dst, c in ((X0, 0), (X1, 1)):
        a("v_mov_b64 %s, %s" % (pair(dst), pair(R3[0][c])))
    for q in (1, 2):
        a("v_cmp_eq_u32 vcc, %d, %s" % (q, v(R3_QI)))
        a("s_nop 1")
        for dst, c in ((X0, 0), (X1, 1)):
            for h in range(2):
                a("v_cndmask_b32 %s, %s, %s, vcc" % (v(dst + h), v(dst + h), v(R3[q][c] + h)))
    a("v_mov_b32 %%[chg], %s" % R3_SWEEPS)          # diagnostics (EO_PROFILE): sweeps the loop ran
    for dst, src in (("%[x0]", X0), ("%[x1]", X1)):
        a("v_mov_b64 %s, %s" % (dst, pair(src)))
    return [l.replace('%%[', '%[') for l in o]


def emit(name, lines):
    print("#define EO_JACOBI_ASM_%s \\" % name)
    for i, l in enumerate(lines):
        end = " \\" if i + 1 < len(lines) else ""
        print('  "%s\\n\\t"%s' % (l, end))
    print("")


def main(prev=False):
    """The committed header; prev: csrc/svo_epnp_ord_asm_prev.h instead - the former M = 12 block alone, under the name
    EO_JACOBI_ASM_12_PREV (a build product: tools/Makefile writes it for the -DEO_JACOBI12_PREV builds)."""
    print("// generated by tools/gen_jacobi_asm.py - do not edit")
    if prev:
        print("// The M = 12 step loop of jacobi_rows with the step body in its former instruction order (-DEO_JACOBI12_PREV).")
        emit("12_PREV", program12(prev=True))
        return
    print("// The step loop of jacobi_rows (svo_epnp_ord_dev.h) for M = 12, 6, 3 columns of A, and for M = 3 with the rows in registers (3R); registers v140..v255, s60..s71.")
    for M in (12, 6, 3):
        emit(str(M), program12() if M == 12 else program(M))
    emit("3R", program3r())
    clob = ", ".join('"v%d"' % i for i in range(140, 256)) + ", " + ", ".join('"s%d"' % i for i in range(60, 72)) + ', "vcc", "scc", "memory"'
    print("#define EO_JACOBI_ASM_CLOBBERS " + clob)


if __name__ == "__main__":
    import sys
    main(prev="--prev" in sys.argv[1:])
