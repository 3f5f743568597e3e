"""Numpy restatement of the sparse stereo matcher (oracle/orc_stereo.c: orc_stereo_match; DESIGN.md, "ComputeStereoMatches"):
row-band candidates, octave and disparity gates, Hamming argmin (first minimum = lowest index), 11 x 11 SAD over +-5 px at the
keypoint's level (first minimum), parabola, the disparity test, the median cut.  One left keypoint at a time, every float32
operation spelled out as one numpy float32 operation, roundf as half away from zero.

Besides uR and depth, match() says per left keypoint HOW it left the matcher (`reason`, one of REASONS - left and right window
tests and each of their sides kept apart), its best SAD before the cut (`sad`, -1: not accepted - the reference for
svo_debug_stereo_match's third output), the candidate the Hamming search found (`cand`, `cand_dist`; -1 / 256: none passed the
gates), and the flags `ham_tie` (two candidates share the least distance), `sad_tie` (two shifts share the least SAD),
`substituted` (disparity <= 0 replaced by 0.01) and `cut` (accepted, then removed by the median cut).  A test uses them to show
that a case reaches the branch it was made for.
"""
import math

import numpy as np

F = np.float32
TH_HIGH, TH_LOW = 100, 50
TH_ORB = (TH_HIGH + TH_LOW) // 2
SAD_W = SAD_L = 5
NLEVELS = 8

REASONS = ("accepted", "maxu_negative", "no_candidate", "hamming_ge_100", "hamming_75_99",
           "left_top", "left_bottom", "left_left", "left_right", "right_left", "right_right",
           "sad_min_first", "sad_min_last", "parabola", "disparity_range")
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def roundf(v):
    """C roundf of a float32: to nearest, halves away from zero (|v| + 0.5 is exact in double)."""
    v = float(v)
    return int(math.copysign(math.floor(abs(v) + 0.5), v))


def geometry(W, H):
    """(w, h, scale) of the 8 levels: scale = (float)pow((double)1.2f, l), sizes = lrintf((float)W * (1.0f / scale))."""
    scale = [F(math.pow(float(F(1.2)), l)) for l in range(NLEVELS)]
    w = [int(np.rint(F(W) * (F(1) / s))) for s in scale]
    h = [int(np.rint(F(H) * (F(1) / s))) for s in scale]
    return w, h, scale


def split_pyramid(pyr, W, H):
    """The packed pyramid (level after level, tight rows) as a list of 2-D arrays."""
    w, h, _ = geometry(W, H)
    out, off = [], 0
    for l in range(NLEVELS):
        out.append(np.asarray(pyr[off:off + w[l] * h[l]]).reshape(h[l], w[l]))
        off += w[l] * h[l]
    return out


def level_coords(x, y, octave, scale):
    """(su, sv): the keypoint's pixel at its level."""
    inv = F(1) / scale[octave]
    return roundf(F(x) * inv), roundf(F(y) * inv)


def match(levL, levR, W, H, kpL, dL, kpR, dR, bf, fx):
    w, h, scale = geometry(W, H)
    nL, nR = len(kpL), len(kpR)
    bf, fx = F(bf), F(fx)
    minD, maxD = F(0), fx
    dL = np.asarray(dL, np.uint8).reshape(-1, 32); dR = np.asarray(dR, np.uint8).reshape(-1, 32)
    minr = np.zeros(nR, np.int64); maxr = np.zeros(nR, np.int64)
    for i in range(nR):
        r = F(2.0) * scale[int(kpR["octave"][i])]
        maxr[i] = math.ceil(float(F(kpR["y"][i]) + r))
        minr[i] = math.floor(float(F(kpR["y"][i]) - r))
    octR = kpR["octave"].astype(np.int64); xR = kpR["x"].astype(np.float32)
    uR = np.full(nL, -1, np.float32); depth = np.full(nL, -1, np.float32); sad = np.full(nL, -1, np.int32)
    reason = np.empty(nL, object)
    cand = np.full(nL, -1, np.int64); cand_dist = np.full(nL, 256, np.int64)
    ham_tie = np.zeros(nL, bool); sad_tie = np.zeros(nL, bool); substituted = np.zeros(nL, bool); cut = np.zeros(nL, bool)
    accepted = []                                     # (best SAD, iL)
    for iL in range(nL):
        levelL = int(kpL["octave"][iL])
        vL, uL = F(kpL["y"][iL]), F(kpL["x"][iL])
        row = int(vL)                                 # (int): towards zero
        minU, maxU = uL - maxD, uL - minD
        if maxU < 0:
            reason[iL] = "maxu_negative"; continue
        gate = ((row >= minr) & (row <= maxr) & (octR >= levelL - 1) & (octR <= levelL + 1) & (xR >= minU) & (xR <= maxU)) \
            if nR else np.zeros(0, bool)
        idx = np.flatnonzero(gate)
        if len(idx) == 0:
            reason[iL] = "no_candidate"; continue
        dist = _POP[dL[iL][None, :] ^ dR[idx]].sum(1)
        k = int(np.argmin(dist))                      # first minimum: the lowest index
        cand[iL], cand_dist[iL] = idx[k], dist[k]
        ham_tie[iL] = (dist == dist[k]).sum() > 1
        if dist[k] >= TH_HIGH:
            reason[iL] = "hamming_ge_100"; continue
        if dist[k] >= TH_ORB:
            reason[iL] = "hamming_75_99"; continue
        uR0 = xR[idx[k]]
        inv = F(1) / scale[levelL]
        su, sv, sr0 = roundf(uL * inv), roundf(vL * inv), roundf(uR0 * inv)
        lw, lh = w[levelL], h[levelL]
        IL, IR = levL[levelL].astype(np.int64), levR[levelL].astype(np.int64)
        if sv - SAD_W < 0:
            reason[iL] = "left_top"; continue
        if sv + SAD_W >= lh:
            reason[iL] = "left_bottom"; continue
        if su - SAD_W < 0:
            reason[iL] = "left_left"; continue
        if su + SAD_W >= lw:
            reason[iL] = "left_right"; continue
        if sr0 - SAD_L - SAD_W < 0:
            reason[iL] = "right_left"; continue
        if sr0 + SAD_L + SAD_W >= lw:
            reason[iL] = "right_right"; continue
        a = IL[sv - SAD_W:sv + SAD_W + 1, su - SAD_W:su + SAD_W + 1] - IL[sv, su]
        dists = []
        for inc in range(-SAD_L, SAD_L + 1):
            c = sr0 + inc
            b = IR[sv - SAD_W:sv + SAD_W + 1, c - SAD_W:c + SAD_W + 1] - IR[sv, c]
            dists.append(int(np.abs(a - b).sum()))
        best, bestinc = 0x7fffffff, 0
        for j, s in enumerate(dists):
            if s < best:
                best, bestinc = s, j - SAD_L
        sad_tie[iL] = dists.count(best) > 1
        if bestinc == -SAD_L:
            reason[iL] = "sad_min_first"; continue
        if bestinc == SAD_L:
            reason[iL] = "sad_min_last"; continue
        d1, d2, d3 = F(dists[SAD_L + bestinc - 1]), F(dists[SAD_L + bestinc]), F(dists[SAD_L + bestinc + 1])
        deltaR = (d1 - d3) / (F(2.0) * (d1 + d3 - F(2.0) * d2))
        if deltaR < -1 or deltaR > 1:
            reason[iL] = "parabola"; continue
        bestuR = scale[levelL] * (F(sr0) + F(bestinc) + deltaR)
        disparity = uL - bestuR
        if not (disparity >= minD and disparity < maxD):
            reason[iL] = "disparity_range"; continue
        if disparity <= 0:
            disparity = F(0.01); bestuR = uL - F(0.01); substituted[iL] = True
        depth[iL] = bf / disparity
        uR[iL] = bestuR
        sad[iL] = best
        reason[iL] = "accepted"
        accepted.append((best, iL))
    if accepted:
        accepted.sort()
        median = F(accepted[len(accepted) // 2][0])
        th = F(2.1) * median
        for s, iL in reversed(accepted):
            if F(s) < th:
                break
            uR[iL] = depth[iL] = -1
            cut[iL] = True
    return dict(uR=uR, depth=depth, sad=sad, reason=reason, cand=cand, cand_dist=cand_dist, ham_tie=ham_tie,
                sad_tie=sad_tie, substituted=substituted, cut=cut)


def tally(res):
    """{reason or flag: count} of one match() result (zero counts left out)."""
    t = {}
    for r in res["reason"]:
        t[r] = t.get(r, 0) + 1
    for f in ("ham_tie", "sad_tie", "substituted", "cut"):
        if res[f].any():
            t[f] = int(res[f].sum())
    kept = int((res["substituted"] & ~res["cut"]).sum())
    if kept:
        t["substituted_kept"] = kept
    return t
