"""Plain references of the semantic gate's matching stages: numpy and pure Python, no project code.

  bf_match_ref      <- find_feature_matches (reference src/pnpmatch.cc:253-300), the contract of svo_bf_match (include/svo.h)
  greedy_gated_ref  <- pass 1 / pass 2 of poseEstimationPnP with the epipolar veto (src/pnpmatch.cc:61-199), the contract of
                       svo_match_greedy_gated (include/svo.h) and of the helpers in csrc/svo_gate.h
  in_boxes_ref, epipolar_distance_ref: the two helpers on their own (float32 points, int boxes, float64 line)

The 8-point reference needs more than float64 and lives in tests/golden/make_fmat_golden.py (mpmath); the helpers that
compare two fundamental matrices up to scale and sign are here, since the CPU and the GPU tests share them."""
import numpy as np

PAD = 10          # src/pnpmatch.cc:103-121
VETO_PX = 0.1     # src/pnpmatch.cc:115


def hamming_matrix(q, t):
    """M x N Hamming distances of 32-byte rows (np.unpackbits)."""
    q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
    t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
    D = np.zeros((len(q), len(t)), np.int64)
    for i in range(len(q)):
        if len(t):
            D[i] = np.unpackbits(np.bitwise_xor(q[i][None, :], t), axis=1).sum(1)
    return D


def bf_match_ref(q, t):
    """(train_idx, dist, keep): nearest train row (first minimum: ties to the lowest index), then
    keep = dist <= max(2 * min, 30) in float64 with min starting at 10000; no train rows: -1 / -1 / 0."""
    D = hamming_matrix(q, t)
    M, N = D.shape
    ti = np.full(M, -1, np.int32); d = np.full(M, -1, np.int32); keep = np.zeros(M, np.uint8)
    if N == 0:
        return ti, d, keep
    ti[:] = np.argmin(D, axis=1)            # np.argmin returns the first minimum
    d[:] = D[np.arange(M), ti]
    mn = min(float(d.min()), 10000.0) if M else 10000.0
    thr = max(2.0 * mn, 30.0)
    keep[:] = d.astype(np.float64) <= thr
    return ti, d, keep


def in_boxes_ref(x, y, boxes, pad=PAD):
    """float32 point against int boxes {left, right, top, bottom} padded by `pad`, strict inequalities.  left - pad is an int;
    the comparison promotes it (|value| < 2^24 here) exactly."""
    x = np.float32(x); y = np.float32(y)
    for left, right, top, bottom in np.asarray(boxes, np.int64).reshape(-1, 4):
        if x > np.float32(left - pad) and x < np.float32(right + pad) and y > np.float32(top - pad) and y < np.float32(bottom + pad):
            return True
    return False


def epipolar_distance_ref(F, last_xy, cur_xy):
    """|l . [cur, 1]| / sqrt(A^2 + B^2) with l = F [last, 1] in float64, float32 points, in the written operation order."""
    F = [np.float64(v) for v in np.asarray(F, np.float64).reshape(9)]
    lx, ly = np.float64(np.float32(last_xy[0])), np.float64(np.float32(last_xy[1]))
    cx, cy = np.float64(np.float32(cur_xy[0])), np.float64(np.float32(cur_xy[1]))
    with np.errstate(invalid="ignore", divide="ignore"):
        A = F[0] * lx + F[1] * ly + F[2]
        B = F[3] * lx + F[4] * ly + F[5]
        Cc = F[6] * lx + F[7] * ly + F[8]
        return np.abs(A * cx + B * cy + Cc) / np.sqrt(A * A + B * B)


def greedy_gated_ref(q, q_skip, t, assigned, max_dist, ratio, q_xy, t_xy, boxes, F):
    """Row-by-row loop of the svo_match_greedy_gated contract.  Returns (best_idx, best, second, accepted, assigned, vetoed,
    info) - info is a list of (row, column, in_box, distance) for every row that passed the descriptor tests, which the case
    generators use (how far a distance is from the threshold, which rows were gated)."""
    D = hamming_matrix(q, t)
    M, N = D.shape
    assigned = np.ascontiguousarray(assigned, np.uint8).copy()
    boxes = np.zeros((0, 4), np.int32) if boxes is None else np.asarray(boxes, np.int32).reshape(-1, 4)
    bi = np.full(M, -1, np.int32); b = np.full(M, 256, np.int32); s = np.full(M, 256, np.int32)
    acc = np.zeros(M, np.uint8); vet = np.zeros(M, np.uint8)
    info = []
    for i in range(M):
        if q_skip is not None and q_skip[i]:
            continue
        best, second, idx = 256, 256, -1
        row = D[i]
        for j in range(N):
            if assigned[j]:
                continue
            if row[j] < best:
                second, best, idx = best, int(row[j]), j
        bi[i], b[i], s[i] = idx, best, second
        if idx < 0:
            continue
        ok = best < max_dist
        if ok and ratio > 0:
            with np.errstate(divide="ignore", invalid="ignore"):
                ok = bool(np.float32(second) / np.float32(best) > np.float32(ratio))
        if ok and len(boxes) > 0:
            inb = in_boxes_ref(t_xy[idx][0], t_xy[idx][1], boxes)
            dist = epipolar_distance_ref(F, q_xy[i], t_xy[idx]) if inb else np.float64(0)
            info.append((i, idx, inb, float(dist)))
            if inb and dist > VETO_PX:          # NaN compares false: no veto
                vet[i] = 1
                ok = False
        if ok:
            acc[i] = 1
            assigned[idx] = 1
    return bi, b, s, acc, assigned, vet, info


# ---- comparing fundamental matrices where the contract leaves scale and sign free ---------------------------------------
def normalise_F(F):
    """Frobenius norm 1, sign fixed by the largest entry (positive)."""
    F = np.asarray(F, np.float64).reshape(3, 3)
    nrm = np.linalg.norm(F)
    if nrm == 0:
        return F.copy()
    F = F / nrm
    k = np.argmax(np.abs(F))
    return F if F.reshape(9)[k] > 0 else -F


def entry_deviation(F, Fref_n):
    """max |F / ||F|| - Fref| over the entries after sign alignment (Fref_n already normalised)."""
    F = np.asarray(F, np.float64).reshape(3, 3)
    Fn = F / np.linalg.norm(F)
    return float(min(np.abs(Fn - Fref_n).max(), np.abs(Fn + Fref_n).max()))


def probe_distances(F, last, cur):
    return np.array([epipolar_distance_ref(F, last[k], cur[k]) for k in range(len(last))])


def probe_deviation(F, Fref, last, cur, spread):
    """The gate's own quantity at the stored probe pairs: max |d(F) - d(Fref)| / (d(Fref) + spread), spread = the points' mean
    distance from their centroid - dimensionless, so that it is comparable with an eigenvector's angle error."""
    d, dr = probe_distances(F, last, cur), probe_distances(Fref, last, cur)
    return float(np.max(np.abs(d - dr) / (dr + spread)))


def design_matrix(p1, p2):
    """Rows of the epipolar constraints p2^T F p1 = 0 for the isotropically normalised points, and the two transforms."""
    def norm(p):
        c = p.mean(0)
        s = np.sqrt(2.0) / np.linalg.norm(p - c, axis=1).mean()
        return (p - c) * s, np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])
    q1, T1 = norm(np.asarray(p1, np.float64)); q2, T2 = norm(np.asarray(p2, np.float64))
    A = np.stack([q2[:, 0] * q1[:, 0], q2[:, 0] * q1[:, 1], q2[:, 0], q2[:, 1] * q1[:, 0], q2[:, 1] * q1[:, 1], q2[:, 1],
                  q1[:, 0], q1[:, 1], np.ones(len(q1))], 1)
    return A, T1, T2


def algebraic_residual(F, p1, p2):
    """||A f|| / ||f|| of F taken back to the normalised frame (f = T2^-T F T1^-1): what the eigenvector minimises."""
    A, T1, T2 = design_matrix(p1, p2)
    Fn = np.linalg.inv(T2).T @ np.asarray(F, np.float64).reshape(3, 3) @ np.linalg.inv(T1)
    f = Fn.reshape(9)
    return float(np.linalg.norm(A @ f) / np.linalg.norm(f))
