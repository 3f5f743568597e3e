"""References of the tests of RANSAC's stopping rule and consensus count (tests/test_pnp_rule_cpu.py, tests/test_pnp_rule_gpu.py):
RANSACPointSetRegistrator::run's loop (OpenCV 3.2 ptsetreg.cpp) restated in Python around the oracle's RANSACUpdateNumIters, the
200-bit margin study of that function's two discrete steps, the hand-made and seeded sample vectors, and PnPRansacCallback::
computeError with explicit float32 steps."""
import json
import os

import numpy as np

import util

MARGINS_PATH = os.path.join(util.GOLDEN, "pnp_rule_margins.json")
NS_ALL = range(6, 513)                 # every n of the exhaustive table: the pairs 5 <= g <= n, 129,285 of them
INT_MAX = 2147483647


def run_rule(cnt, ok, n, update):
    """RANSACPointSetRegistrator::run over precomputed samples: cnt[k] the consensus of sample k, ok[k] whether it gave a model.
    update(ep, maxIters) = RANSACUpdateNumIters(0.99, ep, 5, maxIters).  Returns (best, good, iters, bounds): the winner (-1: none),
    its consensus, the samples visited, and bounds[m] = niters after the first m samples (m = 0 .. 100; the loop's last value
    from where it ended)."""
    if n == 5:                                  # count == modelPoints: one model from the five points, every point an inlier
        return (0, 5, 1, [1] * 101) if ok[0] else (-1, 0, 1, [1] * 101)
    niters, max_good, best, it = 100, 0, -1, 0
    bounds = [100]
    while it < niters:
        if ok[it]:
            g = int(cnt[it])
            if g > max(max_good, 4):
                max_good, best = g, it
                niters = update((n - g) / n, niters)
        it += 1
        bounds.append(niters)
    bounds += [niters] * (101 - len(bounds))
    return best, max_good, it, bounds


def pairs():
    """(g, n) of the exhaustive table, as two int arrays"""
    n = np.concatenate([np.full(k - 4, k) for k in NS_ALL])
    g = np.concatenate([np.arange(5, k + 1) for k in NS_ALL])
    return g, n


def margin_study(dps_bits=200):
    """log(0.01) / log(1 - (g / n)^5) at 200 bits for every pair: its rounding to an integer, and how close it comes to a tie of rint
    (a half-integer; where the quotient is below 100.5 - beyond, the comparison returns maxIters before rint is reached) and to the comparison -num >= niters * (-denom) changing sides (an integer niters in 1 .. 100) - relative to the
    quotient.  Pairs with g == n have denom = 0: the function returns 0 there."""
    import mpmath as mp
    mp.mp.prec = dps_bits
    g, n = pairs()
    num = mp.log(mp.mpf(1) - mp.mpf("0.99"))
    q = np.zeros(len(g)); r = np.zeros(len(g), np.int64)
    tie = (np.inf, None); cmpm = (np.inf, None)
    for i, (gi, ni) in enumerate(zip(g.tolist(), n.tolist())):
        if gi == ni:
            q[i] = np.nan
            continue
        x = mp.mpf(gi) / ni
        qi = num / mp.log(1 - x ** 5)
        q[i] = float(qi)
        ri = int(mp.nint(qi))
        r[i] = min(ri, INT_MAX)
        if qi < 100.5:                           # (rint is only reached where the quotient is below maxIters <= 100)
            m = float(abs(abs(qi - ri) - mp.mpf("0.5")) / qi)
            if m < tie[0]:
                tie = (m, (gi, ni, float(qi)))
        k = min(max(int(mp.nint(qi)), 1), 100)   # the nearest niters the comparison can be asked about
        m = float(abs(qi - k) / k)
        if m < cmpm[0]:
            cmpm = (m, (gi, ni, k))
    return {"g": g, "n": n, "q": q, "r": r, "tie": tie, "cmp": cmpm}


def integers_from_quotient(q, r, niters):
    """RANSACUpdateNumIters' result from the exact quotient q = num / denom (denom < 0): niters if q >= niters, else rint(q); 0 where
    the denominator vanishes (q is NaN)."""
    out = np.where(q >= niters, niters, r)
    return np.where(np.isnan(q), 0, out).astype(np.int64)


def load_margins():
    return json.load(open(MARGINS_PATH))


# ---- sample vectors of the rule ---------------------------------------------------------------------------------------------
def hand_made(update):
    """(name, cnt[100], ok[100], n) - each one a property of the loop placed on purpose"""
    out = []

    def vec(name, n, cnt=None, ok=None):
        c = np.zeros(100, np.int32) if cnt is None else np.asarray(cnt, np.int32)
        o = np.ones(100, np.int32) if ok is None else np.asarray(ok, np.int32)
        out.append((name, c, o, int(n)))
    rng = np.random.default_rng(5)
    vec("nothing ok", 64, rng.integers(5, 65, 100), np.zeros(100))
    c = rng.integers(5, 30, 100); o = np.ones(100); c[17] = 60; o[17] = 0
    vec("a not-ok sample with the largest count", 64, c, o)
    vec("counts <= 4 only", 64, rng.integers(0, 5, 100))
    c = np.zeros(100); c[3] = 5
    vec("count 5 at n = 6", 6, c)
    c = np.zeros(100); c[2] = 20; c[9] = 20; c[30] = 20
    vec("equal counts: the earlier one stays", 64, c)
    for k in (0, 1, 37, 99):
        c = rng.integers(0, 30, 100); c[k] = 64      # (below 30 of 64 the bound stays 100)
        vec("g == n at sample %d" % k, 64, c)
    vec("n == 5, ok", 5, np.full(100, 5))
    vec("n == 5, not ok", 5, np.full(100, 5), np.zeros(100))
    # a strictly better sample exactly at index niters - 1 (visited) and at niters (not visited): sample 0 sets the bound
    n, g0 = 64, 40
    b = update((n - g0) / n, 100)
    assert 2 <= b < 99, b
    for at, what in ((b - 1, "visited"), (b, "not visited")):
        c = np.full(100, 10); c[0] = g0; c[at] = 50
        vec("a better sample at index niters %s (%s)" % ("- 1" if at == b - 1 else "", what), n, c)
    # the two closest margins of the study: the rint tie of (g, n) as the first sample, and the comparison of (g, n, niters) reached
    # through an earlier sample whose bound is that niters
    m = load_margins()
    g, n, _ = m["tie"]["at"]
    c = np.zeros(100); c[0] = g
    vec("closest rint tie (%d, %d)" % (g, n), n, c)
    g, n, k = m["cmp"]["at"]
    # (the quotient falls as g grows, so a bound of exactly k can only come from a smaller g whose quotient rounds to the same k: where
    # none exists the loop cannot ask this comparison at all - the table test evaluates it for every niters directly - and the
    # vector asks the one it can, against the bound of 100)
    first = [h for h in range(5, g) if update((n - h) / n, 100) == k]
    c = np.zeros(100); c[0 if not first else 1] = g
    if first:
        c[0] = first[0]
    vec("closest comparison (%d, %d, %d)%s" % (g, n, k, " after a sample with bound %d" % k if first else ", no smaller consensus has that bound"), n, c)
    return out


def seeded(count=2000, ns=(6, 7, 51, 64, 357, 512), seed=11):
    """count vectors over the given n: consensus values drawn so that the bound shrinks in several steps, a few samples without a
    model, now and then a full consensus"""
    rng = np.random.default_rng(seed)
    cnt = np.zeros((count, 100), np.int32); ok = np.ones((count, 100), np.int32); n = np.zeros(count, np.int32)
    for i in range(count):
        ni = int(ns[i % len(ns)]); n[i] = ni
        kind = (i // len(ns)) % 4
        if kind == 0:                            # uniform over 0 .. n
            c = rng.integers(0, ni + 1, 100)
        elif kind == 1:                          # low counts, slowly rising: many updates, the bound stays high
            c = np.minimum(ni, (rng.random(100) * np.linspace(0.05, 0.6, 100) * ni).astype(np.int64) + rng.integers(0, 6, 100))
        elif kind == 2:                          # around the ratios where the bound falls below 100
            c = np.clip((rng.normal(0.45, 0.12, 100) * ni).astype(np.int64), 0, ni)
        else:                                    # mostly small with one large late
            c = rng.integers(0, max(ni // 4, 6), 100); c[rng.integers(0, 100)] = rng.integers(ni // 2, ni + 1)
        cnt[i] = c
        ok[i] = rng.random(100) > 0.1
    return cnt, ok, n


# ---- PnPRansacCallback::computeError ------------------------------------------------------------------------------------------
def inlier_flags(Xw, obs, K, R, t):
    """projectPoints in double, rounded once to float; the squared distance to the float image point in float; inlier iff <= 64.
    A depth of exactly 0 is projected with scale 1."""
    Xw = np.asarray(Xw, np.float64); obs = np.asarray(obs, np.float64); R = np.asarray(R, np.float64).reshape(3, 3)
    out = np.zeros(len(Xw), np.uint8)
    for i, X in enumerate(Xw):
        x = R[0, 0] * X[0] + R[0, 1] * X[1] + R[0, 2] * X[2] + t[0]
        y = R[1, 0] * X[0] + R[1, 1] * X[1] + R[1, 2] * X[2] + t[1]
        z = R[2, 0] * X[0] + R[2, 1] * X[1] + R[2, 2] * X[2] + t[2]
        z = 1.0 / z if z != 0.0 else 1.0
        x *= z; y *= z
        px = np.float32(x * K[0] + K[2]); py = np.float32(y * K[1] + K[3])
        dx = np.float32(np.float32(obs[i, 0]) - px); dy = np.float32(np.float32(obs[i, 1]) - py)
        err = np.float32(np.float32(dx * dx) + np.float32(dy * dy))
        out[i] = err <= np.float32(64.0)
    return out
