"""The pose-free side of a tracked frame, restated in plain Python from the reference's text - a second witness beside the C
oracle (oracle/orc_track.c) for the device's parallel matching scheme (k_ti_lists / k_ti_resolve, csrc/svo_track.hip):

  Tracking::init                 src/Tracking.cc:42-97     a map point for every keypoint with depth > 0
  pass 1                         src/pnpmatch.cc:61-156    last frame's points in keypoint order; first minimum over the unclaimed
                                                           columns in index order; accepted when best < 15 (then the veto)
  pass 2                         src/pnpmatch.cc:159-199   local points in creation order, not bad, not observed by this frame;
                                                           best < 30 && (float)second / (float)best > 2
  frame::createmappoint          src/frame.cc:182-238      depth > 0 and no map point yet
  cull                           src/Tracking.cc:239-250   create_id <= id - 4, from frame 4 on
and the project's own representation of the map: a pool in creation order, stably compacted after every frame to the local
points and the points the last frame references (pool rows are what svo_debug_track_matches and orc_track_tail hand out).

The epipolar veto needs F from the 8-point solve, so it is taken as given: `veto[i, j]` says whether last-frame keypoint i
matched to column j is vetoed.  `nocreate[j]`: keypoint j lies in a padded detection box (+-5 px), no point is created from it.

RULES are the switches of the mutant table (tests/test_index_cpu.py): each turns one rule into a subtly wrong one.

Beside it: `greedy_rounds`, the round scheme of ti_resolve_pass restated on full distance rows (with `rank_blind` its classic
bug), and `list_model`, what k_ti_lists would store, from distances alone."""
import numpy as np

RULES = dict(ratio_ge=False, global_second=False, last_tie=False, claimed_blocks=False, reverse=False, rank_blind=False,
             keep_observed=False, thr1=15, thr2=30, cull_age=4, drop_referenced=False)

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def distances(q, t):
    """Hamming distances of (M, 32) against (N, 32) uint8 descriptors: (M, N) int32."""
    q = np.asarray(q, np.uint8).reshape(-1, 32); t = np.asarray(t, np.uint8).reshape(-1, 32)
    D = np.zeros((len(q), len(t)), np.int32)
    for k in range(32):
        D += _POP[q[:, k, None] ^ t[None, :, k]]
    return D


def scan_row(d, free, rules=RULES):
    """`if (dist < best) { second = best; best = dist; idx = j; }` over the unclaimed columns in index order:
    (idx, best, second); second = the running minimum when the best was met, 256 if it was the first column looked at."""
    cols = np.flatnonzero(free)
    if len(cols) == 0:
        return -1, 256, 256
    dv = d[cols]
    best = int(dv.min())
    p = int(np.flatnonzero(dv == best)[-1 if rules["last_tie"] else 0])
    second = int(dv[:p].min()) if p > 0 else 256
    if rules["global_second"]:
        rest = np.delete(dv, p)
        second = int(rest.min()) if len(rest) else 256
    if rules["claimed_blocks"]:
        before = d[:cols[p]]
        second = int(before.min()) if len(before) else 256
    return int(cols[p]), best, second


def accept(best, second, thr, ratio, rules=RULES):
    if not best < thr:
        return False
    if not ratio:
        return True
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.float32(second) / np.float32(best)          # best = 0: inf (or NaN for 0 / 0, never greater)
    return bool(r >= 2) if rules["ratio_ge"] else bool(r > 2)


def greedy(D, taken, thr, ratio, rules=RULES, veto=None):
    """Rows in order, each claims its best unclaimed column.  Returns ({row: column}, [vetoed rows]); `taken` is updated."""
    out, vetoed = {}, []
    order = range(len(D) - 1, -1, -1) if rules["reverse"] else range(len(D))
    for r in order:
        j, best, second = scan_row(D[r], ~taken, rules)
        if j < 0 or not accept(best, second, thr, ratio, rules):
            continue
        if veto is not None and veto[r, j]:
            vetoed.append(r)
            continue
        taken[j] = True
        out[r] = j
    return out, vetoed


def greedy_rounds(D, taken, thr, ratio, rank_blind=False):
    """The same pass resolved in rounds, as ti_resolve_pass does: every unresolved row looks at the columns that no EARLIER
    row has claimed; it is final when no earlier unresolved row could still claim its best column and - if the ratio rule
    rejects it - one of its blockers cannot be claimed away either.  Returns ({row: column}, rounds).  rank_blind: a row sees
    every claim made so far, also those of later rows that were resolved first (the bug the claimer ranks prevent)."""
    M, N = D.shape
    INF = 1 << 30
    claimer = np.where(taken, -1, INF).astype(np.int64)      # rank of the row that took the column
    unresolved = list(range(M))
    out, rounds = {}, 0
    while unresolved:
        rounds += 1
        minrow = np.full(N, INF, np.int64)
        free = {}
        for k in unresolved:
            f = (claimer == INF) if rank_blind else (claimer > k)
            free[k] = f
            c = f & (D[k] < thr)
            minrow[c] = np.minimum(minrow[c], k)
        nxt, claims = [], []
        for k in unresolved:
            f = free[k]
            j, best, second = scan_row(D[k], f)
            if j < 0 or best >= thr:
                continue                                     # claims only remove columns: never accepted
            ok = accept(best, second, thr, ratio)
            if minrow[j] < k:
                nxt.append(k); continue
            if not ok:
                blockers = np.flatnonzero(f[:j] & (D[k, :j] <= 2 * best))
                if not (minrow[blockers] >= k).any():
                    nxt.append(k); continue
            if ok:
                claims.append((k, j))
        for k, j in claims:
            claimer[j] = k
            out[k] = j
        assert len(nxt) < len(unresolved)                    # the first unresolved row is always final
        unresolved = nxt
    taken |= claimer != INF
    return out, rounds


def list_model(D):
    """What k_ti_lists stores for rows with these distances: per row the number of columns below 30, and per entry
    (column, distance, blockers) with blockers = earlier columns at a distance in [30, 2 d] (counted for d >= 15 only)."""
    ncols = (D < 30).sum(1)
    entries = []
    for r in range(len(D)):
        e = []
        for c in np.flatnonzero(D[r] < 30):
            d = int(D[r, c])
            nb = int(((D[r, :c] >= 30) & (D[r, :c] <= 2 * d)).sum()) if d >= 15 else 0
            e.append((int(c), d, nb))
        entries.append(e)
    return ncols, entries


class Point:
    __slots__ = ("desc", "create_id", "gid", "bad", "local", "seen")

    def __init__(self, desc, create_id, gid):
        self.desc, self.create_id, self.gid, self.bad, self.local, self.seen = desc, create_id, gid, False, True, -1


class Tracker:
    def __init__(self, rounds=False, **rules):
        self.rules = dict(RULES, **rules)
        self.rounds = rounds                  # resolve the passes with greedy_rounds (no veto then)
        self.frame, self.next_gid, self.pool, self.last_mp = 0, 0, [], []
        self.dynamic0 = False

    def _create(self, desc, id):
        p = Point(np.array(desc, np.uint8), id, self.next_gid)
        self.next_gid += 1
        self.pool.append(p)
        return p

    def _pass(self, D, taken, thr, ratio, veto=None):
        if self.rounds or self.rules["rank_blind"]:
            assert veto is None
            out, rounds = greedy_rounds(D, taken, thr, ratio, self.rules["rank_blind"])
            return out, [], rounds
        out, vetoed = greedy(D, taken, thr, ratio, self.rules, veto)
        return out, vetoed, 0

    def step(self, desc, depth, veto=None, nocreate=None):
        """One frame.  Returns a dict: match_gid / new_gid / rows (pool row matched to each keypoint) per keypoint, the four
        counters, `active` (the two active-row counts), `D1` / `D2` (the passes' distance matrices) and `rows1` / `rows2`."""
        R, id, n = self.rules, self.frame, len(desc)
        desc = np.asarray(desc, np.uint8).reshape(n, 32)
        nocreate = np.zeros(n, bool) if nocreate is None else np.asarray(nocreate, bool)
        mp = [None] * n
        res = dict(n_match_pass1=0, n_match_pass2=0, n_new_mappoints=0, active=[0, 0], rounds=[0, 0], vetoed=[],
                   D1=None, D2=None)
        new_gid = np.full(n, -1, np.int32)
        pass_of = np.zeros(n, np.int32)
        if id == 0:
            for i in range(n):                        # src/Tracking.cc:44,61-66: the flag is never reset
                self.dynamic0 = self.dynamic0 or bool(nocreate[i])
                if depth[i] > 0 and not self.dynamic0:
                    mp[i] = self._create(desc[i], id)
                    new_gid[i] = mp[i].gid
                    res["n_new_mappoints"] += 1
            match = [None] * n
        else:
            row_of = {id_of(p): r for r, p in enumerate(self.pool)}
            taken = np.zeros(n, bool)
            # pass 1
            rows1 = [(i, p) for i, p in enumerate(self.last_mp) if p is not None and not p.bad]
            D1 = distances(np.array([p.desc for _, p in rows1], np.uint8), desc)
            res["D1"], res["rows1"] = D1, [row_of[id_of(p)] for _, p in rows1]
            res["active"][0] = int((D1.min(1) < 15).sum()) if n else 0
            v1 = None if veto is None else np.asarray(veto, bool)[[i for i, _ in rows1]]
            out, vetoed, res["rounds"][0] = self._pass(D1, taken, R["thr1"], False, v1)
            for r in vetoed:
                rows1[r][1].bad = True
                res["vetoed"].append(rows1[r][0])
            for r, j in out.items():
                mp[j] = rows1[r][1]
                mp[j].seen = id
                pass_of[j] = 1
                res["n_match_pass1"] += 1
            # pass 2
            rows2 = [p for p in self.pool if p.local and not p.bad and (R["keep_observed"] or p.seen != id)]
            D2 = distances(np.array([p.desc for p in rows2], np.uint8), desc)
            res["D2"], res["rows2"] = D2, [row_of[id_of(p)] for p in rows2]
            res["active"][1] = int((D2.min(1) < 30).sum()) if n else 0
            out, _, res["rounds"][1] = self._pass(D2, taken, R["thr2"], True)
            for r, j in out.items():
                mp[j] = rows2[r]
                mp[j].seen = id
                pass_of[j] = 2
                res["n_match_pass2"] += 1
            match = list(mp)
            res["rows"] = np.array([row_of[id_of(p)] if p is not None else -1 for p in mp], np.int32)
        if id == 0:
            row_of = {id_of(p): r for r, p in enumerate(self.pool)}
            res["rows"] = np.array([row_of[id_of(p)] if p is not None else -1 for p in mp], np.int32)
        res["match_gid"] = np.array([p.gid if p is not None else -1 for p in match], np.int32)
        if id > 0:
            for i in range(n):                        # frame::createmappoint
                if mp[i] is None and depth[i] > 0 and not nocreate[i]:
                    mp[i] = self._create(desc[i], id)
                    new_gid[i] = mp[i].gid
                    res["n_new_mappoints"] += 1
        res["new_gid"], res["pass_of"], res["n_pool_before"] = new_gid, pass_of, len(self.pool)
        self.last_mp = mp
        if id >= 4:
            for p in self.pool:
                if p.create_id <= id - R["cull_age"]:
                    p.local = False
        ref = set() if R["drop_referenced"] else {id_of(p) for p in mp if p is not None}
        self.pool = [p for p in self.pool if p.local or id_of(p) in ref]
        if R["drop_referenced"]:
            alive = {id_of(p) for p in self.pool}
            self.last_mp = [p if p is not None and id_of(p) in alive else None for p in mp]
        res["n_local_map"] = sum(p.local for p in self.pool)
        res["n_pool"] = len(self.pool)
        self.frame += 1
        return res


def id_of(p):
    return id(p)


def as_reported(r, frame):
    """(match_gid, new_gid) as the oracle's and the device's debug records hold them: the points Tracking::init creates are
    frame 0's own MapPoints (its LM edges), so they are reported as matched there and nothing as created."""
    if frame == 0:
        return r["new_gid"], np.full(len(r["new_gid"]), -1, np.int32)
    return r["match_gid"], r["new_gid"]
