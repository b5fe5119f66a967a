"""Plain-Python restatement of the core and spectrum rules and the (path, core) table for RMCSA actions (include/orl.h,
orl_batch_route_cores), written from the definitions there, slot by slot and hop by hop.  Test infrastructure only; shares no code
with the kernel.  It stands on rmcsa_mask_restate.prov_all — prov(p, m, c, s) of every action, from the reference's definitions — and
complete_restate's m*(p), slots and reach.

For an env's pending service and a pair (p, c): m(p) = m*(p), or the fixed modulation where the path is within its reach; n(p) the
slots under m(p); fits(p, c) = {s : prov(p, m(p), c, s)}; row(p, c) the AND of the hops' free rows in core c; free(p, c) its
popcount.  The winner (s*, c*) of a pair: first (min fits, s*), last (max fits, S - n - s*), best (start of the shortest maximal free
run of row(p, c) with L >= n, ties to the lowest start; L - n), exact (the lowest-start run with L == n: cost 0; else first fit:
1 + s*), min_cuts (fewest cuts, ties lowest s; the cuts).  cuts = hops l of p with s >= 1, s + n <= S - 1, slot s - 1 free on l in core
c and slot s + n free on l in core c.  Table row p C + c: (s*, c*, n, free); no fit: (S, NO_FIT, n, free); a path the service cannot
use: (S, NO_FIT, 0, 0).  The prefix — nothing, (path), (path, core) — admits the candidate pairs; routes over the candidates that fit:
ksp the lowest (p, c), best the smallest c*, least_loaded the largest free(p, c) (ties: the lowest (p, c)), ksp_best_core /
ksp_least_loaded_core the first path with a fit and among its cores the smallest c* / the largest free (ties: the lowest core).
Action: (p, m(p), c, s*), or the reject action (K, M, C, S)."""
import numpy as np

from tests import complete_restate as cr
from tests import rmcsa_mask_restate as rr
from tests.assign_restate import runs_of

RULES = ("first", "last", "best", "exact", "min_cuts")
ROUTES = ("ksp", "best", "least_loaded", "ksp_best_core", "ksp_least_loaded_core")
RULE_IDS = {"first": 0, "last": 1, "best": 2, "exact": 3, "min_cuts": 6}
NO_FIT = 0x7FFFFFFF
KINDS = ("reject", "ksp_upper_core", "later_path", "best_ne_ksp", "least_loaded_ne_ksp", "ksp_best_core_ne_ksp", "ksp_least_loaded_core_ne_ksp",
         "cost_tie", "at_top", "exact_hit", "exact_miss", "min_cuts_ne_first", "cuts_zero", "cuts_ge_2", "other_modulation", "out_of_reach",
         "window_across_word")


class Prepared:
    """Per env of a state, under `modulation` (None: m*(p)): mod[i][p] (-1: the path cannot be used), need[i][p], hop rows
    hops[i][p][c] (one list of bools per hop), their AND row[i][p][c], and fits[i][p][c] from prov_all"""

    def __init__(self, avail, services, topo, tables, modulation=None, pv=None):
        self.n, self.C, self.E, self.S = avail.shape
        self.K, self.M = topo.k_paths, len(tables["lmax_xt"])
        pv = rr.prov_all(avail, services, topo, tables) if pv is None else pv
        mstar, reach, need = cr.best_in_reach(services, topo, tables), cr.reach_of(services, topo, tables), cr.slots_of(services, tables)
        self.mod, self.need, self.hops, self.row, self.fits = [], [], [], [], []
        self.best_mod = []
        for i in range(self.n):
            src, dst = int(services[i, 2]), int(services[i, 3])
            mods, needs, hops_i, rows_i, fits_i = [], [], [], [], []
            for p in range(self.K):
                if modulation is None:
                    m = int(mstar[i, p])
                else:
                    m = int(modulation) if reach[i, p, int(modulation)] else -1
                if p >= int(topo.n_paths[src, dst]):
                    m = -1
                mods.append(m)
                needs.append(int(need[i, m]) if m >= 0 else 0)
                per_core_h, per_core_r, per_core_f = [], [], []
                for c in range(self.C):
                    if m < 0:
                        per_core_h.append([]), per_core_r.append([False] * self.S), per_core_f.append([])
                        continue
                    links = topo.path_links[src, dst, p, :int(topo.path_hops[src, dst, p])]
                    hop_rows = [[bool(v) for v in avail[i, c, int(l), :]] for l in links]
                    per_core_h.append(hop_rows)
                    per_core_r.append([all(h[s] for h in hop_rows) for s in range(self.S)])
                    per_core_f.append([int(s) for s in np.flatnonzero(pv[i, p, m, c])])
                hops_i.append(per_core_h), rows_i.append(per_core_r), fits_i.append(per_core_f)
            self.mod.append(mods), self.need.append(needs), self.hops.append(hops_i), self.row.append(rows_i), self.fits.append(fits_i)
            self.best_mod.append([int(tables["path_best_mod"][src, dst, p]) for p in range(self.K)])

    @property
    def reject(self):
        return (self.K, self.M, self.C, self.S)


def cuts(prep, i, p, c, s):
    n, S, count = prep.need[i][p], prep.S, 0
    for row in prep.hops[i][p][c]:  # hop by hop
        if s >= 1 and s + n <= S - 1 and row[s - 1] and row[s + n]:
            count += 1
    return count


def winner(prep, i, p, c, rule):
    """(s*, c*) of pair (p, c) of env i under `rule`, None where fits(p, c) is empty"""
    n, S, fits = prep.need[i][p], prep.S, prep.fits[i][p][c]
    if not fits:
        return None
    if rule == "first":
        return fits[0], fits[0]
    if rule == "last":
        return fits[-1], S - n - fits[-1]
    if rule in ("best", "exact"):
        runs = [(st, L) for st, L in runs_of(prep.row[i][p][c]) if L >= n]
        if rule == "best":
            shortest = min(L for _, L in runs)
            return min(st for st, L in runs if L == shortest), shortest - n
        exact = [st for st, L in runs if L == n]
        return (min(exact), 0) if exact else (fits[0], 1 + fits[0])
    assert rule == "min_cuts"
    counts = [cuts(prep, i, p, c, s) for s in fits]
    return fits[counts.index(min(counts))], min(counts)


def table(prep, rule):
    """int32 [n, K C, 4]: row p C + c = (s*, c*, n(p), free(p, c))"""
    out = np.zeros((prep.n, prep.K * prep.C, 4), np.int32)
    out[:, :, 0], out[:, :, 1] = prep.S, NO_FIT
    for i in range(prep.n):
        for p in range(prep.K):
            if prep.mod[i][p] < 0:
                continue
            for c in range(prep.C):
                q = p * prep.C + c
                out[i, q, 2], out[i, q, 3] = prep.need[i][p], sum(prep.row[i][p][c])
                w = winner(prep, i, p, c, rule)
                if w is not None:
                    out[i, q, :2] = w
    return out


def admits(prefix, p, c):
    """Does the prefix — (), (path,) or (path, core) of one env — admit the pair?"""
    return (len(prefix) < 1 or p == prefix[0]) and (len(prefix) < 2 or c == prefix[1])


def route(prep, tab, route_name, given=None):
    """int32 [n, 4] actions from a table, by plain loops over the pairs; given: int [n, g], g = 1 (path) or 2 (path, core), or None"""
    K, C = prep.K, prep.C
    out = np.zeros((prep.n, 4), np.int32)
    for i in range(prep.n):
        prefix = () if given is None else tuple(int(v) for v in given[i])
        cands = [(p, c) for p in range(K) for c in range(C) if tab[i, p * C + c, 1] != NO_FIT and admits(prefix, p, c)]
        if route_name in ("ksp_best_core", "ksp_least_loaded_core"):
            cands = [pc for pc in cands if pc[0] == cands[0][0]]
        got, key = None, None
        for p, c in cands:
            s, cost, _, free = (int(v) for v in tab[i, p * C + c])
            this = 0 if route_name == "ksp" else cost if route_name in ("best", "ksp_best_core") else -free
            if key is None or this < key:  # (strictly: ties stay with the lowest pair)
                got, key = (p, prep.mod[i][p], c, s), this
        out[i] = prep.reject if got is None else got
    return out


def brute_action(prep, i, rule, route_name, prefix=()):
    """The action of env i by ONE loop over all (p, c, s) with a key tuple, the reject action where nothing fits"""
    S, best = prep.S, None
    for p in range(prep.K):
        if prep.mod[i][p] < 0:
            continue
        n = prep.need[i][p]
        for c in range(prep.C):
            if not admits(prefix, p, c):
                continue
            m = prep.row[i][p][c]
            for s in range(S):
                if s + n > S or not all(m[s:s + n]):
                    continue
                rk, cost = brute_key(prep, i, p, c, s, rule)
                primary = {"ksp": (0, p), "best": (cost, p), "least_loaded": (-sum(m), p), "ksp_best_core": (p, cost),
                           "ksp_least_loaded_core": (p, -sum(m))}[route_name]
                key = primary + (c,) + rk
                if best is None or key < best[0]:
                    best = (key, (p, prep.mod[i][p], c, s))
    return prep.reject if best is None else best[1]


def brute_key(prep, i, p, c, s, rule):
    """(the rule's key of start s, its cost): the smallest key over fits(p, c) is the pair's winner"""
    n, S, m = prep.need[i][p], prep.S, prep.row[i][p][c]
    lo, hi = s, s
    while lo > 0 and m[lo - 1]:
        lo -= 1
    while hi + 1 < S and m[hi + 1]:
        hi += 1
    L = hi - lo + 1
    if rule == "min_cuts":
        k = sum(1 for row in prep.hops[i][p][c] if s >= 1 and s + n <= S - 1 and row[s - 1] and row[s + n])
        return (k, s), k
    return {"first": ((s,), s), "last": ((-s,), S - n - s), "best": ((L, s), L - n),
            "exact": ((0, s), 0) if L == n and s == lo else ((1, s), 1 + s)}[rule]


def brute_winner(prep, i, p, c, rule):
    best = None
    n, S, m = prep.need[i][p], prep.S, prep.row[i][p][c]
    for s in range(S):
        if prep.mod[i][p] < 0 or s + n > S or not all(m[s:s + n]):
            continue
        key, cost = brute_key(prep, i, p, c, s, rule)
        if best is None or key < best[0]:
            best = (key, s, cost)
    return None if best is None else (best[1], best[2])


def count_kinds(prep, seen):
    """Adds to `seen` what the state holds (KINDS), from the restatement's own tables (modulation=None)"""
    def count(kind, yes):
        seen[kind] = seen.get(kind, 0) + int(bool(yes))

    C, S = prep.C, prep.S
    tabs = {rule: table(prep, rule) for rule in RULES}
    for rule in RULES:
        tab = tabs[rule]
        acts = {r: route(prep, tab, r) for r in ROUTES}
        for i in range(prep.n):
            ksp = tuple(acts["ksp"][i])
            if rule == "first":
                count("reject", ksp == prep.reject)
                count("ksp_upper_core", ksp != prep.reject and ksp[2] > 0)
                count("later_path", ksp != prep.reject and ksp[0] > 0)
                count("other_modulation", ksp != prep.reject and ksp[1] != prep.best_mod[i][ksp[0]])
            for r in ROUTES[1:]:
                count(r + "_ne_ksp", tuple(acts[r][i]) != ksp)
            costs = [int(v) for v in tab[i, :, 1] if v != NO_FIT]
            count("cost_tie", len(costs) > len(set(costs)))
    first, exact, mc = tabs["first"], tabs["exact"], tabs["min_cuts"]
    for i in range(prep.n):
        count("out_of_reach", any(m < 0 for m in prep.mod[i]))
        for q in range(prep.K * C):
            if first[i, q, 1] == NO_FIT:
                continue
            n = int(first[i, q, 2])
            count("exact_hit", exact[i, q, 1] == 0)
            count("exact_miss", exact[i, q, 1] > 0)
            count("min_cuts_ne_first", mc[i, q, 0] != first[i, q, 0])
            count("cuts_zero", mc[i, q, 1] == 0)
            count("cuts_ge_2", mc[i, q, 1] >= 2)
            for tab in tabs.values():
                s = int(tab[i, q, 0])
                count("at_top", s + n == S)
                count("window_across_word", s // 64 != (s + n - 1) // 64)
    return seen
