"""Numpy / plain-Python restatement of the routing rules and the per-path assignment table for RMSA and RWA actions (include/orl.h,
orl_batch_route_spectrum), written from the definitions there, slot by slot and hop by hop.  Test infrastructure only; shares no code
with the kernel.  The per-path state (need, m(p), u[]) is tests/assign_restate.py's Prepared.

For an env's pending service and a path p < n_paths: fits(p) = {s : s + n <= S, m(p)[s .. s + n - 1] free}; the winner of a path is
(s*, c*): first (min fits, s*), last (max fits, S - n - s*), best (start of the shortest maximal free run with L >= n, ties to the
lowest start; L - n), exact (the lowest-start run with L == n: cost 0; else first fit: 1 + s*), most_used (largest U(s), ties lowest s;
n E - U), least_used (smallest U(s); U), min_cuts (fewest cuts(p, s), ties lowest s; the cuts).  cuts(p, s) = hops l of p with s >= 1,
s + n <= S - 1, slot s - 1 free on l and slot s + n free on l.  Routes over the paths that fit: ksp the lowest p, best the smallest c*
(ties lowest p), least_loaded the largest free(p) = popcount m(p) (ties lowest p).  Table row p: (s*, c*, n, free); no fit: (S, NO_FIT, n,
free); p >= n_paths: (S, NO_FIT, 0, 0).  Action: (p, s*, 0, 0), or (k, S, 0, 0).

last_start=False drops s = S - n from fits(p): the reference's range(0, S - n) — only so that the restatement can be pinned to the
reference's heuristics on every env."""
import numpy as np

from tests.assign_restate import Prepared, brute, runs_of  # noqa: F401  (re-exported)

RULES = ("first", "last", "best", "exact", "most_used", "least_used", "min_cuts")
ROUTES = ("ksp", "best", "least_loaded")
NO_FIT = 0x7FFFFFFF
KINDS = ("no_completion", "best_ne_ksp", "least_loaded_ne_ksp", "cost_tie", "min_cuts_ne_first", "cuts_tie", "cuts_zero", "cuts_ge_2",
         "min_cuts_at_0", "min_cuts_at_top")
RMSA_KINDS = KINDS + ("window_across_word",)  # (an RWA window is one slot)


class Links:
    """Per env of a state: the hops' own free rows of every path (lists of bools), for cuts(p, s)"""

    def __init__(self, avail, services, topo):
        self.rows = []
        self.E = avail.shape[1]
        for i in range(len(services)):
            src, dst = int(services[i, 2]), int(services[i, 3])
            per_path = []
            for p in range(int(topo.n_paths[src, dst])):
                hops = int(topo.path_hops[src, dst, p])
                per_path.append([[bool(v) for v in avail[i, int(l), :]] for l in topo.path_links[src, dst, p, :hops]])
            self.rows.append(per_path)


def cuts(links, S, i, p, s, n):
    c = 0
    for row in links.rows[i][p]:  # hop by hop
        if s >= 1 and s + n <= S - 1 and row[s - 1] and row[s + n]:
            c += 1
    return c


def fits_of(prep, i, p, last_start=True):
    cache = prep.__dict__.setdefault("_route_fits", {})  # (every rule asks again)
    if (i, p, last_start) not in cache:
        n, S, m = prep.need[i][p], prep.S, prep.m[i][p]
        out = []
        for s in range(S):
            if s + n <= S and all(m[s:s + n]) and (last_start or s + n < S):
                out.append(s)
        cache[i, p, last_start] = out
    return cache[i, p, last_start]


def winner(prep, links, i, p, rule, last_start=True):
    """(s*, c*) of path p of env i under `rule`, None where fits(p) is empty"""
    n, S, m = prep.need[i][p], prep.S, prep.m[i][p]
    fits = fits_of(prep, i, p, last_start)
    if not fits:
        return None
    if rule == "first":
        return fits[0], fits[0]
    if rule == "last":
        return fits[-1], S - n - fits[-1]
    if rule in ("best", "exact"):
        runs = [(st, L) for st, L in runs_of(m) if any(st <= s < st + L for s in fits)]  # the maximal free runs that hold a fit
        if rule == "best":
            shortest = min(L for _, L in runs)
            st = min(a for a, L in runs if L == shortest)
            return min(s for s in fits if s >= st), shortest - n
        exact = [st for st, L in runs if L == n]
        if exact:
            return min(exact), 0
        return fits[0], 1 + fits[0]
    if rule in ("most_used", "least_used"):
        sums = [sum(prep.u[i][s:s + n]) for s in fits]
        extreme = max(sums) if rule == "most_used" else min(sums)
        s = fits[sums.index(extreme)]
        return s, (n * links.E - extreme) if rule == "most_used" else extreme
    assert rule == "min_cuts"
    counts = [cuts(links, S, i, p, s, n) for s in fits]
    least = min(counts)
    return fits[counts.index(least)], least


def table(prep, links, rule, last_start=True):
    """int32 [n, k, 4]: row p = (s*, c*, n(p), free(p))"""
    out = np.zeros((prep.n, prep.k, 4), np.int32)
    out[:, :, 0], out[:, :, 1] = prep.S, NO_FIT
    for i in range(prep.n):
        for p in range(len(prep.m[i])):
            out[i, p, 2], out[i, p, 3] = prep.need[i][p], sum(prep.m[i][p])
            w = winner(prep, links, i, p, rule, last_start)
            if w is not None:
                out[i, p, :2] = w
    return out


def route(tab, route_name, k, S):
    """int32 [n, 4] actions from a table, by a plain loop over the paths"""
    out = np.zeros((len(tab), 4), np.int32)
    for i in range(len(tab)):
        got, key = None, None
        for p in range(k):
            s, c, _, free = (int(v) for v in tab[i, p])
            if c == NO_FIT:
                continue
            this = 0 if route_name == "ksp" else c if route_name == "best" else -free
            if key is None or this < key:  # (strictly: ties stay with the lowest p)
                got, key = (p, s), this
        out[i, :2] = (k, S) if got is None else got
    return out


def count_kinds(prep, links, seen):
    """Adds to `seen` what the state holds (KINDS), from the restatement's own tables"""
    def count(kind, yes):
        seen[kind] = seen.get(kind, 0) + int(bool(yes))

    k, S = prep.k, prep.S
    first, mc = table(prep, links, "first"), table(prep, links, "min_cuts")
    ksp = route(first, "ksp", k, S)
    for i in range(prep.n):
        count("no_completion", ksp[i, 0] == k)
    for rule in ("first", "best", "min_cuts"):
        tab = first if rule == "first" else mc if rule == "min_cuts" else table(prep, links, rule)
        a_ksp, a_best, a_ll = (route(tab, r, k, S) for r in ROUTES)
        for i in range(prep.n):
            count("best_ne_ksp", a_best[i, 0] != a_ksp[i, 0])
            count("least_loaded_ne_ksp", a_ll[i, 0] != a_ksp[i, 0])
            costs = [int(c) for c in tab[i, :, 1] if c != NO_FIT]
            count("cost_tie", len(costs) > len(set(costs)))
    for i in range(prep.n):
        for p in range(len(prep.m[i])):
            s, c, n = int(mc[i, p, 0]), int(mc[i, p, 1]), int(mc[i, p, 2])
            if c == NO_FIT:
                continue
            count("min_cuts_ne_first", s != first[i, p, 0])
            count("cuts_tie", sum(1 for t in fits_of(prep, i, p) if cuts(links, S, i, p, t, n) == c) > 1)
            count("cuts_zero", c == 0)
            count("cuts_ge_2", c >= 2)
            count("min_cuts_at_0", s == 0)
            count("min_cuts_at_top", s + n == S)
            count("window_across_word", s // 64 != (s + n - 1) // 64)
    return seen


def brute_winner(prep, links, i, p, rule):
    """The rule's (s*, c*) on path p by one loop over all s with a key tuple, None where nothing fits"""
    n, S, m = prep.need[i][p], prep.S, prep.m[i][p]
    best = None
    for s in range(S):
        if s + n > S or not all(m[s:s + n]):
            continue
        lo, hi = s, s
        while lo > 0 and m[lo - 1]:
            lo -= 1
        while hi + 1 < S and m[hi + 1]:
            hi += 1
        L = hi - lo + 1
        U = sum(prep.u[i][s:s + n])
        key, cost = {"first": ((s,), s), "last": ((-s,), S - n - s), "best": ((L, s), L - n),
                     "exact": ((0, s), 0) if L == n and s == lo else ((1, s), 1 + s),
                     "most_used": ((-U, s), n * links.E - U), "least_used": ((U, s), U)}.get(rule, (None, None))
        if rule == "min_cuts":
            c = sum(1 for row in links.rows[i][p] if s >= 1 and s + n <= S - 1 and row[s - 1] and row[s + n])
            key, cost = (c, s), c
        if best is None or key < best[0]:
            best = (key, s, cost)
    return None if best is None else (best[1], best[2])
