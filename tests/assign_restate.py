"""Numpy restatement of the spectrum-assignment rules for RMSA and RWA actions (include/orl.h, orl_batch_assign_spectrum), written
from the definitions there — slot by slot, on run-length encodings of a Python list — from a slot map (bool [n, links, S]), the
pending services and the topology.  Test infrastructure only; shares no code with the kernel.

For the pending service of an env and a path p < n_paths[src, dst]: n(p) the slots it needs (RMSA: get_number_slots under the path's
best modulation, RWA: 1), m(p) the AND of the free-slot rows over the hops of p, fits(p) = {s : s + n <= S, m(p)[s .. s + n - 1] free}.
Rules: first = min fits; last = max fits; best = the start of the shortest maximal free run of m(p) with L >= n (ties: the lowest
start); exact = the lowest-start maximal run with L == n, else first; most_used / least_used = the s of fits(p) with the largest /
smallest U(s) = sum of u[s .. s + n - 1] (ties: the lowest s), u[w] = links of the whole map with slot w occupied.  n_given = 1: the
path is given (out of range: no completion); n_given = 0: the first path with a non-empty fits(p).  No completion: (k, S)."""
import math

import numpy as np

from tests.mask_restate import row_words, unpack_slots  # noqa: F401  (re-exported: the tests read the packed maps with them)

RULES = ("first", "last", "best", "exact", "most_used", "least_used")
KINDS = ("no_completion", "last_start", "run_across_word", "best_tie", "used_tie", "path_high", "path_negative", "later_path",
         "differs_last", "differs_best", "differs_exact", "differs_most_used", "differs_least_used")
RMSA_KINDS = KINDS + ("window_across_word",)  # (an RWA window is one slot)


def runs_of(row):
    """[(start, length)] of the maximal runs of True in a sequence of bools, slot by slot"""
    out, start = [], None
    for s, free in enumerate(row):
        if free and start is None:
            start = s
        if not free and start is not None:
            out.append((start, s - start))
            start = None
    if start is not None:
        out.append((start, len(row) - start))
    return out


class Prepared:
    """Per env of a state: need[i][p], m[i][p] (list of bools) for p < n_paths, and u[i] (occupied links per slot)"""

    def __init__(self, env_type, avail, services, topo, k, S, channel_width=12.5):
        self.k, self.S, self.n = k, S, len(services)
        self.need, self.m, self.u = [], [], []
        self._runs, self._fits = {}, {}
        for i in range(self.n):
            src, dst, br = int(services[i, 2]), int(services[i, 3]), float(services[i, 4])
            need, rows = [], []
            for p in range(int(topo.n_paths[src, dst])):
                hops = int(topo.path_hops[src, dst, p])
                links = [int(l) for l in topo.path_links[src, dst, p, :hops]]
                rows.append([bool(v) for v in avail[i, links, :].all(axis=0)])  # free on every hop
                if env_type == 2:
                    need.append(1)
                else:
                    se = topo.modulations[int(topo.path_best_mod[src, dst, p])].spectral_efficiency
                    need.append(math.ceil(br / (se * channel_width)) + 1)
            self.need.append(need)
            self.m.append(rows)
            self.u.append([int(v) for v in (~avail[i]).sum(axis=0)])

    def runs(self, i, p):
        if (i, p) not in self._runs:
            self._runs[i, p] = runs_of(self.m[i][p])
        return self._runs[i, p]

    def fits(self, i, p):
        if (i, p) not in self._fits:
            n, S = self.need[i][p], self.S
            self._fits[i, p] = [s for st, L in self.runs(i, p) if L >= n for s in range(st, st + L - n + 1) if s + n <= S]
        return self._fits[i, p]

    def window(self, i, p, s):
        return sum(self.u[i][s:s + self.need[i][p]])

    def choose(self, i, p, rule):
        """s* of path p under `rule` (None: fits(p) is empty), and what the choice held: {kind: bool}"""
        n = self.need[i][p]
        fits = self.fits(i, p)
        if not fits:
            return None, {}
        runs = [(st, L) for st, L in self.runs(i, p) if L >= n]
        what = {}
        if rule == "first":
            s = fits[0]
        elif rule == "last":
            s = fits[-1]
        elif rule == "best":
            shortest = min(L for _, L in runs)
            starts = [st for st, L in runs if L == shortest]
            s = starts[0]
            what["best_tie"] = len(starts) > 1
        elif rule == "exact":
            starts = [st for st, L in runs if L == n]
            s = starts[0] if starts else fits[0]
        else:
            sums = [self.window(i, p, t) for t in fits]
            extreme = max(sums) if rule == "most_used" else min(sums)
            where = [t for t, v in zip(fits, sums) if v == extreme]
            s = where[0]
            what["used_tie"] = len(where) > 1
        st, L = [(a, b) for a, b in runs if a <= s < a + b][0]
        what["last_start"] = s + n == self.S
        what["run_across_word"] = st // 64 != (st + L - 1) // 64
        what["window_across_word"] = s // 64 != (s + n - 1) // 64
        if rule != "first":
            what["differs_" + rule] = s != fits[0]
        return s, what


def assign(prep, rule, n_given, given=None, seen=None):
    """int32 [n, 4]: every env's (path, s*, 0, 0) under `rule`, (k, S, 0, 0) where there is no completion; `seen`: a dict of counts
    per kind (KINDS) to add to."""
    assert rule in RULES and n_given in (0, 1) and (given is not None) == (n_given == 1)
    out = np.zeros((prep.n, 4), np.int32)
    seen = {} if seen is None else seen

    def count(kind, yes=True):
        seen[kind] = seen.get(kind, 0) + int(bool(yes))

    for i in range(prep.n):
        np_i = len(prep.m[i])
        got, what = None, {}
        if n_given == 1:
            p = int(given[i])
            count("path_high", p >= np_i)
            count("path_negative", p < 0)
            if 0 <= p < np_i:
                s, what = prep.choose(i, p, rule)
                got = None if s is None else (p, s)
        else:
            for p in range(np_i):
                s, what = prep.choose(i, p, rule)
                if s is not None:
                    got = (p, s)
                    count("later_path", p > 0)
                    break
        count("no_completion", got is None)
        for kind, yes in what.items():
            count(kind, yes)
        out[i, :2] = (prep.k, prep.S) if got is None else got
    return out


def brute(prep, i, p, rule):
    """The rule's choice on path p of env i by one loop over all s, without run-length encoding (None: nothing fits)"""
    n, S, m = prep.need[i][p], prep.S, prep.m[i][p]
    best_s, best_key = None, None
    for s in range(S):
        if s + n > S or not all(m[s:s + n]):
            continue
        lo = s
        while lo > 0 and m[lo - 1]:
            lo -= 1
        hi = s
        while hi + 1 < S and m[hi + 1]:
            hi += 1
        L = hi - lo + 1
        if rule == "first":
            key = s
        elif rule == "last":
            key = -s
        elif rule == "best":
            key = (L, s)  # (the lowest s of a run is its start)
        elif rule == "exact":
            key = (0 if L == n else 1, s)
        elif rule == "most_used":
            key = (-sum(prep.u[i][s:s + n]), s)
        else:
            key = (sum(prep.u[i][s:s + n]), s)
        if best_key is None or key < best_key:
            best_s, best_key = s, key
    return best_s


def path_fits(prep):
    """bool [n, k]: fits(p) is non-empty"""
    out = np.zeros((prep.n, prep.k), bool)
    for i in range(prep.n):
        for p in range(len(prep.m[i])):
            out[i, p] = bool(prep.fits(i, p))
    return out
