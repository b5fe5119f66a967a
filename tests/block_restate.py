"""Plain run-length restatement of the block actions (include/orl.h, orl_batch_block_table / orl_batch_select_blocks), written from the
definitions there from unpacked slot maps.  Test infrastructure only; shares no code with the kernels.

For an env's pending service and every row r of the path features' row order (r = p; RMCSA: r = p C + c): n(r) the slots the service
needs (RMSA / DeepRMSA: get_number_slots under the path's best modulation; RWA: 1; RMCSA: under m*(p), the modulation within reach
with the fewest slots, or under the fixed modulation where the path is within its reach), row(r) the AND of the hops' free rows, its
blocks the maximal free runs of >= n slots in slot order.  Table row r: (n, free, start_0, L_0, ...), (S, 0) for a block that does not
exist, (0, 0, S, 0, ...) for a row the service cannot use.  Mask column r j + b: block b of row r exists; the last column the reject
action; the fallback of the other masks.  Selection of index a: r = a // j, b = a % j; "first" s = start_b, "last" s = start_b + L_b
- n; action (p, s, 0, 0), RMCSA (p, m(p), c, s); the family's reject row for a < 0, a >= R j or a block that does not exist.

avail: bool [n, C, links, S] (C = 1 outside RMCSA); env_type: 0 RMSA, 1 DeepRMSA, 2 RWA, 3 RMCSA."""
import itertools

import numpy as np

from tests import complete_restate as cr
from tests.path_features_restate import slots_needed

KINDS = ("runs_0", "runs_below_j", "runs_j", "runs_above_j", "ends_at_top", "starts_at_0", "exactly_n", "across_word", "short_between")
RWA_KINDS = tuple(k for k in KINDS if k != "short_between")  # (an RWA service needs one wavelength: no free run is shorter)
RMCSA_KINDS = KINDS + ("no_modulation", "fixed_beyond_reach")


class Rows:
    """Per env of a state the R rows: need[i][r] (0: the service cannot use the row), mod[i][r] (RMCSA: m(p), else 0), row[i][r] (a list of
    bools, None for an unusable row)"""

    def __init__(self, env_type, avail, services, topo, tables=None, modulation=None):
        self.env_type = env_type
        self.n, self.C, _, self.S = avail.shape
        self.K = topo.k_paths
        self.R = self.K * self.C
        self.M = len(tables["lmax_xt"]) if env_type == 3 else 0
        assert env_type == 3 or (self.C == 1 and modulation is None)
        if env_type == 3:
            mstar, reach, slots = cr.best_in_reach(services, topo, tables), cr.reach_of(services, topo, tables), cr.slots_of(services, tables)
        self.need, self.mod, self.row = [], [], []
        self.fixed_beyond_reach = 0
        for i in range(self.n):
            src, dst, br = int(services[i, 2]), int(services[i, 3]), float(services[i, 4])
            need, mod, row = [], [], []
            for p in range(self.K):
                n, m = 0, 0
                if p < int(topo.n_paths[src, dst]):
                    if env_type != 3:
                        n = slots_needed(env_type, topo, None, src, dst, p, br)
                    else:
                        m = int(mstar[i, p]) if modulation is None else (int(modulation) if reach[i, p, int(modulation)] else -1)
                        n = int(slots[i, m]) if m >= 0 else 0
                        self.fixed_beyond_reach += int(modulation is not None and m < 0)
                for c in range(self.C):
                    need.append(n), mod.append(m)
                    if n == 0:
                        row.append(None)
                        continue
                    links = topo.path_links[src, dst, p, :int(topo.path_hops[src, dst, p])]
                    row.append([bool(v) for v in avail[i, c][links, :].all(axis=0)])
            self.need.append(need), self.mod.append(mod), self.row.append(row)

    @property
    def reject(self):
        return (self.K, self.M, self.C, self.S) if self.env_type == 3 else (self.K, self.S, 0, 0)


def runs_of(row):
    """[(start, length)] of the maximal free runs of a row, in slot order, by run-length"""
    out, s = [], 0
    for free, grp in itertools.groupby(row):
        L = len(list(grp))
        if free:
            out.append((s, L))
        s += L
    return out


def blocks_of(rows, i, r):
    """The fitting blocks of row r of env i, all of them"""
    if rows.need[i][r] == 0:
        return []
    cache = rows.__dict__.setdefault("_blocks", {})  # (table, mask and every selection ask again)
    if (i, r) not in cache:
        cache[i, r] = [(st, L) for st, L in runs_of(rows.row[i][r]) if L >= rows.need[i][r]]
    return cache[i, r]


def brute_blocks(row, n, S):
    """The same by a loop per slot: a block starts at a free slot whose lower neighbour is taken (or at 0), and counts if the n slots
    from it are free; its length by walking up to the first taken slot or S"""
    out = []
    for s in range(S):
        if not row[s] or (s > 0 and row[s - 1]):
            continue
        if s + n > S or not all(row[s:s + n]):
            continue
        e = s
        while e < S and row[e]:
            e += 1
        out.append((s, e - s))
    return out


def table(rows, j):
    """int32 [n, R, 2 + 2 j]"""
    out = np.zeros((rows.n, rows.R, 2 + 2 * j), np.int32)
    out[:, :, 2::2] = rows.S
    for i in range(rows.n):
        for r in range(rows.R):
            if rows.need[i][r] == 0:
                continue
            out[i, r, 0], out[i, r, 1] = rows.need[i][r], sum(rows.row[i][r])
            for b, (st, L) in enumerate(blocks_of(rows, i, r)[:j]):
                out[i, r, 2 + 2 * b], out[i, r, 3 + 2 * b] = st, L
    return out


def mask(rows, j, allow_rejection, fallback=True):
    """bool [n, R j + 1]"""
    out = np.zeros((rows.n, rows.R * j + 1), bool)
    for i in range(rows.n):
        for r in range(rows.R):
            out[i, r * j:r * j + min(j, len(blocks_of(rows, i, r)))] = True
        if fallback and not allow_rejection and not out[i, :-1].any():
            out[i, :-1] = True
        out[i, -1] = bool(allow_rejection)
    return out


def select(rows, j, indices, placement="first"):
    """int32 [n, 4] actions of the indices"""
    out = np.zeros((rows.n, 4), np.int32)
    for i in range(rows.n):
        a = int(indices[i])
        out[i] = rows.reject
        if not 0 <= a < rows.R * j:
            continue
        r, b = a // j, a % j
        blocks = blocks_of(rows, i, r)
        if b >= len(blocks):
            continue
        st, L = blocks[b]
        s = st if placement == "first" else st + L - rows.need[i][r]
        p, c = r // rows.C, r % rows.C
        out[i] = (p, rows.mod[i][r], c, s) if rows.env_type == 3 else (p, s, 0, 0)
    return out


def draw_indices(rows, j, rng):
    """An index per env, by env index mod 8: 0 - 3 a block that exists where the env has one (any of them), 4 uniform over [0, R j) (mostly
    absent blocks), 5 a negative one, 6 R j (the mask's reject column), 7 beyond it"""
    out = np.zeros(rows.n, np.int32)
    for i in range(rows.n):
        kind = i % 8
        have = [r * j + b for r in range(rows.R) for b in range(min(j, len(blocks_of(rows, i, r))))]
        if kind <= 3 and have:
            out[i] = have[int(rng.integers(len(have)))]
        elif kind <= 4:
            out[i] = rng.integers(rows.R * j)
        else:
            out[i] = -1 - int(rng.integers(3)) if kind == 5 else rows.R * j + (0 if kind == 6 else 1 + int(rng.integers(5)))
    return out


def count_kinds(rows, j, seen):
    """Adds to `seen` what the state's usable rows hold (KINDS), for a table of j blocks per row"""
    def count(kind, yes):
        seen[kind] = seen.get(kind, 0) + int(bool(yes))

    S = rows.S
    for i in range(rows.n):
        count("no_modulation", rows.env_type == 3 and any(n == 0 for n in rows.need[i]))
        for r in range(rows.R):
            n = rows.need[i][r]
            if n == 0:
                continue
            runs = runs_of(rows.row[i][r])
            fit = [(st, L) for st, L in runs if L >= n]
            count("runs_0", len(fit) == 0)
            count("runs_below_j", 1 <= len(fit) < j)
            count("runs_j", len(fit) == j)
            count("runs_above_j", len(fit) > j)
            count("ends_at_top", any(st + L == S for st, L in fit))
            count("starts_at_0", any(st == 0 for st, L in fit))
            count("exactly_n", any(L == n for st, L in fit))
            count("across_word", any(st // 64 != (st + L - 1) // 64 for st, L in fit))
            idx = [k for k, (st, L) in enumerate(runs) if L >= n]
            count("short_between", any(b - a > 1 for a, b in zip(idx, idx[1:])))
    seen["fixed_beyond_reach"] = seen.get("fixed_beyond_reach", 0) + rows.fixed_beyond_reach
    return seen


def craft(env_type, avail, services, topo, tables=None):
    """Slot maps for the kinds, whatever the walk left: `avail` (bool [n, C, links, S]) rewritten by env index mod 6, every row of the env
    alike, n = the slots of the service on its path 0 (an env whose path 0 the service cannot use keeps its map) —
      0  a comb from slot 0: free runs of n, n - 1, n + 1, n, ... slots between single taken slots (a block at 0, blocks of exactly n,
         a run one short of n between two blocks, more blocks than a small j lists)
      1  only the top n + 1 slots free: one block, which ends at S - 1
      2  [0, n) and [62, 62 + n + 2) free where S has them: two blocks, the second across the edge of the first word
      3  three runs of n + 1 slots from slot 1: exactly 3 blocks
      4  the first link of path 0 taken whole in every core: rows of path 0 without a block
      5  thinned at random with a probability that grows with the index"""
    out = avail.copy()
    n_env, C, _, S = avail.shape
    rng = np.random.default_rng(3 * S + C)
    rows = Rows(env_type, avail, services, topo, tables)
    for i in range(n_env):
        n = rows.need[i][0]
        if n == 0:
            continue
        src, dst = int(services[i, 2]), int(services[i, 3])
        kind, pat = i % 6, np.zeros(S, bool)
        if kind == 0:
            s, t = 0, 0
            while s < S:
                L = (n, n - 1, n + 1)[t % 3]
                pat[s:s + L] = True
                s += L + 1
                t += 1
        elif kind == 1:
            pat[max(S - n - 1, 0):] = True
        elif kind == 2:
            pat[:n] = True
            pat[62:62 + n + 2] = True
        elif kind == 3:
            for t in range(3):
                pat[1 + t * (n + 2):1 + t * (n + 2) + n + 1] = True
        elif kind == 4:
            out[i, :, int(topo.path_links[src, dst, 0, 0]), :] = False
            continue
        else:
            out[i] &= rng.random(out[i].shape) >= 0.04 * (1 + (i // 6) % 12)
            continue
        out[i] = pat[None, None, :]
    return out
