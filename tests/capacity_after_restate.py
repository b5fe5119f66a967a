"""Numpy restatement of capacity_after (include/orl.h, orl_batch_capacity_after) — written from the definition in the header, not from
the kernel: for every env and candidate (row, s, n) the window is taken out of the dense slot maps on the links of the candidate's path
in its core, and tests/capacity_restate.py's restate() counts the blocked (pair, class) cells of the result.  No delta, no sharing
between the candidates.  Test infrastructure only.

The candidates of the three sources are decoded here from the fetched tables (whose own contents tests/test_route_spectrum*.py,
tests/test_route_cores*.py and tests/test_block_actions*.py hold against their restatements)."""
import numpy as np

from tests import capacity_restate as cap

CHUNK = 64  # candidates per restate() call (germany50 at 10 cores of 512 slots: one at a time is what fits)


def route_candidates(table, S):
    """table int [n, R, 4] of (s*, c*, n, free) rows -> int64 [n, R, 3] of (row, s, n); n = 0 (absent) where s* >= S"""
    n, R, _ = table.shape
    out = np.zeros((n, R, 3), np.int64)
    out[:, :, 0] = np.arange(R)[None]
    out[:, :, 1] = table[:, :, 0]
    out[:, :, 2] = np.where(table[:, :, 0] >= S, 0, table[:, :, 2])
    return out


def block_candidates(table, j, placement, S):
    """table int [n, R, 2 + 2 j] of (n, free, start_0, L_0, ...) rows -> int64 [n, R j, 3]: candidate r j + b = block b of row r at its
    lower ("first") or upper end ("last"); n = 0 (absent) where start_b >= S"""
    n, R, _ = table.shape
    start, length = table[:, :, 2::2].astype(np.int64), table[:, :, 3::2].astype(np.int64)
    need = np.broadcast_to(table[:, :, :1].astype(np.int64), start.shape)
    out = np.zeros((n, R, j, 3), np.int64)
    out[..., 0] = np.arange(R)[None, :, None]
    out[..., 2] = np.where(start >= S, 0, need)
    out[..., 1] = start if placement == "first" else start + length - out[..., 2]
    return out.reshape(n, R * j, 3)


def present(cands, topo, src, dst, C, S):
    """bool [n, Q]: 0 <= row < k C', p < n_paths[pair], n >= 1, 0 <= s, s + n <= S"""
    row, s, n = (cands[..., i].astype(np.int64) for i in range(3))
    ok = (row >= 0) & (row < topo.k_paths * C) & (n >= 1) & (s >= 0) & (s + n <= S)
    p = np.where(ok, row, 0) // C
    return ok & (p < topo.n_paths[src, dst][:, None])


def pending_pairs(env):
    sv = env.services()
    return sv[:, 2].astype(np.int64), sv[:, 3].astype(np.int64)


def after(avail, topo, need, src, dst, cands, chunk=CHUNK, memo=None):
    """int32 [n, Q + 1, n_cls]: row q = the first n_cls columns of "counts" on env e's maps (avail bool [n, C', E, S]) less candidate q,
    -1 for an absent candidate; row Q the baseline.  Also the share of paths whose AND-row a present candidate can change (those sharing a
    link with its path) and of pairs owning such a path, summed over the present candidates: (paths touched, paths, pairs touched, pairs)."""
    n, C, _, S = avail.shape
    Q, n_cls = cands.shape[1], need.shape[3]
    ok = present(cands, topo, src, dst, C, S)
    out = np.full((n, Q + 1, n_cls), -1, np.int32)
    N, K = topo.n_nodes, topo.k_paths
    exists = (np.arange(K)[None, None, :] < topo.n_paths[:, :, None])
    link_sets = np.zeros((N, N, K, avail.shape[2]), bool)
    for (a, b, p) in zip(*np.nonzero(exists)):
        link_sets[a, b, p, topo.path_links[a, b, p, :int(topo.path_hops[a, b, p])]] = True
    share = np.zeros(4, np.int64)
    for e in range(n):
        key = None if memo is None else (avail[e].tobytes(), int(src[e]), int(dst[e]), cands[e].tobytes())
        if key is not None and key in memo:
            out[e], sh = memo[key]
            share += sh
            continue
        states, where, sh = [avail[e]], [Q], np.zeros(4, np.int64)
        seen = {}
        for q in np.flatnonzero(ok[e]):
            row, s, k = (int(x) for x in cands[e, q])
            if (row, s, k) in seen:
                continue
            seen[row, s, k] = q
            p, c = divmod(row, C)
            a = avail[e].copy()
            links = topo.path_links[src[e], dst[e], p, :int(topo.path_hops[src[e], dst[e], p])]
            a[c, links, s:s + k] = False
            states.append(a)
            where.append(q)
            touched = (link_sets & link_sets[src[e], dst[e], p]).any(axis=3)
            sh += (int(touched.sum()), int(exists.sum()), int(touched.any(axis=2).sum()), int((topo.n_paths > 0).sum()))
        for i in range(0, len(states), chunk):
            counts = cap.restate(np.stack(states[i:i + chunk]), topo, need)[2]
            out[e, where[i:i + chunk]] = counts[:, :n_cls]
        for q in np.flatnonzero(ok[e]):
            out[e, q] = out[e, seen[tuple(int(x) for x in cands[e, q])]]
        share += sh
        if key is not None:
            memo[key] = (out[e].copy(), sh)
    return out, tuple(int(x) for x in share)


def total(classes):
    """"total" of "classes" [n, Q + 1, n_cls]: the row sums, -1 where the row is -1 throughout (an absent candidate)"""
    absent = (classes == -1).all(axis=2)
    return np.where(absent, -1, classes.sum(axis=2)).astype(np.int32)


def pending_classes(fam, services, rates):
    """int64 [n]: the class of every env's pending service (RWA: 0)"""
    return np.zeros(len(services), np.int64) if fam == "RWA" else np.array([rates.index(int(b)) for b in services[:, 4]], np.int64)


def first_fit_candidates(avail, topo, need, src, dst, r):
    """int64 [n, k C', 3]: on every row (p, c) of the pending service the lowest window of need[src, dst, p, r] free slots; n = 0 (absent)
    where the row has none, the path does not exist or cannot carry the class"""
    n, C, _, S = avail.shape
    K = topo.k_paths
    out = np.zeros((n, K * C, 3), np.int64)
    out[:, :, 0] = np.arange(K * C)[None]
    for e in range(n):
        for p in range(int(topo.n_paths[src[e], dst[e]])):
            k = int(need[src[e], dst[e], p, r[e]])
            links = topo.path_links[src[e], dst[e], p, :int(topo.path_hops[src[e], dst[e], p])]
            for c in range(C if k >= 1 else 0):
                free = avail[e, c][links].all(axis=0)
                s = next((s for s in range(S - k + 1) if free[s:s + k].all()), None)
                if s is not None:
                    out[e, p * C + c, 1:] = (s, k)
    return out
