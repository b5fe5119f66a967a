"""Plain numpy restatement of the release horizons (include/orl.h, orl_batch_release_horizons), written from the definition there: a
loop per release record, candidate row and slot.  Test infrastructure only; shares no code with the kernel.

For env e with clock now = services()[e, 0] and row r of the path features' row order (r = p; RMCSA: r = p C + c):
  H[r][s] = float32(max over the pending releases v that cover (r, s) of time(v) - now), the maximum and the subtraction in float64,
            one rounding; 0 where none covers it; -1 throughout a row whose path does not exist
v covers (r, s): its path shares a link with path p of the pending pair, its core is c (RMCSA), slot(v) <= s < slot(v) + max(n(v), 1).
The BLOCKS rows take, for the blocks of tests/block_restate.py, the two neighbours (H[r][start - 1], H[r][start + L]), +inf beyond
the spectrum's edge, (-1, -1) for a block that does not exist or a row the service cannot use.  Both end in float32(holding time).

times: float64 [m]; recs: int [m, >= 5] in the column order of BatchedOpticalEnv.pending() (src * N + dst, path, first slot, slots, core)."""
import numpy as np

from tests import block_restate as br


def link_set(topo, src, dst, p):
    return set(int(l) for l in topo.path_links[src, dst, p, :int(topo.path_hops[src, dst, p])])


def slots_rows(times, recs, service, topo, C, S, seen=None):
    """float32 [K C, S] of one env; seen: a dict the kinds of the state are counted into"""
    K, N = topo.k_paths, topo.n_nodes
    now = np.float64(service[0])
    src, dst = int(service[2]), int(service[3])
    n_paths = int(topo.n_paths[src, dst])
    best = np.full((K * C, S), -np.inf, np.float64)
    count = np.zeros((K * C, S), np.int64)
    lo_t = np.full((K * C, S), np.inf, np.float64)
    cand = [link_set(topo, src, dst, p) if p < n_paths else set() for p in range(K)]
    shares_none = other_core = 0
    for t, r in zip(times, recs):
        pair, vp, slot, n, core = (int(x) for x in r[:5])
        links = link_set(topo, pair // N, pair % N, vp)
        hit = False
        for p in range(K):
            if not (links & cand[p]):
                continue
            hit = True
            for c in range(C):
                if c != core:
                    other_core += 1
                    continue
                for s in range(slot, slot + max(n, 1)):
                    best[p * C + c, s] = max(best[p * C + c, s], np.float64(t))
                    lo_t[p * C + c, s] = min(lo_t[p * C + c, s], np.float64(t))
                    count[p * C + c, s] += 1
        shares_none += not hit
    H = np.zeros((K * C, S), np.float32)
    covered = count > 0
    H[covered] = (best[covered] - now).astype(np.float32)
    H[n_paths * C:] = -1.0
    if seen is not None:
        def add(kind, v):
            seen[kind] = seen.get(kind, 0) + int(v)
        add("two_services_one_slot", ((count > 1) & (lo_t < best)).any())
        live = H[:n_paths * C]
        add("row_all_free", (live == 0).all(axis=1).any())
        add("row_all_busy", (live > 0).all(axis=1).any())
        if S > 64:
            add("edge_63_64_differ", ((live[:, 63] > 0) & (live[:, 64] > 0) & (live[:, 63] != live[:, 64])).any())
        add("shares_no_link", shares_none > 0)
        add("other_core", other_core > 0)
        add("over_128", len(times) > 128)
        add("none_pending", len(times) == 0)
        add("missing_path", n_paths < K)
    return H


def slots_layout(pending, services, topo, C, S, seen=None):
    """float32 [n, K C S + 1]; pending: per env (times, recs)"""
    out = np.zeros((len(services), topo.k_paths * C * S + 1), np.float32)
    for e, (t, r) in enumerate(pending):
        out[e, :-1] = slots_rows(t, r, services[e], topo, C, S, seen).ravel()
        out[e, -1] = np.float32(services[e, 1])
    return out


def blocks_layout(H, rows, j, services, seen=None):
    """float32 [n, R 2 j + 1] from the SLOTS layout H [n, R S + 1] and the block list of block_restate.Rows"""
    n, R, S = rows.n, rows.R, rows.S
    out = np.full((n, R * 2 * j + 1), -1.0, np.float32)
    inf = np.float32(np.inf)
    for e in range(n):
        h = H[e, :-1].reshape(R, S)
        for r in range(R):
            blocks = br.blocks_of(rows, e, r)
            for b, (st, L) in enumerate(blocks[:j]):
                out[e, r * 2 * j + 2 * b] = h[r, st - 1] if st > 0 else inf
                out[e, r * 2 * j + 2 * b + 1] = h[r, st + L] if st + L < S else inf
            if seen is not None:
                seen["block_at_0"] = seen.get("block_at_0", 0) + int(any(st == 0 for st, L in blocks[:j]))
                seen["block_ends_at_S"] = seen.get("block_ends_at_S", 0) + int(any(st + L == S for st, L in blocks[:j]))
                seen["fewer_than_j"] = seen.get("fewer_than_j", 0) + int(rows.need[e][r] > 0 and len(blocks) < j)
                seen["unusable_row"] = seen.get("unusable_row", 0) + int(rows.need[e][r] == 0)
        out[e, -1] = np.float32(services[e, 1])
    return out
