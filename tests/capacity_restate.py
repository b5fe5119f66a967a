"""Numpy restatement of the network capacity view (include/orl.h, orl_batch_network_capacity) from dense slot maps, the topology tables
and the per-(path, class) need table — written from the definitions in the header, not from the kernel.  Test infrastructure only.

For every path index pidx = (src N + dst) K + p and core c: m = the AND of the path's link rows in core c, L = its longest free run
(from a run-length encoding, not from shifts), F = its free slots.  need[src, dst, p, r] = the slots class r needs on the path, 0 where
the path cannot carry it.  serviceable[src, dst, r] = some existing path p and core c have need >= 1 and L >= need."""
import numpy as np

from tests import complete_restate as cr
from tests import slot_agent


def class_rates(fam, kw):
    """The bit rate of every class of a batch made with keywords kw: RWA one class (rate 0); the uniform mode every integer rate of
    its bounds; the discrete mode its bit_rates"""
    if fam == "RWA":
        return [0]
    if kw.get("bit_rate_selection", "continuous") == "discrete":
        return [int(b) for b in kw.get("bit_rates", (10, 40, 100))]
    return list(range(int(kw.get("bit_rate_lower_bound", 25)), int(kw.get("bit_rate_higher_bound", 100)) + 1))


def _all_services(topo, rates):
    """[N N n_cls, 6] service rows (source at column 2, destination 3, bit rate 4), pair-major"""
    N = topo.n_nodes
    src, dst, r = np.meshgrid(np.arange(N), np.arange(N), np.arange(len(rates)), indexing="ij")
    sv = np.zeros((src.size, 6), np.float64)
    sv[:, 2], sv[:, 3], sv[:, 4] = src.ravel(), dst.ravel(), np.asarray(rates, np.float64)[r.ravel()]
    return sv


def need_table(fam, topo, rates, tables=None):
    """int64 [N, N, K, n_cls]: the slots a service of class r needs on path p of (src, dst); 0: the path cannot carry it (RMCSA: no
    modulation within reach).  Entries of paths that do not exist mean nothing."""
    N, K, n_cls = topo.n_nodes, topo.k_paths, len(rates)
    if fam == "RWA":
        return np.ones((N, N, K, 1), np.int64)
    sv = _all_services(topo, rates)
    if fam == "RMCSA":
        mstar = cr.best_in_reach(sv, topo, tables)                     # [n, K], -1: none within reach
        slots = cr.slots_of(sv, tables)                                # [n, M]
        need = np.where(mstar >= 0, np.take_along_axis(slots, np.maximum(mstar, 0), axis=1), 0)
    elif K == slot_agent.K:
        need = slot_agent.slots_needed(sv, topo)                       # [n, K]
    else:  # (slots_needed is written for k = 5: the same expression over this topology's k)
        se = np.array([m.spectral_efficiency for m in topo.modulations], np.float64)
        s, d = sv[:, 2].astype(np.int64), sv[:, 3].astype(np.int64)
        need = np.stack([np.ceil(sv[:, 4] / (se[topo.path_best_mod[s, d, p]] * 12.5)).astype(np.int64) + 1 for p in range(K)], axis=1)
    return need.reshape(N, N, n_cls, K).transpose(0, 1, 3, 2).astype(np.int64)


def longest_runs(rows):
    """int64 [R]: the longest run of True in each row of bool [R, S], from the rows' run-length encoding"""
    R, S = rows.shape
    padded = np.zeros((R, S + 2), np.int8)
    padded[:, 1:-1] = rows
    edge = np.diff(padded, axis=1)              # +1 where a run starts, -1 one past its end; as many of each per row
    r0, starts = np.nonzero(edge == 1)
    _, ends = np.nonzero(edge == -1)            # (row-major order pairs the i-th start of a row with its i-th end)
    out = np.zeros(R, np.int64)
    np.maximum.at(out, r0, ends - starts)
    return out


def path_rows(avail, topo):
    """avail bool [n, C', E, S] -> bool [n, P, C', S] over the existing paths in path-table order, and their indices pidx [P]"""
    N, K = topo.n_nodes, topo.k_paths
    exists = (np.arange(K)[None, None, :] < topo.n_paths[:, :, None]).reshape(-1)
    pidx = np.flatnonzero(exists)
    hops = topo.path_hops.reshape(N * N * K)[pidx]
    links = topo.path_links.reshape(N * N * K, -1)[pidx]
    m = np.ones((avail.shape[0], len(pidx), avail.shape[1], avail.shape[3]), bool)
    for h in range(int(hops.max())):
        on = h < hops
        m[:, on] &= avail[:, :, links[on, h], :].transpose(0, 2, 1, 3)
    return m, pidx


def restate(avail, topo, need):
    """The three layouts of every env of avail (bool [n, C', E, S]): ("paths" int32 [n, N N K C' 2], "serviceable" bool [n, N N n_cls],
    "counts" int32 [n, n_cls + N N])"""
    n, C, _, S = avail.shape
    N, K, n_cls = topo.n_nodes, topo.k_paths, need.shape[3]
    m, pidx = path_rows(avail, topo)
    P = len(pidx)
    L = longest_runs(m.reshape(n * P * C, S)).reshape(n, P, C)
    F = m.sum(axis=3)
    paths = np.full((n, N * N * K, C, 2), -1, np.int32)
    paths[..., 0][:, pidx] = L
    paths[..., 1][:, pidx] = F
    best = np.zeros((n, N * N * K), np.int64)  # max over the cores; 0 for a path that does not exist
    best[:, pidx] = L.max(axis=2)
    nd = need.reshape(N * N * K, n_cls)
    exists = np.zeros(N * N * K, bool)
    exists[pidx] = True
    fits = exists[None, :, None] & (nd[None] >= 1) & (best[:, :, None] >= nd[None])  # [n, N N K, n_cls]
    serviceable = fits.reshape(n, N * N, K, n_cls).any(axis=2)
    has = (topo.n_paths.reshape(-1) > 0)
    counts = np.concatenate([(has[None, :, None] & ~serviceable).sum(axis=1), serviceable.sum(axis=2)], axis=1).astype(np.int32)
    return paths.reshape(n, -1), serviceable.reshape(n, -1), counts


def first_fit(avail_e, topo, need, src, dst, r):
    """(path, core, first slot, slots) of the first fitting run of class r between (src, dst) in env state avail_e (bool [C', E, S]):
    paths in order, then cores, then the lowest start; None where the cell is not serviceable"""
    C, _, S = avail_e.shape
    for p in range(int(topo.n_paths[src, dst])):
        n = int(need[src, dst, p, r])
        if n < 1:
            continue
        links = topo.path_links[src, dst, p, :int(topo.path_hops[src, dst, p])]
        for c in range(C):
            free = avail_e[c][links].all(axis=0)
            for s in range(S - n + 1):
                if free[s:s + n].all():
                    return p, c, s, n
    return None
