"""Numpy restatement of the per-link feature observation (include/orl.h, orl_batch_link_features) from the slot maps, the pending
service, the topology and the links' running statistics; written from the reference's definitions, not from the product code:
_update_link_stats (rmsa_env.py:482-528 = rmcsa_env.py:621-672) over rle (:651-665, tests/mask_restate._rle), the header of
DeepRMSAEnv.observation (deeprmsa_env.py:62-68).  Test infrastructure only.

Rows are float64 [n, 1 + 2 N + C E (10 + k)]; the device holds np.float32 of them.  env_type: 0 RMSA, 1 DeepRMSA, 2 RWA, 3 RMCSA.
avail: bool [n, C, links, S] (C = 1 outside RMCSA); services: [n, 6] (arrival, holding, source_id, destination_id, bit_rate,
service_id); lstat: link_stats_all(), [n, 4, links] (utilization, external_fragmentation, compactness, last_update)."""
import numpy as np

from tests.mask_restate import _rle
from tests.path_features_restate import _header, state_of

BASE = 10  # values per block in front of the k on-path columns


def shape_of(topo, C):
    """(dim, rows, width)"""
    R, F = C * topo.n_links, BASE + topo.k_paths
    return 1 + 2 * topo.n_nodes + R * F, R, F


def cur_stats(slot_allocation):
    """(cur_external_fragmentation, cur_link_compactness) of one row of available_slots (1 = free), statement for statement
    rmsa_env.py:492-528."""
    cur_external_fragmentation = 0.0
    cur_link_compactness = 0.0
    if np.sum(slot_allocation) > 0:
        initial_indices, values, lengths = _rle(slot_allocation)
        unused_blocks = [i for i, x in enumerate(values) if x == 1]
        max_empty = 0
        if len(unused_blocks) > 1 and unused_blocks != [0, len(values) - 1]:
            max_empty = max(lengths[unused_blocks])
        cur_external_fragmentation = 1.0 - (float(max_empty) / float(np.sum(slot_allocation)))
        used_blocks = [i for i, x in enumerate(values) if x == 0]
        if len(used_blocks) > 1:
            lambda_min = initial_indices[used_blocks[0]]
            lambda_max = initial_indices[used_blocks[-1]] + lengths[used_blocks[-1]]
            internal_idx, internal_values, internal_lengths = _rle(slot_allocation[lambda_min:lambda_max])
            unused_spectrum_slots = np.sum(1 - internal_values)
            if unused_spectrum_slots > 0:
                cur_link_compactness = ((lambda_max - lambda_min) / np.sum(1 - slot_allocation)) * (1 / unused_spectrum_slots)
            else:
                cur_link_compactness = 1.0
        else:
            cur_link_compactness = 1.0
    return cur_external_fragmentation, cur_link_compactness


def restate(env_type, avail, services, topo, lstat):
    """The slow form: a loop per env, core and link over _rle."""
    n, C, E, S = avail.shape
    if env_type != 3:
        assert C == 1
    N, K = topo.n_nodes, topo.k_paths
    dim, R, F = shape_of(topo, C)
    out = np.zeros((n, dim))
    out[:, :1 + 2 * N] = _header(env_type, services, N)
    for i in range(n):
        src, dst = int(services[i, 2]), int(services[i, 3])
        on_path = np.zeros((E, K))
        for p in range(int(topo.n_paths[src, dst])):
            on_path[topo.path_links[src, dst, p, :int(topo.path_hops[src, dst, p])], p] = 1.0
        blocks = np.zeros((C, E, F))
        for c in range(C):
            for l in range(E):
                a = avail[i, c, l].astype(np.int64)
                _starts, values, lengths = _rle(a)
                free_runs = lengths[values == 1]
                free_slots = np.flatnonzero(a)
                blk = blocks[c, l]
                blk[0] = np.sum(a) / S
                blk[1] = len(free_runs) / S
                blk[2] = (max(free_runs) if len(free_runs) else 0) / S
                blk[3] = free_slots[0] / S if len(free_slots) else -1.0
                blk[4] = (free_slots[-1] + 1) / S if len(free_slots) else -1.0
                blk[5], blk[6] = cur_stats(a)
                blk[7:10] = lstat[i, 0:3, l]
                blk[BASE:] = on_path[l]
        out[i, 1 + 2 * N:] = blocks.reshape(-1)
    return out


def row_facts(avail):
    """Integers of every row of avail (bool [..., S]), vectorised: free slots, free runs, longest free run and where it starts (the
    first of that length), first free slot, last free slot + 1, used runs, first used slot, last used slot + 1, free ends (0 .. 2)."""
    S = avail.shape[-1]
    m = np.asarray(avail, bool)
    s_idx = np.arange(S)
    pad = np.zeros(m.shape[:-1] + (1,), bool)
    start = m & ~np.concatenate([pad, m[..., :-1]], axis=-1)
    nxt = np.minimum.accumulate(np.where(~m, s_idx, S)[..., ::-1], axis=-1)[..., ::-1]  # the first busy slot at or after s (S: none)
    length = np.where(start, nxt - s_idx, 0)
    used = ~m
    ustart = used & ~np.concatenate([pad, used[..., :-1]], axis=-1)
    return dict(free=m.sum(-1), runs=start.sum(-1), longest=length.max(-1), longest_at=length.argmax(-1),
                first=m.argmax(-1), last=S - m[..., ::-1].argmax(-1), used_runs=ustart.sum(-1), lo=used.argmax(-1),
                hi=S - used[..., ::-1].argmax(-1), ends=m[..., 0].astype(np.int64) + m[..., -1])


def restate_fast(env_type, avail, services, topo, lstat):
    """The same, vectorised over envs, cores and links; checked against restate() in tests/test_link_features.py."""
    n, C, E, S = avail.shape
    N, K = topo.n_nodes, topo.k_paths
    dim, R, F = shape_of(topo, C)
    q = row_facts(avail)
    f, any_free = q["free"], q["free"] > 0
    blocks = np.zeros((n, C, E, F))
    blocks[..., 0] = f / S
    blocks[..., 1] = q["runs"] / S
    blocks[..., 2] = q["longest"] / S
    blocks[..., 3] = np.where(any_free, q["first"] / S, -1.0)
    blocks[..., 4] = np.where(any_free, q["last"] / S, -1.0)
    max_empty = np.where((q["runs"] > 1) & ~((q["runs"] == 2) & (q["ends"] == 2)), q["longest"], 0)
    blocks[..., 5] = np.where(any_free, 1.0 - max_empty.astype(np.float64) / np.maximum(f, 1).astype(np.float64), 0.0)
    comp = ((q["hi"] - q["lo"]) / np.maximum(S - f, 1)) * (1 / np.maximum(q["used_runs"], 1))
    blocks[..., 6] = np.where(any_free, np.where(q["used_runs"] > 1, comp, 1.0), 0.0)
    blocks[..., 7:10] = np.transpose(lstat[:, 0:3, :], (0, 2, 1))[:, None, :, :]
    src, dst = services[:, 2].astype(np.int64), services[:, 3].astype(np.int64)
    on_path = np.zeros((n, E, K))
    rows = np.arange(n)
    for p in range(K):
        has = topo.n_paths[src, dst] > p
        hops = topo.path_hops[src, dst, p]
        for h in range(topo.path_links.shape[-1]):
            on = np.flatnonzero(has & (h < hops))
            on_path[on, topo.path_links[src[on], dst[on], p, h], p] = 1.0
    blocks[..., BASE:] = on_path[:, None, :, :]
    out = np.zeros((n, dim))
    out[:, :1 + 2 * N] = _header(env_type, services, N)
    out[:, 1 + 2 * N:] = blocks.reshape(n, -1)
    return out


def of_batch(batch, fast=True):
    """float64 rows of the batch's present state (a device batch or the oracle stand-in)."""
    env_type, avail, services = state_of(batch)
    return (restate_fast if fast else restate)(env_type, avail, services, batch.topology, batch.link_stats_all())


def blocks_of(rows64, topo, C):
    """[n, C, links, 10 + k] view of the blocks of float64 or float32 rows"""
    dim, R, F = shape_of(topo, C)
    return rows64[:, 1 + 2 * topo.n_nodes:dim].reshape(len(rows64), C, topo.n_links, F)


class Seen:
    """What the rows of the checked states held, for the preconditions of the walks: entirely free rows, rows without a free slot,
    rows whose longest free run crosses a 64-slot word boundary, rows whose last slot S - 1 is free."""

    def __init__(self):
        self.free_rows = self.full_rows = self.crossing = self.top_free = 0

    def add(self, avail):
        S = avail.shape[-1]
        q = row_facts(avail)
        self.free_rows += int((q["free"] == S).sum())
        self.full_rows += int((q["free"] == 0).sum())
        end = q["longest_at"] + q["longest"] - 1
        self.crossing += int(((q["longest"] > 0) & (q["longest"] < S) & (q["longest_at"] // 64 != end // 64)).sum())
        self.top_free += int(avail[..., S - 1].sum())


# What the walks of tests/test_link_features_gpu.py hold at their checkpoints (pf.WALK_ENVS envs, pf.walk_seeds, pf.WALK_POINTS,
# rng = default_rng(S)), shown on the oracle by tests/test_link_features.py::test_the_gpu_walks_hold_their_rows_on_the_oracle:
# case -> the attributes of Seen that are at least 1
WALK_HOLDS = {
    "rmsa_s64": ("free_rows",),
    "rmsa_s65": ("top_free", "free_rows", "crossing"),
    "rmsa_s129": ("crossing", "free_rows"),
    "rmsa_s512": ("crossing", "free_rows"),
    "rwa_s16": ("full_rows", "free_rows"),  # (the RMSA walks fill paths, never a single link: the full rows are RWA's)
    "rwa_s65": ("top_free",),
}
