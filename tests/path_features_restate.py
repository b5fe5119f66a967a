"""Numpy restatement of the path-feature observation (include/orl.h, orl_batch_path_features) from the slot maps, the pending
service, the topology and — RMCSA — the batch's tables; written from the reference's definitions, not from the product code:
DeepRMSAEnv.observation (deeprmsa_env.py:60-121) over get_available_slots (rmsa_env.py:638-649), get_number_slots (:610-621),
rle (:651-665) and get_available_blocks (:667-697), one row per path and, for RMCSA, per core in the order of
rmcsa_env.py:889-906.  Test infrastructure only.

Rows are float64 [n, 1 + 2 N + R (2 j + 3)]; the device holds np.float32 of them.  env_type: 0 RMSA, 1 DeepRMSA, 2 RWA, 3 RMCSA.
avail: bool [n, C, links, S] (C = 1 outside RMCSA); services: [n, 6] (arrival, holding, source_id, destination_id, bit_rate,
service_id); tables (RMCSA): rmcsa_mask_restate.tables_of(batch) or slot_agent.rmcsa_tables(case)."""
import math

import numpy as np

from tests.mask_restate import _rle


def shape_of(env_type, topo, C, j):
    R = topo.k_paths * (C if env_type == 3 else 1)
    return 1 + 2 * topo.n_nodes + R * (2 * j + 3), R


def slots_needed(env_type, topo, tables, src, dst, p, bit_rate, modulation=-1, channel_width=12.5):
    """get_number_slots of the pending service on path p (RWA: one wavelength; RMCSA: the table entry of the path's best modulation,
    or of `modulation` when it is not -1)."""
    if env_type == 2:
        return 1
    if env_type == 3:
        m = int(tables["path_best_mod"][src, dst, p]) if modulation == -1 else modulation
        return int(tables["n_slots"][tables["rate_index"][int(bit_rate)]][m])
    se = topo.modulations[int(topo.path_best_mod[src, dst, p])].spectral_efficiency
    return math.ceil(bit_rate / (se * channel_width)) + 1


def _header(env_type, services, N):
    n = len(services)
    src, dst = services[:, 2].astype(np.int64), services[:, 3].astype(np.int64)
    head = np.zeros((n, 1 + 2 * N))
    if env_type != 2:
        head[:, 0] = services[:, 4] / 100
    head[np.arange(n), 1 + np.minimum(src, dst)] = 1
    head[np.arange(n), 1 + N + np.maximum(src, dst)] = 1
    return head


def restate(env_type, avail, services, topo, j, tables=None, modulation=-1, channel_width=12.5):
    """The slow form: a loop per env, path and core over _rle, statement by statement as deeprmsa_env.py:71-108."""
    n, C, _, S = avail.shape
    if env_type != 3:
        assert C == 1
    N, K = topo.n_nodes, topo.k_paths
    dim, R = shape_of(env_type, topo, C, j)
    out = np.zeros((n, dim))
    out[:, :1 + 2 * N] = _header(env_type, services, N)
    for i in range(n):
        src, dst, br = int(services[i, 2]), int(services[i, 3]), float(services[i, 4])
        spectrum_obs = np.full((R, 2 * j + 3), fill_value=-1.0)
        for p in range(int(topo.n_paths[src, dst])):
            links = topo.path_links[src, dst, p, :int(topo.path_hops[src, dst, p])]
            num_slots = slots_needed(env_type, topo, tables, src, dst, p, br, modulation, channel_width)
            for c in range(C):
                r = p * C + c
                available_slots = np.prod(avail[i, c][links, :].astype(np.int64), axis=0)  # get_available_slots
                starts, values, lengths = _rle(available_slots)
                ok = np.intersect1d(np.where(values == 1), np.where(lengths >= num_slots))[:j]  # get_available_blocks
                for idb, (initial_index, length) in enumerate(zip(starts[ok], lengths[ok])):
                    spectrum_obs[r, idb * 2 + 0] = 2 * (initial_index - 0.5 * S) / S
                    spectrum_obs[r, idb * 2 + 1] = (length - 8) / 8
                spectrum_obs[r, j * 2] = (num_slots - 5.5) / 3.5
                spectrum_obs[r, j * 2 + 1] = 2 * (np.sum(available_slots) - 0.5 * S) / S
                av_indices = np.argwhere(values == 1)
                if av_indices.shape[0] > 0:
                    spectrum_obs[r, j * 2 + 2] = (np.mean(lengths[av_indices]) - 4) / 4
        out[i, 1 + 2 * N:] = spectrum_obs.reshape(-1)
    return out


def restate_fast(env_type, avail, services, topo, j, tables=None, modulation=-1, channel_width=12.5):
    """The same, vectorised over envs (for whole batches); checked against restate() in tests/test_path_features.py."""
    n, C, _, S = avail.shape
    N, K = topo.n_nodes, topo.k_paths
    dim, R = shape_of(env_type, topo, C, j)
    WD = 2 * j + 3
    out = np.full((n, dim), -1.0)
    out[:, :1 + 2 * N] = _header(env_type, services, N)
    src, dst, br = services[:, 2].astype(np.int64), services[:, 3].astype(np.int64), services[:, 4]
    rows, s_idx = np.arange(n), np.arange(S)
    H = topo.path_links.shape[-1]
    if env_type == 3:
        br_row = np.array([tables["rate_index"][int(b)] for b in br], np.int64)
    else:
        se = np.array([m.spectral_efficiency for m in topo.modulations], np.float64)
    for p in range(K):
        has = topo.n_paths[src, dst] > p
        hops = topo.path_hops[src, dst, p]
        if env_type == 2:
            ns = np.ones(n, np.int64)
        elif env_type == 3:
            mod = tables["path_best_mod"][src, dst, p].astype(np.int64) if modulation == -1 else np.full(n, modulation, np.int64)
            ns = tables["n_slots"][br_row, mod].astype(np.int64)
        else:
            eff = se[topo.path_best_mod[src, dst, p]]
            ns = np.array([math.ceil(b / (e * channel_width)) + 1 for b, e in zip(br, eff)], np.int64)
        for c in range(C):
            m = np.ones((n, S), bool)
            for h in range(H):
                link = np.maximum(topo.path_links[src, dst, p, h], 0)
                m &= np.where((h < hops)[:, None], avail[rows, c, link, :], True)
            # maximal free runs: where they start, and for every slot the first busy slot at or after it (S: none)
            start = m & ~np.concatenate([np.zeros((n, 1), bool), m[:, :-1]], axis=1)
            nxt = np.minimum.accumulate(np.where(~m, s_idx[None, :], S)[:, ::-1], axis=1)[:, ::-1]
            length = nxt - s_idx[None, :]
            fit = start & (length >= ns[:, None])
            first = np.sort(np.where(fit, s_idx[None, :], S), axis=1)[:, :j]  # the first j fitting runs' starts, S = no such run
            if first.shape[1] < j:
                first = np.concatenate([first, np.full((n, j - first.shape[1]), S)], axis=1)
            got = first < S
            ln = np.take_along_axis(length, np.minimum(first, S - 1), axis=1)
            blk = np.full((n, WD), -1.0)
            blk[:, 0:2 * j:2] = np.where(got, 2 * (first - 0.5 * S) / S, -1.0)
            blk[:, 1:2 * j:2] = np.where(got, (ln - 8) / 8, -1.0)
            blk[:, 2 * j] = (ns - 5.5) / 3.5
            tot, nruns = m.sum(axis=1), start.sum(axis=1)
            blk[:, 2 * j + 1] = 2 * (tot - 0.5 * S) / S
            blk[:, 2 * j + 2] = np.where(nruns > 0, (tot / np.maximum(nruns, 1) - 4) / 4, -1.0)
            r = p * C + c
            lo = 1 + 2 * N + r * WD
            out[:, lo:lo + WD] = np.where(has[:, None], blk, -1.0)
    return out


def state_of(batch):
    """(env_type, avail bool [n, C, links, S], services) of a batch's read-back state — a device batch or the oracle stand-in."""
    from tests.rmcsa_mask_restate import unpack_cores

    C, S = batch.num_spatial_resources, batch.num_spectrum_resources
    return batch.ENV_TYPE, unpack_cores(batch.slots_packed(), C, batch.topology.n_links, S), batch.services().copy()


def of_batch(batch, j, modulation=None, tables=None, fast=True):
    """float64 rows of the batch's present state; RMCSA takes `tables` (default: rmcsa_mask_restate.tables_of(batch))."""
    env_type, avail, services = state_of(batch)
    if env_type == 3 and tables is None:
        from tests.rmcsa_mask_restate import tables_of

        tables = tables_of(batch)
    f = restate_fast if fast else restate
    return f(env_type, avail, services, batch.topology, j, tables, -1 if modulation is None else int(modulation))


def block_counts(rows64, services, topo, R, j):
    """Per block row of float64 rows [n, dim]: (the path exists, blocks listed, the row has a free slot) — bool / int / bool [n, R];
    what the tests' preconditions count."""
    blk = rows64[:, 1 + 2 * topo.n_nodes:].reshape(len(rows64), R, 2 * j + 3)
    src, dst = services[:, 2].astype(np.int64), services[:, 3].astype(np.int64)
    exists = (np.arange(R)[None, :] // (R // topo.k_paths)) < topo.n_paths[src, dst][:, None]
    listed = (blk[:, :, 1:2 * j:2] != -1.0).sum(axis=2)  # (length - 8) / 8 = -1 would need a run of length 0
    return exists, listed, blk[:, :, 2 * j + 2] != -1.0  # (mean - 4) / 4 = -1 would need a mean run length of 0


# ---- the walks of tests/test_path_features.py (over the oracle) and tests/test_path_features_gpu.py (on the device) -------------
# RMSA with S = 64 under a load that fills paths completely (rows without a free slot), RWA with 16 wavelengths likewise
RMSA_S64_KW = dict(load=300, mean_service_holding_time=25, episode_length=25, allow_rejection=True, num_spectrum_resources=64)
RWA_S16_KW = dict(load=200, mean_service_holding_time=25, num_spectrum_resources=16)
WALK_ENVS, WALK_POINTS = 64, (60, 120, 180)


def walk_seeds(S):
    """(chosen on the oracle: with these the S = 64 walk holds rows without a free slot at every checkpoint,
    tests/test_path_features.py::test_the_gpu_walks_hold_full_rows_on_the_oracle)"""
    return list(range(WALK_ENVS))


def random_actions(batch, rng):
    """DeepRMSA: uniformly random integer actions (reject included); RMSA / RWA: SAP_FF with 30 % random (path, slot) pairs."""
    n = batch.num_envs
    if batch.ENV_TYPE == 1:
        return rng.integers(0, batch.k_paths * batch.j + 1, size=(n, 1))
    a = batch.policy("SAP_FF")[:, :2].copy()
    pick = rng.random(n) < 0.3
    a[pick, 0] = rng.integers(0, batch.k_paths, size=pick.sum())
    a[pick, 1] = rng.integers(0, batch.num_spectrum_resources, size=pick.sum())
    return a


def walk(batch, rng, n_steps):
    for _ in range(n_steps):
        batch.step(random_actions(batch, rng), auto_reset=True)
