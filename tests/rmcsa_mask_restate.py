"""Numpy restatement of RMCSA's two-stage action masks (include/orl.h, ORL_MASK_PATH_MOD / ORL_MASK_CORE_SLOT) from the slot maps,
the pending service, the topology and the batch's tables — written from the reference's definitions, not from the product code:
RMCSAEnv.step (rmcsa_env.py:209-289) with is_path_free (:767-794), get_number_slots (:753-765) and _crosstalk_is_acceptable
(:341-384).  Test infrastructure only.

prov(p, m, c, s): stepping (path p, modulation m, core c, first slot s) provisions the pending service.  "path_modulation": column
p * M + m = some (c, s) has prov; "core_slot": column c * S + s = prov for the env's given (p, m).  Last column = allow_rejection;
a row without a provisioning column gets, when allow_rejection is off, every other column set (the fallback).

`tables`: slot_agent.rmcsa_tables(case) — n_slots [rate][mod], lmax_snr [mod][rate], lmax_xt [mod], rate_index {bit rate: row},
path_length [N, N, k] — or tables_of(batch) for a live batch."""
import numpy as np

LAYOUTS = ("path_modulation", "core_slot")


def tables_of(batch):
    """The same tables from a batch object (what it handed to the ABI), without deriving the configuration a second time."""
    keep = batch._keep
    return dict(n_slots=keep["n_slots"].astype(np.int64), lmax_snr=keep["lmax_snr"], lmax_xt=keep["lmax_xt"],
                rate_index={int(r): i for i, r in enumerate(keep["bit_rates"])}, path_length=keep["path_length"], path_best_mod=keep["path_mod"])


def prov(avail_e, service, topo, tables, p, m, c, s):
    """Does stepping (p, m, c, s) provision `service` in the env whose slot maps are avail_e (bool [C, links, S])?"""
    C, _, S = avail_e.shape
    src, dst = int(service[2]), int(service[3])
    br = tables["rate_index"][int(service[4])]
    if not (0 <= p < int(topo.n_paths[src, dst]) and 0 <= m < len(tables["lmax_xt"]) and 0 <= c < C and 0 <= s):
        return False
    n = int(tables["n_slots"][br][m])                                   # get_number_slots
    if s + n > S:                                                       # is_path_free: initial_slot + number_slots > S
        return False
    links = topo.path_links[src, dst, p, :int(topo.path_hops[src, dst, p])]
    if np.any(avail_e[c][links, s:s + n] == 0):
        return False
    length = tables["path_length"][src, dst, p]                         # _crosstalk_is_acceptable: both reach limits
    return bool(length < tables["lmax_xt"][m] and length < tables["lmax_snr"][m][br])


def _finish(body, allow_rejection, fallback):
    out = np.zeros((body.shape[0], body.shape[1] + 1), bool)
    out[:, :-1] = body
    if fallback and not allow_rejection:
        out[~body.any(axis=1), :-1] = True
    out[:, -1] = bool(allow_rejection)
    return out


def restate_rmcsa(avail, services, topo, tables, layout, given=None, allow_rejection=False, fallback=True):
    """bool [n, dim] for the envs whose slot maps are avail (bool [n, C, links, S]) and pending services `services` ([n, 6]);
    `given` ([n, 2] (path, modulation)) for "core_slot".  One prov() per column."""
    n, C, _, S = avail.shape
    K, M = topo.k_paths, len(tables["lmax_xt"])
    if layout == "path_modulation":
        body = np.zeros((n, K * M), bool)
        for i in range(n):
            for p in range(K):
                for m in range(M):
                    body[i, p * M + m] = any(prov(avail[i], services[i], topo, tables, p, m, c, s) for c in range(C) for s in range(S))
    else:
        assert layout == "core_slot"
        body = np.zeros((n, C * S), bool)
        for i in range(n):
            p, m = int(given[i][0]), int(given[i][1])
            for c in range(C):
                for s in range(S):
                    body[i, c * S + s] = prov(avail[i], services[i], topo, tables, p, m, c, s)
    return _finish(body, allow_rejection, fallback)


def prov_all(avail, services, topo, tables):
    """prov of every action at once: bool [n, k, M, C, S], vectorised over envs (free runs through cumulative sums, as
    slot_agent.rmcsa_agent_actions)."""
    n, C, _, S = avail.shape
    K, M = topo.k_paths, len(tables["lmax_xt"])
    src, dst = services[:, 2].astype(np.int64), services[:, 3].astype(np.int64)
    br = np.array([tables["rate_index"][int(b)] for b in services[:, 4]], np.int64)
    n_of = tables["n_slots"][br]                                        # [n, M]
    rows = np.arange(n)
    s_idx = np.arange(S)
    H = topo.path_links.shape[-1]
    out = np.zeros((n, K, M, C, S), bool)
    for p in range(K):
        has = topo.n_paths[src, dst] > p
        hops = topo.path_hops[src, dst, p]
        free = np.ones((n, C, S), bool)
        for h in range(H):
            link = np.maximum(topo.path_links[src, dst, p, h], 0)
            on = has & (h < hops)
            free &= np.where(on[:, None, None], avail[rows, :, link, :], True)
        cum = np.concatenate([np.zeros((n, C, 1), np.int64), np.cumsum(free, axis=2)], axis=2)
        length = tables["path_length"][src, dst, p]
        for m in range(M):
            nm = n_of[:, m]
            end = s_idx[None, :] + nm[:, None]                          # [n, S]
            hi = np.take_along_axis(cum, np.broadcast_to(np.minimum(end, S)[:, None, :], (n, C, S)), axis=2)
            fits = (end <= S)[:, None, :] & (hi - cum[:, :, :S] == nm[:, None, None])
            reach = has & (length < tables["lmax_xt"][m]) & (length < tables["lmax_snr"][m][br])
            out[:, p, m] = fits & reach[:, None, None]
    return out


def restate_rmcsa_fast(avail, services, topo, tables, layout, given=None, allow_rejection=False, fallback=True, pv=None):
    """The same as restate_rmcsa, vectorised (checked against it in tests/test_rmcsa_mask.py).  fallback=False: the provisioning
    columns as they are; pv: a prov_all() of the same state, computed once for several calls."""
    if pv is None:
        pv = prov_all(avail, services, topo, tables)
    n, K, M, C, S = pv.shape
    if layout == "path_modulation":
        body = pv.any(axis=(3, 4)).reshape(n, K * M)
    else:
        assert layout == "core_slot"
        g = np.asarray(given).astype(np.int64)
        ok = (g[:, 0] >= 0) & (g[:, 0] < K) & (g[:, 1] >= 0) & (g[:, 1] < M)
        body = pv[np.arange(n), np.clip(g[:, 0], 0, K - 1), np.clip(g[:, 1], 0, M - 1)].reshape(n, C * S) & ok[:, None]
    return _finish(body, allow_rejection, fallback)


def unpack_cores(packed, C, E, S):
    """slots_packed() -> bool [n, C, links, S]"""
    from tests.mask_restate import row_words, unpack_slots

    return unpack_slots(packed, C * E, S, row_words(S)).reshape(len(packed), C, E, S)


# ---- the two-stage uniformly random masked agent (tests/test_rmcsa_mask.py over the oracle, tests/test_rmcsa_mask_gpu.py on the device)
AGENT_ENVS, AGENT_STEPS, AGENT_SEED = 256, 200, 77
AGENT_KW = dict(load=150, num_spectrum_resources=64, num_spatial_resources=7, worst_xt=-84.7, allow_rejection=False,
                mean_service_holding_time=10.0, episode_length=40)
AGENT_SEEDS = [9000 + 3 * i for i in range(AGENT_ENVS)]


def sample_columns(mask, rng):
    """One uniformly drawn set column of every row's non-reject part (bool [n, dim]; every row has one)."""
    body = mask[:, :-1]
    kth = (rng.random(len(body)) * body.sum(axis=1)).astype(np.int64)
    return (np.cumsum(body, axis=1) > kth[:, None]).argmax(axis=1)


def two_stage_walk(batch, masks, M, n_steps=AGENT_STEPS, seed=AGENT_SEED):
    """Stage 1 from "path_modulation", stage 2 from "core_slot" under the sampled pair, then the step; masks(layout, given) hands
    out the rows of `batch`'s present state.  Returns (fallback [steps, n], accepted [steps, n]).  A fallback row is told by its
    core-slot stage: with every service at least 2 slots wide, column S - 1 of a core never provisions, so a core-slot row of
    ones only is the fallback's."""
    rng = np.random.default_rng(seed)
    S = batch.num_spectrum_resources
    fallback, accepted = [], []
    for _ in range(n_steps):
        col = sample_columns(masks("path_modulation", None), rng)
        pair = np.stack([col // M, col % M], axis=1).astype(np.int32)
        cs = masks("core_slot", pair)
        col2 = sample_columns(cs, rng)
        actions = np.concatenate([pair, np.stack([col2 // S, col2 % S], axis=1).astype(np.int32)], axis=1)
        before = batch.counters()[:, 1].copy()
        batch.step(actions, auto_reset=True)
        fallback.append(cs[:, :-1].all(axis=1))
        accepted.append(batch.counters()[:, 1] - before)
    return np.array(fallback), np.array(accepted)
