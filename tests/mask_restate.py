"""Numpy restatement of the action masks (include/orl.h, ORL_MASK_JOINT / ORL_MASK_PATH) from a slot map, the pending service
and the topology — written from the reference's definitions, not from the product code: is_path_free (rmsa_env.py:623-636),
get_available_blocks (rmsa_env.py:667-697) with DeepRMSAEnv.step's decode (deeprmsa_env.py:48-58), RWAEnv's wavelength test
(rwa_env.py:385-400) and the PathOnlyFirstFitAction loops (rmsa_env.py:848-871, rwa_env.py:518-533).  Test infrastructure only."""
import math

import numpy as np


def row_words(S):
    """64-bit words of a slot row in slots_packed() (the library's row widths 1, 2, 5, 8)."""
    return 1 if S <= 64 else 2 if S <= 128 else 5 if S <= 320 else 8


def unpack_slots(packed, n_links, S, row_words):
    """slots_packed() ([n, map_words] uint64, bit s of word s // 64 of a row = slot s free) -> bool [n, links, S] (one core)."""
    n = packed.shape[0]
    bits = np.unpackbits(np.ascontiguousarray(packed).view(np.uint8).reshape(n, -1), axis=1, bitorder="little")
    return bits[:, : n_links * row_words * 64].reshape(n, n_links, row_words * 64)[:, :, :S].astype(bool)


def _rle(a):
    """rmsa_env.py:651-665"""
    a = np.asarray(a)
    change = np.flatnonzero(a[1:] != a[:-1])
    ends = np.append(change, len(a) - 1)
    lengths = np.diff(np.append(-1, ends))
    starts = np.cumsum(np.append(0, lengths))[:-1]
    return starts, a[ends], lengths


def restate(env_type, avail, services, topo, k, S, j=1, channel_width=12.5, allow_rejection=False, layout="joint"):
    """bool [n, dim] for the envs whose slot maps are avail (bool [n, links, S]) and pending services `services` ([n, 6]:
    arrival, holding, source_id, destination_id, bit_rate, service_id), with the fallback of include/orl.h applied."""
    n = len(services)
    cpp = 1 if layout == "path" else (j if env_type == 1 else S)
    out = np.zeros((n, k * cpp + 1), bool)
    for i in range(n):
        src, dst, br = int(services[i, 2]), int(services[i, 3]), float(services[i, 4])
        for p in range(int(topo.n_paths[src, dst])):
            hops = int(topo.path_hops[src, dst, p])
            links = topo.path_links[src, dst, p, :hops]
            free = np.prod(avail[i, links, :].astype(np.int64), axis=0)  # get_available_slots
            if env_type == 2:
                ns = 1
            else:
                se = topo.modulations[int(topo.path_best_mod[src, dst, p])].spectral_efficiency
                ns = math.ceil(br / (se * channel_width)) + 1  # get_number_slots
            # is_path_free(path, s, ns) for every s (RWA: ns = 1, the wavelength test)
            fits = np.array([s + ns <= S and not np.any(free[s:s + ns] == 0) for s in range(S)], bool)
            if layout == "path":
                last = S - ns if env_type == 0 else S  # range(0, S - n) / range(S)
                out[i, p] = bool(fits[:max(last, 0)].any())
            elif env_type == 1:
                starts, values, lengths = _rle(free)
                nb = len(np.intersect1d(np.where(values == 1), np.where(lengths >= ns))[:j])
                out[i, p * j:p * j + nb] = True
            else:
                out[i, p * S:(p + 1) * S] = fits
        if not out[i, :-1].any() and not allow_rejection:
            out[i, :-1] = True
        out[i, -1] = bool(allow_rejection)
    return out


def restate_fast(env_type, avail, services, topo, k, S, j=1, channel_width=12.5, allow_rejection=False, layout="joint",
                 fallback=True):
    """The same, vectorised over envs (for full-size batches); checked against restate() in tests/test_action_mask.py.
    fallback=False: the provisioning columns as they are (a row where nothing provisions stays all 0) — what tells a fallback
    row apart from a row where every action provisions."""
    n = len(services)
    cpp = 1 if layout == "path" else (j if env_type == 1 else S)
    out = np.zeros((n, k * cpp + 1), bool)
    src, dst, br = services[:, 2].astype(np.int64), services[:, 3].astype(np.int64), services[:, 4]
    se = np.array([m.spectral_efficiency for m in topo.modulations], np.float64)
    H = topo.path_links.shape[-1]
    rows = np.arange(n)
    for p in range(k):
        has = topo.n_paths[src, dst] > p
        hops = topo.path_hops[src, dst, p]
        m = np.ones((n, S), bool)
        for h in range(H):
            link = topo.path_links[src, dst, p, h]
            on = has & (h < hops)
            m &= np.where(on[:, None], avail[rows, np.maximum(link, 0), :], True)
        m &= has[:, None]
        if env_type == 2:
            ns = np.ones(n, np.int64)
        else:
            eff = se[topo.path_best_mod[src, dst, p]]
            ns = np.array([math.ceil(b / (e * channel_width)) + 1 for b, e in zip(br, eff)], np.int64)
        c = np.concatenate([np.zeros((n, 1), np.int64), np.cumsum(m, axis=1)], axis=1)
        s = np.arange(S)[None, :]
        end = s + ns[:, None]
        fits = (end <= S) & (np.take_along_axis(c, np.minimum(end, S), axis=1) - c[:, :S] == ns[:, None])
        if layout == "path":
            last = (S - ns) if env_type == 0 else np.full(n, S)
            out[:, p] = (fits & (s < last[:, None])).any(axis=1)
        elif env_type == 1:
            starts = m & ~np.concatenate([np.zeros((n, 1), bool), m[:, :-1]], axis=1)
            nb = np.minimum((starts & fits).sum(axis=1), j)
            out[:, p * j:(p + 1) * j] = np.arange(j)[None, :] < nb[:, None]
        else:
            out[:, p * S:(p + 1) * S] = fits
    if fallback and not allow_rejection:
        fb = ~out[:, :-1].any(axis=1)
        out[fb, :-1] = True
    out[:, -1] = bool(allow_rejection)
    return out
