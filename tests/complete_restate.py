"""Numpy restatement of the first-fit completion of partial RMCSA actions (include/orl.h, orl_batch_complete_actions), on
rmcsa_mask_restate.prov_all — prov(p, m, c, s) of every action, written from the reference's definitions — and the batch's tables.
Test infrastructure only.

For an env whose first g action columns are given: g = 3 the lowest s with prov(p, m, c, s); g = 2 the lowest column c * S + s with
prov(p, m, c, s); g = 1 the modulation m*(p) — within both reach limits, fewest slots at the service's bit rate, ties to the lowest
index — then as g = 2; g = 0 the first path whose g = 1 completion exists.  No completion: the reject action (k, M, C, S)."""
import numpy as np

from tests import rmcsa_mask_restate as rr

KINDS = ("last_start", "upper_core", "later_path", "by_reach", "by_occupancy", "other_modulation")


def slots_of(services, tables):
    """[n, M]: slots of each env's pending service under every modulation"""
    return tables["n_slots"][np.array([tables["rate_index"][int(b)] for b in services[:, 4]], np.int64)]


def reach_of(services, topo, tables):
    """bool [n, k, M]: the path exists and its length is below both reach limits of the modulation at the service's bit rate"""
    src, dst = services[:, 2].astype(np.int64), services[:, 3].astype(np.int64)
    br = np.array([tables["rate_index"][int(b)] for b in services[:, 4]], np.int64)
    length = tables["path_length"][src, dst][:, :, None]                      # [n, k, 1]
    has = np.arange(topo.k_paths)[None, :] < topo.n_paths[src, dst][:, None]  # [n, k]
    return has[:, :, None] & (length < tables["lmax_xt"][None, None, :]) & (length < tables["lmax_snr"].T[br][:, None, :])


def best_in_reach(services, topo, tables):
    """m*(p): int [n, k], -1 where no modulation is within reach for the path"""
    reach = reach_of(services, topo, tables)
    need = np.where(reach, slots_of(services, tables)[:, None, :], np.iinfo(np.int64).max)
    return np.where(reach.any(axis=2), need.argmin(axis=2), -1)  # (argmin: the first of equal minima)


def complete(pv, services, topo, tables, g, given=None):
    """int32 [n, 4]: the completion of every env's prefix given[i, :g] under pv = prov_all() of the same state."""
    n, K, M, C, S = pv.shape
    reject = (K, M, C, S)
    mstar = best_in_reach(services, topo, tables)
    out = np.zeros((n, 4), np.int32)

    def from_pair(i, p, m):
        if not (0 <= p < K and 0 <= m < M):
            return reject
        cols = np.flatnonzero(pv[i, p, m].reshape(C * S))
        return (p, m, int(cols[0]) // S, int(cols[0]) % S) if len(cols) else reject

    def from_path(i, p):
        if not 0 <= p < K or mstar[i, p] < 0:
            return reject
        return from_pair(i, p, int(mstar[i, p]))

    for i in range(n):
        pre = [int(v) for v in (given[i][:g] if g else ())]
        if g == 0:
            got = reject
            for p in range(K):
                got = from_path(i, p)
                if got != reject:
                    break
        elif g == 1:
            got = from_path(i, pre[0])
        elif g == 2:
            got = from_pair(i, pre[0], pre[1])
        else:
            assert g == 3
            p, m, c = pre
            got = reject
            if 0 <= p < K and 0 <= m < M and 0 <= c < C:
                s = np.flatnonzero(pv[i, p, m, c])
                if len(s):
                    got = (p, m, c, int(s[0]))
        out[i] = got
    return out


def complete_state(avail, services, topo, tables, g, given=None):
    """complete() from the slot maps (bool [n, C, links, S]) and pending services themselves"""
    return complete(rr.prov_all(avail, services, topo, tables), services, topo, tables, g, given)


def prov_under(pv, g, given=None):
    """bool [n]: some action with the env's prefix provisions — prov alone, no m*(p)"""
    n, K, M, C, S = pv.shape
    out = np.zeros(n, bool)
    for i in range(n):
        pre = [int(v) for v in (given[i][:g] if g else ())]
        if not all(0 <= v < hi for v, hi in zip(pre, (K, M, C))):
            continue
        out[i] = pv[(i,) + tuple(pre)].any()
    return out


class Seen:
    """What the completions of the checked states held (KINDS), for the preconditions."""

    def __init__(self):
        for k in KINDS:
            setattr(self, k, 0)

    def add(self, other):
        for k in KINDS:
            setattr(self, k, getattr(self, k) + getattr(other, k))
        return self

    def all_positive(self):
        return all(getattr(self, k) > 0 for k in KINDS)

    def count(self, pv, pv_free, services, topo, tables, g, given, done):
        """`done`: complete() of the same arguments; pv_free: prov_all() of the same state under tables without reach limits
        (free_tables)."""
        n, K, M, C, S = pv.shape
        need, reach = slots_of(services, tables), reach_of(services, topo, tables)
        rej = (done == np.array([K, M, C, S])).all(axis=1)
        idx = np.flatnonzero(~rej)
        p, m, c, s = (done[idx, j] for j in range(4))
        self.last_start += int((s + need[idx, m] == S).sum())
        self.upper_core += int((c > 0).sum())
        if g == 0:
            self.later_path += int((p > 0).sum())
        if g <= 1:
            best = tables["path_best_mod"][services[idx, 2].astype(np.int64), services[idx, 3].astype(np.int64), p]
            self.other_modulation += int((m != best).sum())
        # a reject: by reach alone (without the limits the prefix would provision), by occupancy alone (a modulation is within reach)
        room = prov_under(pv_free, g, given)
        for i in np.flatnonzero(rej):
            pre = tuple(int(v) for v in (given[i][:g] if g else ()))
            if not all(0 <= v < hi for v, hi in zip(pre, (K, M, C))):
                continue
            if reach[(i,) + pre[:2]].any():
                self.by_occupancy += 1
            elif room[i]:
                self.by_reach += 1


def free_tables(tables):
    """`tables` with both reach limits lifted"""
    return dict(tables, lmax_xt=np.full_like(tables["lmax_xt"], np.inf), lmax_snr=np.full_like(tables["lmax_snr"], np.inf))
