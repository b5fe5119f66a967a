"""Numpy restatement of MatrixObservationWithPaths (qos_constrained_ra.py:440-493; include/orl.h,
orl_batch_matrix_paths_observation) from the link counters, the pending service and the topology, written from the reference's
loop, not from the product code.  Test infrastructure only.

  spectrum  int [n, E]: topology.graph["available_spectrum"] (free units per link)
  pending   int [n, 3]: (source_id, destination_id, service_class) of the pending service
  topo      optical_rl_gym_amd.topology.Topology (n_paths, path_hops, path_links)
Both forms return uint8 [n, E * S * (k + 1) + 1]: the [E, (k + 1) S] matrix flattened row-major, then the class."""
import numpy as np


def restate(spectrum, pending, topo, S, k):
    """The reference's loop, one env at a time (its float64 matrix as uint8: every entry is 0 or 1)."""
    n, E = spectrum.shape
    out = np.zeros((n, E * S * (k + 1) + 1), np.uint8)
    for i in range(n):
        a = [int(x) for x in spectrum[i]]
        src, dst, cls = (int(x) for x in pending[i])
        obs = np.zeros((E, S * (k + 1)))
        for link in range(E):
            obs[link, 0:S - a[link]] = 1
        for p in range(int(topo.n_paths[src, dst])):
            start = (p + 1) * S
            for link in topo.path_links[src, dst, p, :int(topo.path_hops[src, dst, p])]:
                obs[link, start:start + S - a[link] + 1] = 1  # (numpy clips the slice at the end of the row, as there)
            if cls == 0:
                break  # high-priority services only accept the shortest path
        out[i, :-1] = obs.reshape(-1)
        out[i, -1] = cls
    return out


def on_allowed_paths(pending, topo, E, k):
    """bool [n, E, k]: link l lies on allowed path p of the env's pending pair (p < n_paths, and p = 0 for class 0)."""
    n = len(pending)
    src, dst, cls = (np.asarray(pending[:, j], np.int64) for j in range(3))
    n_paths = topo.n_paths[src, dst]
    on = np.zeros((n, E, k), bool)
    rows = np.arange(n)
    for p in range(k):
        allowed = (p < n_paths) & ((cls != 0) | (p == 0))
        hops = topo.path_hops[src, dst, p]
        links = topo.path_links[src, dst, p]
        for h in range(links.shape[1]):
            sel = allowed & (h < hops)
            on[rows[sel], links[sel, h], p] = True
    return on


def run_lengths(spectrum, pending, topo, S, k):
    """int64 [n, E, k + 1]: the length of the run of ones that opens block b of link l (the closed form of include/orl.h)."""
    n, E = spectrum.shape
    a = np.asarray(spectrum, np.int64)
    on = on_allowed_paths(pending, topo, E, k)
    L = np.zeros((n, E, k + 1), np.int64)
    L[:, :, 0] = S - a
    full = np.minimum(S - a + 1, S)
    for b in range(1, k + 1):
        spill = on[:, :, b - 2] & (a == 0) if b >= 2 else np.zeros((n, E), bool)
        L[:, :, b] = np.where(on[:, :, b - 1], full, np.where(spill, 1, 0))
    return L


def restate_fast(spectrum, pending, topo, S, k):
    """The same rows from the closed form: block b of link l = ones in its first len(l, b) columns."""
    n, E = spectrum.shape
    L = run_lengths(spectrum, pending, topo, S, k)
    out = np.empty((n, E * S * (k + 1) + 1), np.uint8)
    out[:, :-1] = (np.arange(S)[None, None, None, :] < L[..., None]).reshape(n, -1)
    out[:, -1] = np.asarray(pending[:, 2], np.int64)
    return out


def spills(spectrum, pending, topo, k):
    """bool [n]: the row has a spill column — a link without a free unit on allowed path p, not on path p + 1, p + 2 <= k."""
    n, E = spectrum.shape
    on = on_allowed_paths(pending, topo, E, k)
    empty = (np.asarray(spectrum) == 0)[:, :, None]
    return (empty & on[:, :, :-1] & ~on[:, :, 1:]).any(axis=(1, 2))
