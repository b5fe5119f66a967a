"""The states tests/test_route_cores.py (oracle, no GPU) and tests/test_route_cores_gpu.py (device) check the core and spectrum rules on,
beyond the walked ones: crafted slot maps under the walked pending services, the prefixes drawn by env index, and the one fixed
modulation a shape is checked under.  Test infrastructure only."""
import numpy as np

from tests import complete_restate as cr

SHAPES = ("rmcsa_c7_s64", "rmcsa_c3_s128", "rmcsa_c2_s129")  # the shapes walked on the oracle too (tests/test_rmcsa_complete.py's)


def craft(avail, services, topo, tab):
    """Slot maps [n, C, links, S] rewritten by env index mod 6, n = the slots of m*(path 0) (an env whose path 0 has no modulation
    within reach keeps its map; a pattern that names more cores than the shape has wraps mod C):
      0  everything free except slot n + 1 on every row: min_cuts wins at 0 with 0 cuts
      1  core 0 full, in core 1 the first link of path 0 keeps only its top n slots, the other cores free: ksp lands in an upper
         core at S - n, best and least_loaded leave it
      2  only the top n + 2 slots free everywhere: min_cuts wins at S - n, first fit at S - n - 2
      3  the first link of path 0 full in every core: a later path is chosen
      4  every core keeps only [0, n + 3) free, core C - 1 only [5, 5 + n): exact fit costs 0 in the last core only
      5  thinned at random with a probability growing with the index: ties and rows without a fit"""
    out = avail.copy()
    n_env, C, _, S = avail.shape
    rng = np.random.default_rng(S + 7 * C)
    mstar, need = cr.best_in_reach(services, topo, tab), cr.slots_of(services, tab)
    for i in range(n_env):
        if mstar[i, 0] < 0:
            continue
        n = int(need[i, int(mstar[i, 0])])
        src, dst = int(services[i, 2]), int(services[i, 3])
        first_link = int(topo.path_links[src, dst, 0, 0])
        kind = i % 6
        if kind == 0:
            out[i] = True
            if n + 1 < S:
                out[i, :, :, n + 1] = False
        elif kind == 1:
            out[i] = True
            out[i, 0] = False
            out[i, 1 % C, first_link, :S - n] = False
        elif kind == 2:
            out[i] = False
            out[i, :, :, max(S - n - 2, 0):] = True
        elif kind == 3:
            out[i, :, first_link, :] = False
        elif kind == 4:
            out[i] = False
            out[i, :, :, :n + 3] = True
            lo = min(5, S - n)
            out[i, C - 1] = False
            out[i, C - 1, :, lo:lo + n] = True
        else:
            out[i] &= rng.random(out[i].shape) >= 0.04 * (1 + (i // 6) % 12)
    return out


def draw_given(n_env, K, C, g, shift=0):
    """A prefix int32 [n, g] (path) or (path, core) by env index mod 7: 0 - 2 in range (the path may still lie beyond n_paths), 3 the
    path = K, 4 a negative path, 5 the core = C (g = 1: path K + 2), 6 a negative core (g = 1: path -3)."""
    given = np.zeros((n_env, 2), np.int32)
    for i in range(n_env):
        kind = i % 7
        p, c = (i // 7 + i + shift) % K, (i // 3 + shift) % C
        if kind == 3:
            p = K
        elif kind == 4:
            p = -1 - (i % 2)
        elif kind == 5:
            p, c = (K + 2, c) if g == 1 else (p, C)
        elif kind == 6:
            p, c = (-3, c) if g == 1 else (p, -1)
        given[i] = (p, c)
    return np.ascontiguousarray(given[:, :g])


def fixed_modulation(services, topo, tab):
    """The one fixed modulation a state is checked under: the one within reach on the most (env, path) pairs that is not within reach
    on all of them (so that it leaves paths beyond reach); the last one if every modulation reaches all or nothing."""
    reach = cr.reach_of(services, topo, tab)
    share = reach.sum(axis=(0, 1))
    total = reach.shape[0] * reach.shape[1]
    partial = [m for m in range(reach.shape[2]) if 0 < share[m] < total]
    return max(partial, key=lambda m: share[m]) if partial else reach.shape[2] - 1
