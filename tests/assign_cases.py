"""The shapes, states and given paths that the tests of the spectrum-assignment rules share (tests/test_assign_spectrum.py on the
oracle, tests/test_assign_spectrum_gpu.py on the device): the same function walks either backend — the first AGENT_ENVS envs under
slot_agent's boundary-seeking agents, the others under the heuristic — so the CPU test establishes on the oracle what the states of
the GPU test hold.  Helper module, no tests."""
import functools
from collections import namedtuple

import numpy as np

from tests import assign_restate as ar
from tests import slot_agent

K = 5
ENV_TYPE = {"RMSA": 0, "RWA": 2}
AGENT_ENVS = 24
AGENT_STEPS = 60
HEURISTIC = {"RMSA": "SAP_FF", "RWA": "SAP_FF"}
Shape = namedtuple("Shape", "name fam topology S envs kw")


def _rmsa(S, envs, load, topology="nsfnet_chen", **kw):
    kw = dict(dict(load=load, num_spectrum_resources=S, allow_rejection=True, mean_service_holding_time=10.0, episode_length=50), **kw)
    return Shape("rmsa_%s_s%d" % (topology[:3], S), "RMSA", topology, S, envs, kw)


def _rwa(S, envs, load):
    return Shape("rwa_nsf_s%d" % S, "RWA", "nsfnet_chen", S, envs,
                 dict(load=load, num_spectrum_resources=S, allow_rejection=True, mean_service_holding_time=10.0, episode_length=40))


# the smallest shapes at which the kernel can go wrong (the loads: slot_agent's for the same S)
SHAPES = [_rmsa(64, 512, 60),    # W = 1, s = S - n on the last bit of the word
          _rmsa(65, 512, 60),    # W = 2, one slot in the second word
          _rmsa(129, 20, 130),   # W = 5, the third group of 8 is half empty
          _rmsa(321, 24, 330),   # W = 8
          _rmsa(512, 24, 150, bit_rate_selection="discrete", bit_rates=(40, 100, 400)),  # services of up to 33 slots
          _rwa(65, 24, 400), _rwa(129, 24, 150), _rwa(512, 24, 150),
          _rmsa(128, 24, 130, topology="germany50")]  # 88 links: the link loop of rules 4 and 5 passes 64
SHAPE_BY_NAME = {s.name: s for s in SHAPES}
CPU_SHAPES = ("rmsa_nsf_s65", "rmsa_nsf_s129", "rwa_nsf_s129")  # the ones walked on the oracle too


def seeds_of(shape):
    return [700 + 11 * i + shape.S for i in range(shape.envs)]


@functools.lru_cache(maxsize=None)
def topology(name):
    from optical_rl_gym_amd.topology import Topology

    topo = Topology.load(name)
    assert topo.k_paths == K
    return topo


def state_of(env, shape):
    topo = topology(shape.topology)
    return ar.unpack_slots(env.slots_packed(), topo.n_links, shape.S, ar.row_words(shape.S)), env.services().copy()


def agent_steps(env, shape, n_steps, rng, t0=0):
    """n_steps on the backend's read-back state: slot_agent's agent of the family on the first AGENT_ENVS envs (a Python loop per
    env), the heuristic's action on the others of a larger batch."""
    topo = topology(shape.topology)
    n = min(shape.envs, AGENT_ENVS)
    for t in range(t0, t0 + n_steps):
        avail, services = state_of(env, shape)
        acts = np.array(env.policy(HEURISTIC[shape.fam]), np.int32).copy()
        if shape.fam == "RWA":
            acts[:n] = slot_agent.rwa_agent_actions(avail[:n], services[:n], topo, t, rng, shape.S)[0]
        else:
            acts[:n] = slot_agent.agent_actions(avail[:n], services[:n], topo, t, rng, shape.S)
        env.step(acts, auto_reset=True)


def need_on_path0(shape, services, topo):
    if shape.fam == "RWA":
        return np.ones(len(services), np.int64)
    return slot_agent.slots_needed(services, topo)[:, 0]


def crowd(shape, avail, services):
    """Slot maps no walk at these loads makes: `avail` (bool [n, links, S]) with further slots taken, by env index mod 4 — 0: every
    slot of every row taken with a probability that grows with the index; 1: the first link of path 0 full (path 0 has no room,
    later paths may) and random occupancy elsewhere; 2: only the top n slots free everywhere, n = the slots on path 0 (a choice
    lands on S - n; where path 0 needs the most slots, nothing else fits); 3: a comb on every link — free runs of n + 1, n - 1, n,
    n + 1, n, ... slots (n: path 0's; a run of 0 slots is left out) between single taken slots: best fit has a tie, exact fit
    passes the first run."""
    topo = topology(shape.topology)
    out = avail.copy()
    n_env, _, S = avail.shape
    rng = np.random.default_rng(S + n_env)
    need = need_on_path0(shape, services, topo)
    for i in range(n_env):
        src, dst = int(services[i, 2]), int(services[i, 3])
        kind, n = i % 4, int(need[i])
        if kind == 0:
            out[i] &= rng.random(out[i].shape) >= 0.04 * (1 + (i // 4) % 12)
        elif kind == 1:
            out[i] &= rng.random(out[i].shape) >= 0.1
            out[i, int(topo.path_links[src, dst, 0, 0]), :] = False
        elif kind == 2:
            out[i, :, :max(S - n, 0)] = False
        else:
            comb, s, j = np.zeros(S, bool), (i // 4) % 3, 0
            while s < S:
                L = (n + 1, n - 1, n)[j % 3]
                comb[s:s + L] = True
                s += L + 1
                j += 1
            out[i] &= comb[None, :]
    return out


def draw_paths(services, topo, rng):
    """A given path per env, by env index mod 6: 0 - 2 a path in range, 3 p = n_paths[src, dst] (k where the pair has all k), 4 a
    negative one, 5 p = k + 1"""
    n_paths = topo.n_paths[services[:, 2].astype(np.int64), services[:, 3].astype(np.int64)]
    out = np.zeros(len(services), np.int32)
    for i in range(len(services)):
        kind = i % 6
        out[i] = rng.integers(int(n_paths[i])) if kind <= 2 else int(n_paths[i]) if kind == 3 else -1 - int(rng.integers(3)) if kind == 4 else K + 1
    return out


def set_maps(env, snap, avail):
    """The snapshot `snap` of a device batch with the slot maps `avail` (bool [n, links, S]) in place of its own, restored into it."""
    n, E, S = avail.shape
    lay = env.state_layout()
    words = env.lib.orl_batch_map_words(env._h)
    W = env.lib.orl_batch_row_words(env._h)
    assert lay[2] == 8 * words and words >= E * W
    bits = np.zeros((n, E, 64 * W), np.uint8)
    bits[:, :, :S] = avail
    packed = np.packbits(bits, axis=2, bitorder="little").view("<u8").reshape(n, E * W)
    buf = snap.copy()
    off = n * (lay[0] + lay[1])
    maps = buf[off:off + n * lay[2]].view(np.uint64).reshape(n, words)
    maps[:, :E * W] = packed
    env.set_state(buf)


def expected(shape, avail, services, rng, seen):
    """[(rule, n_given, given, want)] for the six rules and both n_given on one state, the kinds it holds counted into `seen`;
    and the state's Prepared"""
    topo = topology(shape.topology)
    prep = ar.Prepared(ENV_TYPE[shape.fam], avail, services, topo, K, shape.S)
    out = []
    for rule in ar.RULES:
        for g in (0, 1):
            given = draw_paths(services, topo, rng) if g else None
            out.append((rule, g, given, ar.assign(prep, rule, g, given, seen)))
    return out, prep
