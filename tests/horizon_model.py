"""An independent source of release times for the release-horizon tests (include/orl.h, orl_batch_release_horizons): the oracle exposes
no event list, so this model keeps one per env beside whichever backend is stepped — the oracle in tests/test_release_horizons.py, a
device batch in tests/test_release_horizons_gpu.py — from what goes in and comes out of step() alone.  Test infrastructure only.

Per env a list of (release time, src, dst, path, core, first slot, slots).  A record is appended when a stepped action is accepted:
the action and services() are read before the step, the reward after it; release time = arrival + holding time in float64
(optical_network_env.py, _add_release).  After every step the records with time <= the new services()[:, 0] leave (the release loop of
optical_network_env.py:143-154).  An episode's end keeps the network state and with it the records; reset(full=True) drops them.

Also the walks both tests take: the family's heuristic for a warm-up, then slot_agent's boundary-seeking agents, which are refused
on purpose now and then."""
import numpy as np

from tests import assign_cases as ac
from tests import rmcsa_mask_restate as rr
from tests import slot_agent

HEURISTIC = {"RMSA": "SAP_FF", "RWA": "SAP_FF", "RMCSA": "SAP_BM_FC_FF"}
# name -> warm-up steps under the heuristic, agent steps and, where the shape's own does not bring the kinds about, the load.  The other
# keywords are those of tests/assign_cases.py and tests/slot_agent.py.  Loads chosen on the oracle (tests/test_release_horizons.py counts
# the kinds): rmsa_nsf_s129 at 220 Erlang holds 150 - 190 releases per env; rwa_nsf_s129 at 1 500 Erlang fills whole rows (about 800
# releases per env); rmcsa_c2_s129 at 1 200 Erlang fills rows of a core.
N_ENVS = 24


def _case(name):
    if name in ac.SHAPE_BY_NAME:
        s = ac.SHAPE_BY_NAME[name]
        return s.fam, dict(s.kw), s.S
    c = slot_agent.CASE_BY_NAME[name]
    return c.fam, dict(c.kw), c.S


WALKS = {"rmsa_nsf_s65": dict(warm=150, agent=40), "rmsa_nsf_s129": dict(warm=700, agent=30, load=220), "rwa_nsf_s129": dict(warm=1100, agent=40, load=1500),
         "rmcsa_c7_s64": dict(warm=200, agent=30), "rmcsa_c2_s129": dict(warm=900, agent=30, load=1200)}
SEED0 = 4100  # env e of every walk is seeded SEED0 + e


def walk_config(name):
    """(family, keywords, S, envs, seeds) of a named walk"""
    fam, kw, S = _case(name)
    if "load" in WALKS[name]:
        kw["load"] = WALKS[name]["load"]
    return fam, kw, S, N_ENVS, [SEED0 + e for e in range(N_ENVS)]


class Model:
    def __init__(self, fam, topo, n_envs, tables=None):
        self.fam, self.topo, self.n, self.tab = fam, topo, n_envs, tables
        self.ev = [[] for _ in range(n_envs)]
        self.released = [0] * n_envs   # records that have left, per env
        self.out_of_order = [False] * n_envs  # a record left while one appended before it stayed
        self._pre = None

    def before(self, services, actions):
        self._pre = (np.array(services, np.float64), np.array(actions, np.int64))

    def _record(self, e, sv, a):
        src, dst = int(sv[2]), int(sv[3])
        t = sv[0] + sv[1]
        if self.fam == "RWA":
            return (t, src, dst, int(a[0]), 0, int(a[1]), 0)
        if self.fam == "RMCSA":
            n = int(self.tab["n_slots"][self.tab["rate_index"][int(sv[4])]][int(a[1])])
            return (t, src, dst, int(a[0]), int(a[2]), int(a[3]), n)
        n = int(slot_agent.slots_needed(sv[None, :], self.topo)[0, int(a[0])])
        return (t, src, dst, int(a[0]), 0, int(a[1]), n)

    def after(self, reward, services):
        sv0, acts = self._pre
        for e in range(self.n):
            if reward[e] > 0:
                self.ev[e].append(self._record(e, sv0[e], acts[e]))
            now = float(services[e, 0])
            keep = [r for r in self.ev[e] if not r[0] <= now]
            if len(keep) != len(self.ev[e]):
                self.released[e] += len(self.ev[e]) - len(keep)
                gone = [i for i, r in enumerate(self.ev[e]) if r[0] <= now]
                self.out_of_order[e] |= any(not self.ev[e][i][0] <= now for i in range(gone[-1]))
            self.ev[e] = keep

    def reset_full(self):
        self.ev = [[] for _ in range(self.n)]

    def copy_env(self, dst, src):
        self.ev[dst] = list(self.ev[src])

    def times(self, e):
        return np.array([r[0] for r in self.ev[e]], np.float64)

    def records(self, e):
        """int64 [m, 5] in the column order of BatchedOpticalEnv.pending(): (src * N + dst, path, first slot, slots, core)"""
        N = self.topo.n_nodes
        return np.array([(r[1] * N + r[2], r[3], r[5], r[6], r[4]) for r in self.ev[e]], np.int64).reshape(-1, 5)

    def busy(self, e, C, S):
        """int64 [C, links, S]: how many records hold each slot (the pending_is_the_slot_map idiom of tests/test_op_walk_gpu.py)"""
        topo = self.topo
        out = np.zeros((C, topo.n_links, S), np.int64)
        for _, src, dst, p, c, lo, n in self.ev[e]:
            n = max(n, 1)
            assert p < int(topo.n_paths[src, dst]) and lo + n <= S and c < C, (e, src, dst, p, c, lo, n)
            out[c, topo.path_links[src, dst, p, :int(topo.path_hops[src, dst, p])], lo:lo + n] += 1
        return out


def avail_of(env, C, S):
    """bool [n, C, links, S] of a backend's packed slot maps"""
    return rr.unpack_cores(env.slots_packed(), C, env.topology.n_links, S)


def agent_actions(fam, avail, services, topo, tab, t, rng, S, C):
    if fam == "RMCSA":
        return slot_agent.rmcsa_agent_actions(avail, services, topo, tab, t, rng, S, C)[0]
    if fam == "RWA":
        return slot_agent.rwa_agent_actions(avail[:, 0], services, topo, t, rng, S)[0]
    return slot_agent.agent_actions(avail[:, 0], services, topo, t, rng, S)


def step(env, model, actions):
    """One step of the backend with the model beside it; returns the reward"""
    model.before(env.services(), actions)
    _, rew, _, _ = env.step(np.ascontiguousarray(actions, np.int32), auto_reset=True)
    model.after(np.asarray(rew), env.services())
    return np.asarray(rew)


def walk(name, env, model, checkpoint):
    """The named walk on `env` (the oracle or a device batch of walk_config(name)) with `model` beside it; checkpoint(tag) is called after
    the warm-up's tenth step, half and end and after every tenth agent step and the last.  Returns (accepted, refused) over the agent steps."""
    fam, kw, S, n, _ = walk_config(name)
    C = kw.get("num_spatial_resources", 1)
    topo, tab = env.topology, model.tab
    w = WALKS[name]
    for t in range(w["warm"]):
        step(env, model, np.array(env.policy(HEURISTIC[fam]), np.int32))
        if t + 1 in (10, w["warm"] // 2, w["warm"]):  # (10: maps still mostly free — rows without a busy slot, blocks at slot 0)
            checkpoint("warm %d" % (t + 1))
    rng = np.random.RandomState(S + C)
    acc = ref = 0
    for t in range(w["agent"]):
        acts = agent_actions(fam, avail_of(env, C, S), env.services(), topo, tab, t, rng, S, C)
        rew = step(env, model, acts)
        acc += int((rew > 0).sum())
        ref += int((rew <= 0).sum())
        if (t + 1) % 10 == 0 or t + 1 == w["agent"]:
            checkpoint("agent %d" % (t + 1))
    return acc, ref
