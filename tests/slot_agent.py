"""Agent-made slot maps at the 64-slot edges: a deterministic boundary-seeking agent for RMSA, the table of cases and the oracle's
walk of each — shared by tests/test_agent_maps.py (CPU: the walk meets the conditions it exists for) and
tests/test_agent_maps_gpu.py (the device replays it under every step implementation).  Helper module, no tests.

Why: RMSA's first fit searches range(0, S - n) and never takes the last slot, while step() accepts initial_slot + n == S from an
agent; and the device-resident loop only ever runs a heuristic.  So the top bit of a row's last word, a release that ends at S
and slot maps no first fit would make are reached only through an agent's actions, and the loop meets them only when it is handed
such a map.  The walk: 120 agent steps, run("SAP_FF", 100), 40 agent steps.

The agent works on the ORACLE's state (slot maps, pending services) and the topology tables: for env e at step t it lists every
(path, start) whose n = ceil(bit_rate / (se * 12.5)) + 1 slots are free on all links of the path and end at or below S, keeps
those that meet the goal (t + e) % 4 — 0: end on a multiple of 64 or on S; 1: start on a multiple of 64; 2: straddle a word
boundary; 3: any — or all of them when none does, and draws one with a seeded RandomState; no candidate: the reject action.

RMCSA and RWA have agents of their own (rmcsa_agent_actions, rwa_agent_actions) for what their heuristics never do either: SAP_BM_FC_FF
takes the lowest free core and the path's best modulation and never the last slot, so a core above 0 that is fuller than core 0, a
width that comes from another modulation, the top bit of a last word in a high core, and actions that are refused or reject in part
(core == C or mod == M under a valid path) come from an agent alone; RWA batches otherwise run at row widths of 1 and 2 words.  Their
walks (RMCSA_PHASES, RWA_PHASES) hand the maps to the loop more than once — RMCSA: three launches of one step first."""
import functools
from collections import namedtuple

import numpy as np

from tests import row_ref
from tests.mask_restate import restate_fast, row_words, unpack_slots

TOPOLOGY, K = "nsfnet_chen", 5
PHASES = (("agent", 120), ("run", 100), ("agent", 40))
# RMCSA: three launches of one step each on the prev_core values the agent left, then a longer run; RWA: SAP_LF, so that the loop
# itself works the row's top word
RMCSA_PHASES = (("agent", 90), ("run", 1), ("run", 1), ("run", 1), ("agent", 12), ("run", 60), ("agent", 30))
RWA_PHASES = (("agent", 90), ("run", 60), ("agent", 30))
LOOP_POLICY = {"RMSA": "SAP_FF", "DeepRMSA": "SAP", "RMCSA": "SAP_BM_FC_FF", "RWA": "SAP_LF"}
SAMPLED_POLICIES = {"RMSA": ("SAP_FF", "LLP_FF"), "DeepRMSA": ("SAP",), "RMCSA": ("SAP_BM_FC_FF",), "RWA": ("SAP_FF", "SAP_LF", "LLP_FF")}
Case = namedtuple("Case", "name fam S load kw batch dev_kw acc", defaults=({}, None))


def phases_of(case):
    return {"RMCSA": RMCSA_PHASES, "RWA": RWA_PHASES}.get(case.fam, PHASES)


def cores_of(case):
    return case.kw.get("num_spatial_resources", 1)


def _rmsa(S, load):
    return Case("rmsa_s%d" % S, "RMSA", S, load,
                dict(load=load, num_spectrum_resources=S, allow_rejection=True, mean_service_holding_time=10.0, episode_length=50), 64)


CASES = [_rmsa(65, 60), _rmsa(128, 130), _rmsa(129, 130), _rmsa(257, 260), _rmsa(321, 330), _rmsa(449, 450), _rmsa(512, 500),
         # uniformly random integer actions (reject included): blocks of index >= 2 only exist in fragmented maps
         Case("deep_s129_j4", "DeepRMSA", 129, 130,
              dict(mean_service_holding_time=10.0, mean_service_inter_arrival_time=10.0 / 130, j=4, num_spectrum_resources=129,
                   allow_rejection=True, episode_length=50), 64)]


def _rmcsa(C, S, load, acc, name=None, batch=24, worst_xt=-84.7, dev_kw=None, **kw):
    """acc: the acceptance over the agent steps observed on the oracle at this load (tests/test_agent_maps.py prints it)"""
    kw = dict(kw, load=load, num_spectrum_resources=S, num_spatial_resources=C, worst_xt=worst_xt, allow_rejection=True,
              mean_service_holding_time=10.0, episode_length=40)
    return Case(name or "rmcsa_c%d_s%d" % (C, S), "RMCSA", S, load, kw, batch, dev_kw or {}, acc)


def _rwa(S, load, acc):
    return Case("rwa_s%d" % S, "RWA", S, load, dict(load=load, num_spectrum_resources=S, allow_rejection=True, mean_service_holding_time=10.0,
                                                    episode_length=40), 24, {}, acc)


WXT_CASE, RATES_CASE, HIST_CASE = "rmcsa_c3_s128", "rmcsa_c2_s512", "rmcsa_c7_s65"
HIST_ENVS = (0, 11, 23)
WIDE = 33  # slots of a 400 Gb/s service on BPSK: ceil(400 / 12.5) + 1
CASES += [
    # RMCSA (C, S): load per case chosen on the oracle for the conditions of tests/test_agent_maps.py.  The maps never fill in 195 steps:
    # what bounds the acceptance are the reach limits (no candidate at all for about a quarter of the services) and goal 5
    _rmcsa(7, 64, 150, 0.5616), _rmcsa(7, 65, 150, 0.5777, dev_kw=dict(action_histograms=True)),
    # worst_xt = -54.8: QPSK at low bit rates reaches further by SNR (6 116 km at 25 Gb/s) than by crosstalk (2 399 km)
    _rmcsa(3, 128, 150, 0.4574, worst_xt=-54.8),
    _rmcsa(2, 129, 150, 0.5625, batch=20),     # 20 envs: the third group of 8 is half empty
    _rmcsa(17, 65, 150, 0.5638),               # 4 * 17 = 68 sums: past the 16-word line of cs_words
    _rmcsa(31, 64, 150, 0.5694),               # the 5-bit core field full, the reject index at 31
    # 400 Gb/s on BPSK: 33 slots, inside lmax_snr (191 km) on the 150 km paths only
    _rmcsa(2, 512, 150, 0.3971, bit_rate_selection="discrete", bit_rates=(40, 100, 400)),
    # RWA: the agent never runs out of free pairs at these loads; what it is refused are the busy pairs of goal 2
    _rwa(65, 400, 0.7524), _rwa(129, 150, 0.7524), _rwa(320, 150, 0.7524), _rwa(512, 150, 0.7524)]
CASE_BY_NAME = {c.name: c for c in CASES}
# (fixture, case, the kinds of refused action its stream must hold): one env's whole walk replayed in the reference
# (oracle/gen_golden_agent.py); "beyond lmax_xt only" is kind 1, a busy RWA pair kind 0
REFERENCE_FIXTURES = (("g11_rmcsa_agent_c7_s65", "rmcsa_c7_s65", frozenset((0, 2, 3, 4, 5, 6, 7))), ("g11_rmcsa_agent_wxt", WXT_CASE, frozenset((1,))),
                      ("g11_rwa_agent_s129", "rwa_s129", frozenset((0,))))
# the two-wavefront form needs a specialisation library per configuration (RMCSA: the one-wavefront kernel, specialised)
PAIR_CASES = ("rmsa_s129", "rmsa_s321", "rmcsa_c7_s65", "rmcsa_c17_s65", "rwa_s129")


def spec_flags_of(case):
    """The flags of the case's specialisation library under the implementation the environment asks for (no device needed)."""
    from optical_rl_gym_amd import envs

    return envs.ENV_CLASSES[case.fam].spec_flags(batch=case.batch, topology=TOPOLOGY, **dict(case.kw, **case.dev_kw))


def seeds_of(case):
    return [500 + 7 * i + case.S + 1000 * (cores_of(case) - 1) for i in range(case.batch)]


@functools.lru_cache(maxsize=None)
def topology():
    from optical_rl_gym_amd.topology import Topology

    return Topology.load(TOPOLOGY)


def slots_needed(services, topo):
    """[n, K]: get_number_slots of the pending service on each of its paths (rmsa_env.py:610-621)"""
    src, dst, br = services[:, 2].astype(np.int64), services[:, 3].astype(np.int64), services[:, 4]
    se = np.array([m.spectral_efficiency for m in topo.modulations], np.float64)
    return np.stack([np.ceil(br / (se[topo.path_best_mod[src, dst, p]] * 12.5)).astype(np.int64) + 1 for p in range(K)], axis=1)


def agent_actions(avail, services, topo, t, rng, S):
    """The boundary-seeking agent's RMSA actions [n, 4] (path, first slot) for slot maps avail (bool [n, links, S])."""
    n_env = len(services)
    fits = restate_fast(0, avail, services, topo, K, S, allow_rejection=True, layout="joint", fallback=False)[:, :-1]
    need = slots_needed(services, topo)
    acts = np.zeros((n_env, 4), np.int32)
    for e in range(n_env):
        cand = np.flatnonzero(fits[e])
        if len(cand) == 0:
            acts[e, :2] = (K, S)
            continue
        path, start = cand // S, cand % S
        end = start + need[e, path]
        goal = (t + e) % 4
        if goal == 0:
            ok = (end % 64 == 0) | (end == S)
        elif goal == 1:
            ok = start % 64 == 0
        elif goal == 2:
            ok = start // 64 != (end - 1) // 64
        else:
            ok = np.ones(len(cand), bool)
        pool = np.flatnonzero(ok) if ok.any() else np.arange(len(cand))
        c = pool[rng.randint(len(pool))]
        acts[e, :2] = (path[c], start[c])
    return acts


# ---- RMCSA: (path, modulation, core, first slot) ------------------------------------------------------------------------------
KINDS = ("beyond lmax_snr", "beyond lmax_xt only", "busy in this core, free in another", "start + n == S + 1", "core == C", "mod == M",
         "slot == S", "full reject")
PROVISION, NO_CANDIDATE = -1, len(KINDS)  # what an action was meant as, next to the kinds of deliberately refused ones
RUN_STEP = -2                             # (in a fixture's stream: the heuristic's action of a run phase)


@functools.lru_cache(maxsize=None)
def rmcsa_tables(name):
    """The tables the batch hands to the ABI for the case (envs.py: n_slots [rate][mod], lmax_snr [mod][rate], lmax_xt [mod], the bit
    rates of the rows) — made without a device."""
    from optical_rl_gym_amd import envs

    keep = envs.ENV_CLASSES["RMCSA"]._derived(topology=TOPOLOGY, **CASE_BY_NAME[name].kw)._keep
    return dict(n_slots=keep["n_slots"].astype(np.int64), lmax_snr=keep["lmax_snr"], lmax_xt=keep["lmax_xt"],
                rate_index={int(r): i for i, r in enumerate(keep["bit_rates"])}, path_length=keep["path_length"], path_best_mod=keep["path_mod"])


def _draw(rng, mask):
    idx = np.flatnonzero(mask.ravel())
    return np.unravel_index(idx[rng.randint(len(idx))], mask.shape)


def rmcsa_agent_actions(avail, services, topo, tab, t, rng, S, C):
    """The RMCSA agent's actions [n, 4] for slot maps avail (bool [n, C, links, S]) and what each was meant as: meta [n, 4] =
    (PROVISION / kind of refused action / NO_CANDIDATE, slots of the service under the action's modulation, a lower core had a
    candidate too, the modulation is not the path's best)."""
    n_env, M = len(services), len(tab["lmax_xt"])
    acts, meta = np.zeros((n_env, 4), np.int32), np.zeros((n_env, 4), np.int64)
    s_idx = np.arange(S)
    for e in range(n_env):
        src, dst = int(services[e, 2]), int(services[e, 3])
        br = tab["rate_index"][int(services[e, 4])]
        n_of = tab["n_slots"][br]                                        # [M]
        free = np.zeros((C, K, S), bool)                                 # the path's links all free, per core
        length = np.full(K, np.inf)
        for p in range(int(topo.n_paths[src, dst])):
            links = topo.path_links[src, dst, p, :int(topo.path_hops[src, dst, p])]
            free[:, p] = avail[e][:, links, :].all(axis=1)
            length[p] = tab["path_length"][src, dst, p]
        has = np.isfinite(length)
        cum = np.concatenate([np.zeros((C, K, 1), np.int64), np.cumsum(free, axis=2)], axis=2)
        end = s_idx[None, :] + n_of[:, None]                             # [M, S]
        inside = end <= S
        run = cum[:, :, np.minimum(end, S)] - cum[:, :, None, :S]        # [C, K, M, S] free slots of [s, s + n)
        fits = (run == n_of[None, None, :, None]) & inside[None, None] & has[None, :, None, None]
        snr = (length[:, None] < tab["lmax_snr"][:, br][None, :])        # [K, M]
        xt = (length[:, None] < tab["lmax_xt"][None, :])
        cand = fits & (snr & xt)[None, :, :, None]
        best = tab["path_best_mod"][src, dst]                            # [K]
        if not cand.any():
            acts[e], meta[e, 0] = (K, M, C, S), NO_CANDIDATE
            continue
        goal = (t + e) % 6
        if goal == 5:
            some = np.unravel_index(np.flatnonzero(cand.ravel())[rng.randint(int(cand.sum()))], cand.shape)  # (c, p, m, s)
            first = (t // 6) % len(KINDS)
            for kind in [(first + i) % len(KINDS) for i in range(len(KINDS))]:
                pool = None
                if kind == 0:
                    pool = fits & ~snr[None, :, :, None]
                elif kind == 1:
                    pool = fits & (snr & ~xt)[None, :, :, None]
                elif kind == 2:
                    reach = (snr & xt & has[:, None])[None, :, :, None]
                    pool = ~fits & inside[None, None] & reach & cand.any(axis=0)[None]
                elif kind == 3:  # one slot too far up; the slots below S themselves free where that exists
                    at = S + 1 - n_of                                    # [M]
                    pool = np.zeros_like(fits)
                    tail = (cum[:, :, S][:, :, None] - cum[:, :, np.clip(at, 0, S)]) == (n_of - 1)[None, None, :]  # [C, K, M]
                    tail &= (snr & xt & has[:, None])[None] & ((at >= 0) & (at < S))[None, None, :]
                    if not tail.any():
                        tail = np.broadcast_to((has[:, None] & ((at >= 0) & (at < S))[None, :])[None], tail.shape)
                    for m in range(M):
                        if 0 <= at[m] < S:
                            pool[:, :, m, at[m]] = tail[:, :, m]
                if pool is not None:
                    if not pool.any():
                        continue
                    c, p, m, s0 = _draw(rng, pool)
                else:
                    c, p, m, s0 = some
                    if kind == 4:
                        c = C
                    elif kind == 5:
                        m = M
                    elif kind == 6:
                        s0 = S
                    else:
                        p, m, c, s0 = K, M, C, S
                acts[e] = (p, m, c, s0)
                meta[e] = (kind, n_of[m] if m < M else 0, 0, 0)
                break
            continue
        c_i, p_i, m_i, s_i = np.nonzero(cand)
        e_i = s_i + n_of[m_i]
        if goal == 0:
            ok = (e_i % 64 == 0) | (e_i == S)
        elif goal == 1:
            ok = s_i % 64 == 0
        elif goal == 2:
            ok = s_i // 64 != (e_i - 1) // 64
        elif goal == 3:  # the highest core that has a candidate: C - 1 as long as it has room, whatever the cores below hold
            ok = c_i == c_i.max()
        else:
            ok = m_i != best[p_i]
        pool = np.flatnonzero(ok) if ok.any() else np.arange(len(c_i))
        i = pool[rng.randint(len(pool))]
        acts[e] = (p_i[i], m_i[i], c_i[i], s_i[i])
        meta[e] = (PROVISION, n_of[m_i[i]], int((c_i < c_i[i]).any()), int(m_i[i] != best[p_i[i]]))
    return acts, meta


# ---- RWA: (path, wavelength) ------------------------------------------------------------------------------------------------
BUSY_PAIR = 0  # meta of an RWA action meant to be refused: a pair with a wavelength in use on the path


def rwa_agent_actions(avail, services, topo, t, rng, S):
    """The RWA agent's actions [n, 4] (path, wavelength) for slot maps avail (bool [n, links, S]); meta [n, 4] as the RMCSA agent's."""
    n_env = len(services)
    free = restate_fast(2, avail, services, topo, K, S, allow_rejection=True, layout="joint", fallback=False)[:, :-1]
    acts, meta = np.zeros((n_env, 4), np.int32), np.zeros((n_env, 4), np.int64)
    for e in range(n_env):
        cand = np.flatnonzero(free[e])
        if len(cand) == 0:
            acts[e, :2], meta[e, 0] = (K, S), NO_CANDIDATE
            continue
        goal = (t + e) % 4
        if goal == 2:
            n_paths = int(topo.n_paths[int(services[e, 2]), int(services[e, 3])])
            busy = np.flatnonzero(~free[e, :n_paths * S])
            if len(busy):
                c = busy[rng.randint(len(busy))]
                acts[e, :2], meta[e, 0] = (c // S, c % S), BUSY_PAIR
                continue
        w = cand % S
        if goal == 0:
            ok = (w % 64 == 63) | (w == S - 1)
        elif goal == 1:
            ok = (w % 64 == 0) & (w > 0)
        else:
            ok = np.ones(len(cand), bool)
        pool = np.flatnonzero(ok) if ok.any() else np.arange(len(cand))
        c = cand[pool[rng.randint(len(pool))]]
        acts[e, :2], meta[e] = (c // S, c % S), (PROVISION, 1, 0, 0)
    return acts, meta


def _state(ora):
    return dict(counters=ora.counters().copy(), services=ora.services().copy(), active=ora.active().copy(), slots_packed=ora.slots_packed().copy(),
                link_stats_all=ora.link_stats_all().copy(), net_stats_all=ora.net_stats_all().copy())


def expected_masks(case, avail, services, topo):
    if case.fam == "RMCSA":  # (no action masks)
        return {}
    env_type = {"RMSA": 0, "DeepRMSA": 1, "RWA": 2}[case.fam]
    layouts = ("joint",) if case.fam == "DeepRMSA" else ("joint", "path")
    return {layout: restate_fast(env_type, avail, services, topo, K, case.S, j=case.kw.get("j", 1), allow_rejection=True, layout=layout)
            for layout in layouts}


def _walk(case, agent=True):
    """The oracle's walk of a case.  agent=False: the control, every agent step replaced by the loop's heuristic.  `runs`: per run
    phase the slot maps (bool [n, C * links, S], core-major) before and after it, the actions of the step before it with what
    was accepted, and the envs in which a slot that an agent-placed service held when the run began is free after it;
    before_run / after_run: the maps of the last one."""
    from oracle.oracle import OracleBatch

    topo = topology()
    S, E, C = case.S, topo.n_links, cores_of(case)
    ora = OracleBatch(case.fam, TOPOLOGY, seeds_of(case), **case.kw)
    rng = np.random.RandomState(case.S)
    policy = LOOP_POLICY[case.fam]
    tab = rmcsa_tables(case.name) if case.fam == "RMCSA" else None
    steps, states, samples, runs, t = [], [], [], [], 0
    # slots held by a service an agent step placed.  A step provisions before it releases, so within one step no slot is freed
    # and taken again: exact over agent steps and one-step runs; a longer run may refill a slot, so the mask is dropped after it
    placed = np.zeros((ora.n, C * E, S), bool)
    last_actions = last_accepted = None  # of the step before a run: the agent's, or the heuristic's in a one-step run
    for kind, length in phases_of(case):
        if kind == "run":
            before = unpack_slots(ora.slots_packed(), C * E, S, row_words(S))
            rec = dict(before=before, length=length, last_actions=last_actions, last_accepted=last_accepted)
            if length == 1:  # (policy() does not step the batch)
                last_actions, accepted_before = ora.policy(policy).copy(), ora.counters()[:, 1].copy()
            if agent:
                ora.run(policy, length)
            else:
                for _ in range(length):
                    ora.step(ora.policy(policy), auto_reset=True)
            if length == 1:
                last_accepted = ora.counters()[:, 1] - accepted_before == 1
            after = unpack_slots(ora.slots_packed(), C * E, S, row_words(S))
            rec.update(after=after, agent_released=(placed & after).any(axis=(1, 2)))
            placed = placed & ~after if length == 1 else np.zeros_like(placed)
            runs.append(rec)
        else:
            for _ in range(length):
                services = ora.services().copy()
                avail = unpack_slots(ora.slots_packed(), C * E, S, row_words(S))
                rec = dict(t=t, services=services, meta=None)
                if t % 5 == 0:
                    samples.append(avail.reshape(-1, S))
                if t % 10 == 0 and agent:
                    rec["masks"] = expected_masks(case, avail, services, topo)
                    rec["policies"] = {p: ora.policy(p).copy() for p in SAMPLED_POLICIES[case.fam]}
                if not agent:
                    a = ora.policy(policy).copy()
                elif case.fam == "DeepRMSA":
                    a = np.zeros((ora.n, 4), np.int32)
                    a[:, 0] = rng.randint(0, K * case.kw["j"] + 1, ora.n)
                elif case.fam == "RMCSA":
                    a, rec["meta"] = rmcsa_agent_actions(avail.reshape(ora.n, C, E, S), services, topo, tab, t, rng, S, C)
                elif case.fam == "RWA":
                    a, rec["meta"] = rwa_agent_actions(avail, services, topo, t, rng, S)
                else:
                    a = agent_actions(avail, services, topo, t, rng, S)
                accepted_before = ora.counters()[:, 1].copy()
                obs, reward, done, info = ora.step(a, auto_reset=True)
                rec.update(actions=a, reward=reward.copy(), done=done.copy(), info=info.copy(), obs=None if obs is None else obs.copy(),
                           accepted=ora.counters()[:, 1] - accepted_before == 1)
                steps.append(rec)
                last_actions, last_accepted = a, rec["accepted"]
                after = unpack_slots(ora.slots_packed(), C * E, S, row_words(S))
                placed = (placed | (avail & ~after)) & ~after
                t += 1
        states.append(_state(ora))
    out = dict(case=case, steps=steps, states=states, samples=np.concatenate(samples).astype(np.uint8), runs=runs,
               before_run=runs[-1]["before"], after_run=runs[-1]["after"])
    if agent and case.dev_kw.get("action_histograms"):
        out["histograms"] = {e: tuple(h.copy() for h in ora.action_histograms_of(e)) for e in HIST_ENVS}
    return out


@functools.lru_cache(maxsize=None)
def walk(name):
    return _walk(CASE_BY_NAME[name])


@functools.lru_cache(maxsize=None)
def control_walk(name):
    return _walk(CASE_BY_NAME[name], agent=False)


# ---- what the sampled rows hold -------------------------------------------------------------------------------------------
def row_classes(rows, S):
    """Counts over sampled link rows [R, S] (1 = free) of the classes the cases exist for."""
    bounds = [b for b in range(64, S, 64)]
    lower, upper = rows[:, [b - 1 for b in bounds]], rows[:, bounds]
    return dict(last_slot_used=int((rows[:, S - 1] == 0).sum()),
                used_block_across=int(((lower == 0) & (upper == 0)).any(axis=1).sum()),
                free_run_across=int(((lower == 1) & (upper == 1)).any(axis=1).sum()),
                edge_on_boundary=int((lower != upper).any(axis=1).sum()),
                eight_used_blocks=int((row_ref.summary(rows)["nu"] >= 8).sum()))


def acceptance(w):
    acc = np.array([s["accepted"] for s in w["steps"]])
    return float(acc.mean())
