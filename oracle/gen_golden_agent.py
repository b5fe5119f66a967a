#!/usr/bin/env python3
"""Agent-made RMCSA and RWA action streams replayed in the reference (tests/slot_agent.py holds the agents and the walks).

Runs only where the reference tree is at hand (ORL_REFERENCE; imported through oracle/refshim, like gen_golden.py):
    python oracle/gen_golden_agent.py
Writes tests/golden/g11_rmcsa_agent_c7_s65.npz, g11_rmcsa_agent_wxt.npz and g11_rwa_agent_s129.npz with gen_golden.run_trace:
the whole walk of one env of the cases rmcsa_c7_s65, rmcsa_c3_s128 (worst_xt = -54.8: services inside lmax_snr and beyond
lmax_xt) and rwa_s129 as ONE stored action stream — the agent's actions of the agent phases and, for the run phases, the
actions the loop's heuristic gives on the oracle's state at every step — replayed in the reference on that env's seed.  The
env is the first whose stream holds every kind of refused action the fixture is there for: env 0, but for the worst_xt case,
where a service beyond lmax_xt alone is rare (13 of the walk's 3 168 agent actions) and env 0 meets none: env 1.  The `g*` name
enrols the fixtures in test_oracle_reproduces_reference_trace and test_hip_reproduces_reference_trace.

The RMCSA streams hold every kind of deliberately refused action of the agent (tests/slot_agent.py, KINDS): beyond a reach
limit, busy in the chosen core, one slot past S, and the partial rejects (path < k with mod == M, core == C or slot == S).
The reference raised on none of them: step() tests all four indices against their upper bounds before it touches the slot
map (rmcsa_env.py:222-227), and its actions_output array has a cell for each (rmcsa_env.py:145-153).  (Its own heuristic
returns a 3-tuple for reject, which step() could not unpack; the stream's full reject is the 4-tuple (k, M, C, S).)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402  (sets up the shim, numpy.int, the reference import)

sys.path.insert(0, gg.REPO)

import gym  # noqa: E402  (the stand-in under oracle/refshim)

from oracle.oracle import OracleBatch  # noqa: E402
from tests import slot_agent  # noqa: E402


def env_with(case, kinds):
    w = slot_agent.walk(case.name)
    for e in range(case.batch):
        if kinds <= {int(s["meta"][e, 0]) for s in w["steps"]}:
            return e
    raise SystemExit("%s: no env meets all of %r" % (case.name, kinds))


def stream_of_env(case, e):
    """The actions of env `e` over the whole walk: the stored agent actions, and the loop's heuristic on a one-env oracle that follows
    the walk (run() is the heuristic's action and an auto-reset step, step after step)."""
    w = slot_agent.walk(case.name)
    ora = OracleBatch(case.fam, slot_agent.TOPOLOGY, slot_agent.seeds_of(case)[e:e + 1], **case.kw)
    steps = iter(w["steps"])
    out, kinds = [], []
    for kind, length in slot_agent.phases_of(case):
        for _ in range(length):
            if kind == "run":
                a, what = ora.policy(slot_agent.LOOP_POLICY[case.fam]).copy(), slot_agent.RUN_STEP
            else:
                rec = next(steps)
                assert np.array_equal(ora.services()[0], rec["services"][e])  # the one-env oracle is where the walk's env was
                a, what = rec["actions"][e:e + 1], int(rec["meta"][e, 0])
            ora.step(a, auto_reset=True)
            out.append(a[0])
            kinds.append(what)
    return np.array(out, np.int64), np.array(kinds, np.int64)


def main():
    for name, case_name, needed in slot_agent.REFERENCE_FIXTURES:
        case = slot_agent.CASE_BY_NAME[case_name]
        e = env_with(case, needed)
        acts, kinds = stream_of_env(case, e)
        kw = dict(case.kw, seed=slot_agent.seeds_of(case)[e])
        if case.fam == "RMCSA":
            env = gym.make("RMCSA-v0", topology=gg.load_topology(slot_agent.TOPOLOGY), **kw)
            extra = dict(info_keys=gg.RMCSA_INFO)
        else:
            acts = acts[:, :2]
            env = gym.make("RWA-v0", topology=gg.load_topology(slot_agent.TOPOLOGY), **kw)
            extra = dict(info_keys=gg.RWA_INFO, vec_info_keys=("path_action_probability", "wavelength_action_probability"))
        gg.run_trace(name, env, actions=acts, n_steps=len(acts), snapshot_every=50,
                     meta=dict(env=case.fam, topology=slot_agent.TOPOLOGY, kwargs=kw, policy="ACTIONS", case=case_name, env_index=e,
                               kinds=[int(k) for k in kinds]), **extra)


if __name__ == "__main__":
    main()
