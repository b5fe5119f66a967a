"""First-fit completion of partial RMCSA actions (include/orl.h, orl_batch_complete_actions) without a GPU: the ABI surface, the
kernel in the code object, and the numpy restatement the GPU tests compare with (tests/complete_restate.py) — pinned to the oracle's
own step on agent-made states, prefix by prefix — with the preconditions of the GPU test established on those states."""
import functools
import os
import re
import shutil
import sys

import numpy as np
import pytest

from optical_rl_gym_amd import _lib
from tests import complete_restate as cr
from tests import rmcsa_mask_restate as rr
from tests import slot_agent
from tests.oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOPOLOGY = slot_agent.TOPOLOGY
K, M = 5, 6
SHAPES = ("rmcsa_c7_s64", "rmcsa_c3_s128", "rmcsa_c2_s129")
STATE_SEEDS = (4242, 77, 905, 31, 1234, 68)  # one walked state per seed and point
POINTS = (30, 90)                            # agent steps before the probe
# At load 150 the maps of SHAPES stay below 12 % utilisation however long the agent walks (the reach limits refuse a quarter of the
# services), and on them no path is ever without room: a completion on s = S - n, the empty prefix choosing a path above 0 (the
# reach limits are monotone in the path's length, so only occupancy moves it) and a reject by occupancy alone do not occur under any
# seed or step count.  One more walk on a map small enough to fill — 2 cores x 16 slots at the same load, the tables of rmcsa_c7_s64
# (they depend on worst_xt and the bit rates, not on C or S) — holds them.
CROWDED = slot_agent.Case("crowded_c2_s16", "RMCSA", 16, 150,
                          dict(slot_agent.CASE_BY_NAME["rmcsa_c7_s64"].kw, num_spectrum_resources=16, num_spatial_resources=2, episode_length=1000), 16)
CROWDED_POINTS = (120, 160)
CROWDED_SEEDS = tuple(range(70, 102))
WALKS = [(name, steps) for name in SHAPES for steps in POINTS] + [(CROWDED.name, steps) for steps in CROWDED_POINTS]


def test_header_and_binding_declare_the_completion():
    h = open(os.path.join(ROOT, "include", "orl.h")).read()
    assert re.search(r"int orl_batch_complete_actions\(orl_batch\* b, int n_given,\s*const int32_t\* given[^;]*,\s*int32_t\* actions_out[^;]*\);", h)
    assert re.search(r"#define ORL_ABI_VERSION 2\b", h) and _lib.ABI_VERSION == 2
    assert len(_lib.EXPORTS["orl_batch_complete_actions"][1]) == 4
    for word in ("m\\*\\(p\\)", "monotone", "s = S - n is tried", "reject action \\(k, M, C, S\\)"):
        assert re.search(word, h), word


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_completion_kernels_exist_for_every_row_width_without_scratch_or_lds():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs

    from optical_rl_gym_amd import _build

    lib = _build.build()
    found = {}
    for k in kernel_regs.kernels(lib):
        m = re.match(r"(?:void )?k_rmcsa_complete<(\d+)>", kernel_regs.demangle(k["name"]))
        if m:
            found[int(m.group(1))] = k
    assert sorted(found) == list(_build.ROW_WIDTHS)
    for w, k in found.items():
        assert int(k["vgpr_spill_count"]) == 0 and int(k["sgpr_spill_count"]) == 0 and int(k["private_segment_fixed_size"]) == 0, (w, k)
        assert int(k["group_segment_fixed_size"]) == 0, (w, k)


def probes_of(C):
    """Every prefix in range and the ones out of range, per number of given columns: [(g, prefix)]"""
    out = [(0, ())]
    out += [(1, (p,)) for p in range(-1, K + 1)]
    out += [(2, (p, m)) for p in range(K) for m in range(M)] + [(2, pair) for pair in ((K, 0), (0, M), (-1, 0), (0, -1))]
    out += [(3, (p, m, c)) for p in range(K) for m in range(M) for c in range(C)] + [(3, (0, 0, C)), (3, (0, 0, -1))]
    return out


def _state(ora, rows):
    return rr.unpack_cores(ora.slots_packed()[rows], ora.C, ora.E, ora.S), ora.services()[rows].copy()


@functools.lru_cache(maxsize=None)
def _probe(name, steps):
    """One oracle state per seed after `steps` steps of slot_agent's RMCSA agent, each held by one env per probe (the oracle has
    no snapshot: the envs of a seed take identical actions until the probe), then every probe's restated completion stepped."""
    case = CROWDED if name == CROWDED.name else slot_agent.CASE_BY_NAME[name]
    topo, tab = slot_agent.topology(), slot_agent.rmcsa_tables("rmcsa_c7_s64" if case is CROWDED else name)
    C, S = slot_agent.cores_of(case), case.S
    probes = probes_of(C)
    seeds = CROWDED_SEEDS if case is CROWDED else STATE_SEEDS
    R, G = len(probes), len(seeds)
    lead = np.arange(G) * R
    ora = OracleBackend("RMCSA", TOPOLOGY, list(np.repeat(seeds, R)), **case.kw)
    rng = np.random.RandomState(steps + S)
    for t in range(steps):
        avail, services = _state(ora, lead)
        acts, _ = slot_agent.rmcsa_agent_actions(avail, services, topo, tab, t, rng, S, C)
        ora.step(np.repeat(acts, R, axis=0), auto_reset=True)
    avail, services = _state(ora, lead)
    assert (ora.services() == np.repeat(services, R, axis=0)).all()
    pv = rr.prov_all(avail, services, topo, tab)
    pv_free = rr.prov_all(avail, services, topo, cr.free_tables(tab))
    reject = np.array([K, M, C, S])
    seen = cr.Seen()
    actions = np.zeros((G * R, 4), np.int32)
    for j, (g, pre) in enumerate(probes):
        given = np.tile(np.array(pre, np.int32).reshape(1, g), (G, 1))
        done = cr.complete(pv, services, topo, tab, g, given)
        actions[lead + j] = done
        rej = (done == reject).all(axis=1)
        # the reject action exactly when no action under the prefix provisions: m*(p) loses nothing (g = 0, 1)
        assert np.array_equal(rej, ~cr.prov_under(pv, g, given)), (g, pre)
        assert (done[~rej, :g] == given[~rej]).all()
        if g == 2:  # the lowest set column of the pair's core-slot row
            cs = rr.restate_rmcsa_fast(None, None, topo, tab, "core_slot", given=given, allow_rejection=True, fallback=False, pv=pv)[:, :-1]
            assert np.array_equal(~rej, cs.any(axis=1))
            col = cs.argmax(axis=1)
            assert np.array_equal(done[~rej, 2] * S + done[~rej, 3], col[~rej]) and (done[~rej, :2] == given[~rej]).all()
        seen.count(pv, pv_free, services, topo, tab, g, given, done)
    before = ora.counters()[:, 1].copy()
    ora.step(actions, auto_reset=False)
    accepted = ora.counters()[:, 1] - before
    # the oracle accepts the service exactly when the completion is not the reject action
    assert np.array_equal(accepted == 1, ~(actions == reject).all(axis=1)) and set(np.unique(accepted)) <= {0, 1}
    return seen


@pytest.mark.parametrize("name,steps", WALKS)
def test_restated_completion_is_what_the_oracle_accepts(name, steps):
    seen = _probe(name, steps)
    print(name, steps, vars(seen))


def test_the_walks_meet_every_kind_the_gpu_test_counts():
    """A completion on s = S - n, one in a core above 0, g = 0 choosing a path above 0, a reject by reach alone, a reject by
    occupancy alone, m*(p) other than the path's best-modulation byte: each at least once on the states above."""
    assert [w for w in WALKS if w[0] in SHAPES] == [(name, steps) for name in SHAPES for steps in POINTS]
    total = cr.Seen()
    for name, steps in WALKS:
        total.add(_probe(name, steps))
    print(vars(total))
    assert total.all_positive(), vars(total)
