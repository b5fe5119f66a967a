"""Core and spectrum rules with a (path, core) table for RMCSA actions (include/orl.h, orl_batch_route_cores) without a GPU: the ABI
surface, the kernel's instantiations in the code object, the facades, the launch plan, and the restatement the GPU tests compare with
(tests/route_cores_restate.py) — pinned to a brute-force one-loop key search, to the restatement of orl_batch_complete_actions and to
the oracle's own step — with the kinds the GPU test needs established on walked, crowded and crafted states
(tests/route_cores_cases.py)."""
import ctypes
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
from tests import route_cores_cases as cc
from tests import route_cores_restate as rc
from tests import slot_agent
from tests.oracle_backend import OracleBackend
from tests.test_rmcsa_complete import CROWDED, CROWDED_POINTS, CROWDED_SEEDS, POINTS, STATE_SEEDS
from tests.test_rmcsa_complete_gpu import crowd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOPOLOGY = slot_agent.TOPOLOGY
K, M = 5, 6
WALKS = [(name, steps) for name in cc.SHAPES for steps in POINTS] + [(CROWDED.name, CROWDED_POINTS[1])]
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
# k_route_spectrum<W, ROUTE_CUTS> of the parent commit, read with tools/kernel_regs.py: W -> (vgpr spills, sgpr spills, scratch bytes)
PARENT_ROUTE_CUTS = {1: (0, 0, 0), 2: (0, 0, 0), 5: (0, 0, 0), 8: (0, 0, 0)}


def test_header_and_binding_declare_both_exports():
    h = open(os.path.join(ROOT, "include", "orl.h")).read()
    assert re.search(r"int orl_batch_route_cores\(orl_batch\* b, int rule, int route, int modulation[^;]*, int n_given,\s*const int32_t\* given[^;]*,"
                     r"\s*int32_t\* actions_out[^;]*, int32_t\* table_out[^;]*\);", h)
    assert re.search(r"int orl_batch_core_table_shape\(const orl_batch\* b, int32_t\* rows, int32_t\* width, int32_t\* pitch\);", h)
    assert re.search(r"#define ORL_ABI_VERSION 2\b", h) and _lib.ABI_VERSION == 2
    for name, value in (("ORL_ROUTE_KSP_BEST_CORE", "3"), ("ORL_ROUTE_KSP_LEAST_LOADED_CORE", "4"), ("ORL_BUF_CORE_TABLE", "12")):
        assert re.search(r"#define %s %s\b" % (name, value), h), name
    assert len(_lib.EXPORTS["orl_batch_route_cores"][1]) == 8 and len(_lib.EXPORTS["orl_batch_core_table_shape"][1]) == 4
    from optical_rl_gym_amd.envs import BatchedOpticalEnv as B

    assert B.CORE_RULES == rc.RULE_IDS and tuple(B.CORE_RULES) == rc.RULES
    assert B.CORE_ROUTES == {"ksp": 0, "best": 1, "least_loaded": 2, "ksp_best_core": 3, "ksp_least_loaded_core": 4} and tuple(B.CORE_ROUTES) == rc.ROUTES
    assert B.ROUTES == {"ksp": 0, "best": 1, "least_loaded": 2}  # (route_spectrum's stay three)
    assert B._BUFFERS["core_table"][0] == 12 and "route_cores()" in B._VIEWS["core_table"][0]
    assert B.core_route_ids("min_cuts", "ksp_least_loaded_core") == (6, 4) and B.core_route_ids(3, 1) == (3, 1)
    for bad in (("most_used", "ksp"), ("least_used", "ksp"), ("worst", "ksp"), ("first", "shortest")):
        with pytest.raises(ValueError):
            B.core_route_ids(*bad)
    # the prefix: (path), (path, core); cores alone, bad shapes and a contradicting n_given are refused in Python
    ok = np.zeros(4, np.int32)
    assert B.core_prefix(None, None, None, 4) == (None, 0) and B.core_prefix(None, None, 2, 4) == (None, 2)
    g, n = B.core_prefix(ok + 3, ok + 1, None, 4)
    assert n == 2 and g.dtype == np.int32 and g.tolist() == [[3, 1]] * 4 and B.core_prefix(ok, None, None, 4)[1] == 1
    for bad in ((None, ok, None), (ok[:3], None, None), (ok, ok[:3], None), (ok.astype(np.float64), None, None), (ok, ok, 1), (ok, None, 2),
                (ok.reshape(4, 1), None, None)):
        with pytest.raises(ValueError):
            B.core_prefix(bad[0], bad[1], bad[2], 4)


def test_facades_offer_the_call_to_rmcsa():
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd import gym_api
    from optical_rl_gym_amd.sharding import MultiDeviceBatch

    for cls in (orl.envs.BatchedOpticalEnv, MultiDeviceBatch, gym_api.RMCSAEnv):
        assert hasattr(cls, "route_cores"), cls
    for cls in (orl.envs.BatchedOpticalEnv, MultiDeviceBatch):
        assert hasattr(cls, "core_table_shape"), cls
    for cls in (gym_api.RMSAEnv, gym_api.RWAEnv, gym_api.DeepRMSAEnv):
        assert not hasattr(cls, "route_cores"), cls


@needs_hipcc
def test_kernels_exist_for_every_row_width_and_mode_without_lds_or_spills():
    """k_route_cores<W, MODE> for every row width, ROUTE_PLAIN (0) and ROUTE_CUTS (2): no LDS; the plain one without spills or
    scratch, the cut one with no more of either than k_route_spectrum<W, ROUTE_CUTS> of the parent commit — and than
    this build's."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs

    from optical_rl_gym_amd import _build

    figures = lambda k: (int(k["vgpr_spill_count"]), int(k["sgpr_spill_count"]), int(k["private_segment_fixed_size"]))
    for variant in ("default", "alt"):
        found, spectrum = {}, {}
        for k in kernel_regs.kernels(_build.build(variant=variant)):
            name = kernel_regs.demangle(k["name"])
            m = re.match(r"(?:void )?k_route_cores<(\d+), (\d+)>", name)
            if m:
                found[int(m.group(1)), int(m.group(2))] = k
            m = re.match(r"(?:void )?k_route_spectrum<(\d+), 2>", name)
            if m:
                spectrum[int(m.group(1))] = k
        assert sorted(found) == sorted((w, mode) for w in _build.ROW_WIDTHS for mode in (0, 2)), variant
        for (w, mode), k in found.items():
            print(variant, w, mode, k)
            assert int(k["group_segment_fixed_size"]) == 0, (w, mode, k)
            if mode == 0:
                assert figures(k) == (0, 0, 0), (w, k)
            else:
                assert all(a <= b for a, b in zip(figures(k), PARENT_ROUTE_CUTS[w])), (w, k)
                assert all(a <= b for a, b in zip(figures(k), figures(spectrum[w]))), (w, k)


@needs_hipcc
def test_plan_and_shape():
    """View 8, appended behind orl_batch_route_spectrum's: RMCSA only, a table row of 4 K C int32 at a pitch of 4 K C, 4 wavefronts, no
    LDS whatever the rule, a grid that covers B and not a workgroup more."""
    from tests.helpers import VIEW_PLAN_FIELDS

    lib = _lib.lib()
    f = {n: i for i, n in enumerate(VIEW_PLAN_FIELDS)}
    out = (ctypes.c_int32 * len(VIEW_PLAN_FIELDS))()
    for env in (0, 1, 2, 4):
        assert lib.orl_debug_view_plan(env, 1, 8, 14, 22, 5, 1, 64, 1, 6, 8, 0, out) == 0  # no such view for another family
    assert lib.orl_debug_view_plan(3, 1, 8, 14, 22, 5, 7, 64, 1, 6, 9, 0, out) == 0  # no view 9
    for W, S in ((1, 64), (2, 128), (5, 320), (8, 512)):
        for K_, C in ((1, 1), (5, 7), (5, 31), (8, 1), (64, 31)):
            for B in (1, 31, 32, 33, 65536):
                for rule in (0, 1, 2, 3, 6):
                    assert lib.orl_debug_view_plan(3, W, B, 14, 22, K_, C, S, 1, 6, 8, rule, out) == len(VIEW_PLAN_FIELDS)
                    r = list(out)
                    assert (r[f["dim"]], r[f["rows"]], r[f["width"]], r[f["pitch"]], r[f["elem_bytes"]]) == (4 * K_ * C, K_ * C, 4, 4 * K_ * C, 4)
                    assert (r[f["ok"]], r[f["waves"]], r[f["block"]], r[f["lds_bytes"]], r[f["counted"]]) == (1, 4, 256, 0, 0)
                    assert (r[f["grid"]] - 1) * 32 < B <= r[f["grid"]] * 32


# ---- the restatement -------------------------------------------------------------------------------------------------------
def _restatement_checks(avail, services, topo, tab, envs, fixed_mods):
    """On the envs `envs` of a state: tables and routes against the one-loop key searches, prefixes included, and against
    complete_restate.  Returns the Prepared of modulation=None over all envs."""
    pv = rr.prov_all(avail, services, topo, tab)
    prep = rc.Prepared(avail, services, topo, tab, None, pv)
    C, S = prep.C, prep.S
    tabs = {rule: rc.table(prep, rule) for rule in rc.RULES}
    g1, g2 = cc.draw_given(prep.n, K, C, 1), cc.draw_given(prep.n, K, C, 2)
    for rule in rc.RULES:
        tab_ = tabs[rule]
        for i in envs:
            for p in range(K):
                for c in range(C):
                    want = rc.brute_winner(prep, i, p, c, rule)
                    row = tab_[i, p * C + c]
                    got = None if row[1] == rc.NO_FIT else (int(row[0]), int(row[1]))
                    assert got == want, (rule, i, p, c)
                    if want is None:
                        assert row[0] == S and (prep.mod[i][p] >= 0 or (row[2:] == 0).all())
        for route in rc.ROUTES:
            for given in (None, g1, g2):
                acts = rc.route(prep, tab_, route, given)
                for i in envs:
                    assert tuple(acts[i]) == rc.brute_action(prep, i, rule, route, () if given is None else tuple(int(v) for v in given[i])), (
                        rule, route, i, None if given is None else given[i])
    # first + ksp is the first-fit completion
    first = tabs["first"]
    assert np.array_equal(rc.route(prep, first, "ksp"), cr.complete(pv, services, topo, tab, 0))
    for p in range(-1, K + 1):
        given = np.full((prep.n, 1), p, np.int32)
        assert np.array_equal(rc.route(prep, first, "ksp", given), cr.complete(pv, services, topo, tab, 1, given)), p
    for m in fixed_mods:
        sub = np.array(list(envs))
        pm = rc.Prepared(avail[sub], services[sub], topo, tab, m, pv[sub])
        tm = rc.table(pm, "first")
        for p in range(-1, K + 1):
            for c in range(-1, C + 1):
                want = cr.complete(pv[sub], services[sub], topo, tab, 3, np.tile(np.array([p, m, c], np.int32), (len(sub), 1)))
                got = rc.route(pm, tm, "ksp", np.tile(np.array([p, c], np.int32), (len(sub), 1)))
                assert np.array_equal(got, want), (m, p, c)
    return prep


def _state(ora, rows):
    return rr.unpack_cores(ora.slots_packed()[rows], ora.C, ora.E, ora.S), ora.services()[rows].copy()


@functools.lru_cache(maxsize=None)
def _walked(name, steps):
    """One oracle state per seed after `steps` agent steps, each held by one env per (rule, route) (the oracle has no snapshot);
    the restatement on it, on its crowded and on its crafted maps; then the oracle stepped with every restated action."""
    case = CROWDED if name == CROWDED.name else slot_agent.CASE_BY_NAME[name]
    topo, tab = slot_agent.topology(), slot_agent.rmcsa_tables("rmcsa_c7_s64" if case is CROWDED else name)
    C, S = slot_agent.cores_of(case), case.S
    probes = [(rule, route) for rule in rc.RULES for route in rc.ROUTES]
    seeds = CROWDED_SEEDS[:12] if case is CROWDED else STATE_SEEDS
    R, G = len(probes), len(seeds)
    lead = np.arange(G) * R
    ora = OracleBackend("RMCSA", TOPOLOGY, list(np.repeat(seeds, R)), **case.kw)
    rng = np.random.RandomState(steps + S)
    for t in range(steps):
        avail, services = _state(ora, lead)
        acts, _ = slot_agent.rmcsa_agent_actions(avail, services, topo, tab, t, rng, S, C)
        ora.step(np.repeat(acts, R, axis=0), auto_reset=True)
    avail, services = _state(ora, lead)
    seen = {}
    prep = _restatement_checks(avail, services, topo, tab, range(G), fixed_mods=range(M) if steps == POINTS[0] else ())
    rc.count_kinds(prep, seen)
    for maps in (crowd(avail, services, topo, tab), cc.craft(avail, services, topo, tab)):
        rc.count_kinds(_restatement_checks(maps, services, topo, tab, range(G), fixed_mods=()), seen)
    # the oracle's own step under every rule x route: accepted exactly when the action is not the reject action, and exactly the
    # slots [s*, s* + n) taken on the hops of p in core c
    actions = np.zeros((G * R, 4), np.int32)
    for j, (rule, route) in enumerate(probes):
        actions[lead + j] = rc.route(prep, rc.table(prep, rule), route)
    before, acc0 = _state(ora, np.arange(G * R))[0], ora.counters()[:, 1].copy()
    ora.step(actions, auto_reset=False)
    after, accepted = _state(ora, np.arange(G * R))[0], ora.counters()[:, 1] - acc0
    reject = np.array(prep.reject)
    gone = 0
    for e in range(G * R):
        i, a = e // R, actions[e]
        rej = bool((a == reject).all())
        assert accepted[e] == (0 if rej else 1), (probes[e % R], i, a)
        want = np.zeros_like(before[e])
        if not rej:
            p, m, c, s = (int(v) for v in a)
            src, dst = int(services[i, 2]), int(services[i, 3])
            assert m == prep.mod[i][p] and prep.need[i][p] == int(cr.slots_of(services, tab)[i, m])
            want[c, topo.path_links[src, dst, p, :int(topo.path_hops[src, dst, p])], s:s + prep.need[i][p]] = True
        taken = before[e] & ~after[e]
        if not np.array_equal(taken, want):  # (a service that leaves before the next arrival is released within the same step)
            assert not taken.any(), (probes[e % R], i, a)
            gone += 1
    assert gone <= G * R // 20, gone  # holding time 10 against an inter-arrival time of 1 / 15: well under one in twenty
    return seen


@pytest.mark.parametrize("name,steps", WALKS)
def test_restatement_is_the_brute_force_the_completion_and_what_the_oracle_provisions(name, steps):
    print(name, steps, _walked(name, steps))


def test_the_states_hold_every_kind_the_gpu_test_needs():
    """A reject, a ksp winner in a core above 0, a later path, every other route leaving ksp's choice, a cost tie between two pairs,
    s* + n == S, an exact hit and an exact miss, a min_cuts winner that is not first fit, cuts 0 and cuts >= 2, m*(p) other than the
    path's best-modulation byte, a path out of reach, a window across a word: each at least once over the states above."""
    total = {}
    for name, steps in WALKS:
        for kind, count in _walked(name, steps).items():
            total[kind] = total.get(kind, 0) + count
    print(total)
    assert set(total) == set(rc.KINDS) and all(total[k] > 0 for k in rc.KINDS), {k: total.get(k, 0) for k in rc.KINDS}
