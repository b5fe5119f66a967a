"""Routing rules and the per-path assignment table for RMSA and RWA actions (include/orl.h, orl_batch_route_spectrum) without a GPU:
the ABI surface, the kernel's instantiations in the code object, the facades, the launch plan, and the restatement the GPU tests
compare with (tests/route_restate.py) — pinned to the reference's own heuristics through the oracle, to the restatement of
orl_batch_assign_spectrum, to brute-force loops and to the oracle's step — with the preconditions of the GPU test established on
the states that test uses (tests/assign_cases.py walks either backend; tests/route_cases.py crafts the rest)."""
import ctypes
import functools
import os
import re
import shutil
import sys

import numpy as np
import pytest

from optical_rl_gym_amd import _lib
from tests import assign_cases as ac
from tests import assign_restate as ar
from tests import route_cases as rc
from tests import route_restate as rr
from tests.oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = ac.K
POINTS = (30, 90)  # agent steps before the probe (tests/test_assign_spectrum.py's)
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


def test_header_and_binding_declare_the_call():
    h = open(os.path.join(ROOT, "include", "orl.h")).read()
    assert re.search(r"int orl_batch_route_spectrum\(orl_batch\* b, int rule, int route, int32_t\* actions_out[^;]*,\s*int32_t\* table_out[^;]*\);", h)
    assert re.search(r"int orl_batch_assign_table_shape\(const orl_batch\* b, int32_t\* rows, int32_t\* width, int32_t\* pitch\);", h)
    assert re.search(r"#define ORL_ABI_VERSION 2\b", h) and _lib.ABI_VERSION == 2
    for name, value in (("ORL_ASSIGN_MIN_CUTS", "6"), ("ORL_ROUTE_KSP", "0"), ("ORL_ROUTE_BEST", "1"), ("ORL_ROUTE_LEAST_LOADED", "2"),
                        ("ORL_ROUTE_NO_FIT", "0x7fffffff"), ("ORL_BUF_ASSIGN_TABLE", "11")):
        assert re.search(r"#define %s %s\b" % (name, value), h), name
    assert len(_lib.EXPORTS["orl_batch_route_spectrum"][1]) == 5 and len(_lib.EXPORTS["orl_batch_assign_table_shape"][1]) == 4
    from optical_rl_gym_amd.envs import BatchedOpticalEnv as B

    assert tuple(B.ASSIGN_RULES) == ar.RULES and tuple(B.ROUTE_RULES) == rr.RULES and tuple(B.ROUTES) == rr.ROUTES
    assert B.ROUTE_RULES == dict(B.ASSIGN_RULES, min_cuts=6) and B.ROUTES == {"ksp": 0, "best": 1, "least_loaded": 2}
    assert rr.NO_FIT == 0x7FFFFFFF and B._BUFFERS["assign_table"][0] == 11
    assert B.route_ids("min_cuts", "least_loaded") == (6, 2) and B.route_ids(3, 1) == (3, 1)
    for bad in (("worst", "ksp"), ("first", "shortest")):
        with pytest.raises(ValueError):
            B.route_ids(*bad)


def test_facades_offer_the_routes_to_rmsa_and_rwa_only():
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd import gym_api
    from optical_rl_gym_amd.sharding import MultiDeviceBatch

    for cls in (orl.envs.BatchedOpticalEnv, MultiDeviceBatch, gym_api.RMSAEnv, gym_api.RWAEnv):
        assert hasattr(cls, "route_spectrum"), cls
    for cls in (orl.envs.BatchedOpticalEnv, MultiDeviceBatch):
        assert hasattr(cls, "assign_table_shape"), cls
    assert not hasattr(gym_api.DeepRMSAEnv, "route_spectrum") and not hasattr(gym_api.RMCSAEnv, "route_spectrum")


@needs_hipcc
def test_kernels_exist_for_every_row_width_and_instantiation_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs

    from optical_rl_gym_amd import _build

    lib = _build.build()
    found = {}
    for k in kernel_regs.kernels(lib):
        m = re.match(r"(?:void )?k_route_spectrum<(\d+), (\d+)>", kernel_regs.demangle(k["name"]))
        if m:
            found[int(m.group(1)), int(m.group(2))] = k
    assert sorted(found) == sorted((w, mode) for w in _build.ROW_WIDTHS for mode in (0, 1, 2))  # plain, counted, cuts
    for key, k in found.items():
        assert int(k["vgpr_spill_count"]) == 0 and int(k["sgpr_spill_count"]) == 0 and int(k["private_segment_fixed_size"]) == 0, (key, k)


@needs_hipcc
def test_plan_and_shape():
    """view 7, appended behind the seven pinned by tests/test_view_plan.py: VIEW_ASSIGN's plan for rules 0 - 5 (min_cuts: the plain
    one), a table row of 4 K int32 at a pitch of 4 K, LDS within 48 KiB, a grid that covers B and not a workgroup more."""
    from tests.helpers import VIEW_PLAN_FIELDS, VIEWS

    lib = _lib.lib()
    f = {n: i for i, n in enumerate(VIEW_PLAN_FIELDS)}

    def plan(view, W, B, K_, S, rule, env=0):
        out = (ctypes.c_int32 * len(VIEW_PLAN_FIELDS))()
        assert lib.orl_debug_view_plan(env, W, B, 14, 22, K_, 1, S, 1, 6, view, rule, out) == len(VIEW_PLAN_FIELDS)
        return list(out)

    assert len(VIEWS) == 7 and VIEWS.index("assign") == 3
    out = (ctypes.c_int32 * len(VIEW_PLAN_FIELDS))()
    assert lib.orl_debug_view_plan(0, 1, 8, 14, 22, 5, 1, 64, 1, 6, 8, 0, out) == 0  # no view 8
    for W, S in ((1, 64), (2, 128), (5, 320), (8, 512)):
        for K_ in (1, 5, 8, 9, 64):
            for B in (1, 31, 32, 33, 65536):
                for rule in range(7):
                    for env in (0, 2):
                        r = plan(7, W, B, K_, S, rule, env)
                        assert (r[f["dim"]], r[f["rows"]], r[f["width"]], r[f["pitch"]], r[f["elem_bytes"]]) == (4 * K_, K_, 4, 4 * K_, 4)
                        a = plan(3, W, B, K_, S, min(rule, 3) if rule == 6 else rule, env)
                        assert r[f["ok"]:] == a[f["ok"]:], (W, K_, B, rule)
                        assert r[f["ok"]] == 1 and r[f["lds_bytes"]] <= 48 * 1024 and r[f["block"]] == 64 * r[f["waves"]]
                        assert (r[f["lds_bytes"]] > 0) == (rule in (4, 5)) == bool(r[f["counted"]])
                        per_wg = 8 * r[f["waves"]]
                        assert (r[f["grid"]] - 1) * per_wg < B <= r[f["grid"]] * per_wg


# ---- the restatement -------------------------------------------------------------------------------------------------------
def _brute_checks(prep, links, envs):
    """Every rule's per-path winner against a plain loop over all (p, s) with a key tuple; every route against a plain loop over paths"""
    k, S = prep.k, prep.S
    for rule in rr.RULES:
        tab = rr.table(prep, links, rule)
        for i in envs:
            for p in range(k):
                want = rr.brute_winner(prep, links, i, p, rule) if p < len(prep.m[i]) else None
                got = None if tab[i, p, 1] == rr.NO_FIT else (int(tab[i, p, 0]), int(tab[i, p, 1]))
                assert got == want, (rule, i, p)
                if want is None:
                    assert tab[i, p, 0] == S and (p < len(prep.m[i]) or (tab[i, p, 2:] == 0).all())
            fit = [p for p in range(k) if tab[i, p, 1] != rr.NO_FIT]
            for route in rr.ROUTES:
                a = rr.route(tab[i:i + 1], route, k, S)[0]
                if not fit:
                    assert tuple(a) == (k, S, 0, 0)
                    continue
                if route == "ksp":
                    p = fit[0]
                elif route == "best":
                    p = min(fit, key=lambda q: (int(tab[i, q, 1]), q))
                else:
                    p = min(fit, key=lambda q: (-int(tab[i, q, 3]), q))
                assert tuple(a) == (p, int(tab[i, p, 0]), 0, 0), (rule, route, i)


def _sibling_checks(prep, links):
    """Route ksp under rules 0 - 5 is assign_spectrum's n_given = 0; column 0 of table row p its n_given = 1 on path p"""
    k, S = prep.k, prep.S
    for rule in ar.RULES:
        tab = rr.table(prep, links, rule)
        assert np.array_equal(rr.route(tab, "ksp", k, S), ar.assign(prep, rule, 0)), rule
        for p in range(k):
            given = np.full(prep.n, p, np.int32)
            assert np.array_equal(tab[:, p, 0], ar.assign(prep, rule, 1, given)[:, 1]), (rule, p)


def _fewest_hops_first(tab, services, topo, S):
    """RWA only.  The reference's RWA shortest_available_path_first_fit (rwa_env.py:438-458) is not k-shortest-path order: among the
    paths with a free wavelength it takes the one with the FEWEST HOPS (ties: the lowest index), and the k paths are ordered by
    length, not hops — on NSFNET a later path often has fewer hops, so route "ksp" (the lowest p, which an existing GPU test pins to
    assign_spectrum) differs from it by definition (measured on rwa_nsf_s129 after 30 steps: 5 of 24 envs).  The pin to the
    reference is therefore taken on the table: SAP_FF's answer on EVERY env is the first-fit row of the fewest-hop path that fits."""
    out = np.zeros((len(tab), 4), np.int32)
    for i in range(len(tab)):
        src, dst = int(services[i, 2]), int(services[i, 3])
        fit = [p for p in range(tab.shape[1]) if tab[i, p, 1] != rr.NO_FIT]
        p = min(fit, key=lambda q: (int(topo.path_hops[src, dst, q]), q)) if fit else None
        out[i, :2] = (tab.shape[1], S) if p is None else (p, tab[i, p, 0])
    return out


@functools.lru_cache(maxsize=None)
def _walked(name):
    """The oracle of a shape walked to the POINTS; at each: the reference pin, the sibling pin, the brute-force loops, and a step of
    the oracle with restated actions (rule and route by env index)."""
    shape = ac.SHAPE_BY_NAME[name]
    topo = ac.topology(shape.topology)
    ora = OracleBackend(shape.fam, shape.topology, ac.seeds_of(shape), **shape.kw)
    rng = np.random.RandomState(shape.S)
    t, n = 0, shape.envs
    # the reference's RMSA heuristics search range(0, S - n): last_start=False; its RWA ones try every wavelength (rwa_env.py:496)
    last_start = shape.fam == "RWA"
    for point in POINTS:
        ac.agent_steps(ora, shape, point - t, rng, t0=t)
        t = point
        avail, services = ac.state_of(ora, shape)
        prep, links = rc.prepared(shape.fam, topo, K, shape.S, avail, services)
        first = rr.table(prep, links, "first", last_start=last_start)
        for route, policy in (("ksp", "SAP_FF"), ("least_loaded", "LLP_FF")):
            got, want = rr.route(first, route, K, shape.S), np.array(ora.policy(policy), np.int32)
            if shape.fam == "RWA" and policy == "SAP_FF":
                got = _fewest_hops_first(first, services, topo, shape.S)
            bad = np.flatnonzero((got != want).any(axis=1))
            print(name, point, route, policy, "envs that differ: %d of %d" % (len(bad), n))
            assert len(bad) == 0, (name, point, policy, bad[:5], got[bad[:5]], want[bad[:5]])
        _sibling_checks(prep, links)
        _brute_checks(prep, links, range(min(n, 32)))
        exp = rc.expected(shape.fam, topo, K, shape.S, avail, services)
        actions = np.zeros((n, 4), np.int32)
        for i in range(n):
            actions[i] = exp[rr.RULES[i % 7]][1][rr.ROUTES[(i // 7) % 3]][i]
        before = ora.counters()[:, 1].copy()
        ora.step(actions, auto_reset=True)
        t += 1
        accepted = ora.counters()[:, 1] - before
        # the oracle provisions the service exactly when the answer is not the reject action
        assert np.array_equal(accepted == 1, actions[:, 0] < K) and set(np.unique(accepted)) <= {0, 1}, (name, point)
        assert (actions[:, 0] < K).any()
    return True


@pytest.mark.parametrize("name", ac.CPU_SHAPES)
def test_restatement_is_the_reference_the_sibling_the_brute_force_and_what_the_oracle_provisions(name):
    assert _walked(name)


@functools.lru_cache(maxsize=None)
def _kinds(name):
    """What the states of the GPU test hold for a shape, here from the oracle: the walked state, its crowded and its crafted maps"""
    shape = ac.SHAPE_BY_NAME[name]
    topo = ac.topology(shape.topology)
    ora = OracleBackend(shape.fam, shape.topology, ac.seeds_of(shape), **shape.kw)
    ac.agent_steps(ora, shape, ac.AGENT_STEPS, np.random.RandomState(shape.S))
    avail, services = ac.state_of(ora, shape)
    seen = {}
    for maps in (avail, ac.crowd(shape, avail, services), rc.craft(shape.fam, topo, K, shape.S, avail, services)):
        rc.expected(shape.fam, topo, K, shape.S, maps, services, seen)
    prep, links = rc.prepared(shape.fam, topo, K, shape.S, rc.craft(shape.fam, topo, K, shape.S, avail, services), services)
    _brute_checks(prep, links, range(min(shape.envs, 16)))
    return seen


@pytest.mark.parametrize("fam", ["RMSA", "RWA"])
def test_the_states_hold_every_kind_the_gpu_test_needs(fam):
    """Per family, over the states tests/test_route_spectrum_gpu.py checks for the shapes walked here too: no completion, route best
    and route least_loaded on another path than ksp, a cost tie between two paths, a min_cuts winner that is not first fit, a tie
    of cuts within a path, c* = 0 and c* >= 2 under min_cuts, a min_cuts winner at s = 0 and one with s + n = S, and (RMSA) a window
    across a word edge.  A condition on the inputs, not a measurement."""
    total = {}
    for name in ac.CPU_SHAPES:
        if ac.SHAPE_BY_NAME[name].fam == fam:
            for kind, c in _kinds(name).items():
                total[kind] = total.get(kind, 0) + c
    print(fam, total)
    missing = [kind for kind in (rr.RMSA_KINDS if fam == "RMSA" else rr.KINDS) if total.get(kind, 0) == 0]
    assert not missing, (missing, total)
