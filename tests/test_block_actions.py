"""Block actions (include/orl.h, orl_batch_block_table / orl_batch_select_blocks) without a GPU: the ABI surface, the facades, the launch
plan of view 9, the kernels in the code object, and the restatement the GPU tests compare with (tests/block_restate.py) — pinned to a
per-slot loop, to mask_restate's DeepRMSA block list, to the oracle's own step (a DeepRMSA oracle stepped with block indices beside an
RMSA oracle stepped with the restated actions) and to the first-fit tables of route_restate / route_cores_restate — with the kinds the
GPU test needs established on walked, crowded and crafted states."""
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
from tests import block_restate as br
from tests import mask_restate as mr
from tests import rmcsa_mask_restate as rr
from tests import route_cases
from tests import route_cores_cases as cc
from tests import route_cores_restate as rcr
from tests import route_restate
from tests import slot_agent
from tests.oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOPOLOGY = slot_agent.TOPOLOGY
K = 5
J_KINDS = 3  # the block count the kinds are counted under
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
# k_path_features<W> of the parent commit, read with tools/kernel_regs.py: W -> (vgpr spills, sgpr spills, scratch bytes)
PARENT_PATH_FEATURES = {1: (0, 0, 0), 2: (0, 0, 0), 5: (0, 6, 0), 8: (0, 22, 0)}
# the shapes walked on the oracle here (the GPU test walks them on the device the same way, among its others)
RMSA_SHAPES, RWA_SHAPES, RMCSA_SHAPES = ("rmsa_nsf_s65", "rmsa_nsf_s129"), ("rwa_nsf_s129",), ("rmcsa_c7_s64", "rmcsa_c2_s129")
RMCSA_STEPS, CPU_ENVS = 30, 48


def test_header_and_binding_declare_the_exports():
    h = open(os.path.join(ROOT, "include", "orl.h")).read()
    assert re.search(r"int orl_batch_block_table_shape\(const orl_batch\* b, int j, int32_t\* rows, int32_t\* width[^;]*, int32_t\* table_pitch,"
                     r"\s*int32_t\* mask_dim, int32_t\* mask_pitch\);", h)
    assert re.search(r"int orl_batch_block_table\(orl_batch\* b, int j, int modulation[^;]*, int32_t\* table_out[^;]*,\s*uint8_t\* mask_out[^;]*\);", h)
    assert re.search(r"int orl_batch_select_blocks\(orl_batch\* b, int j, int modulation, int placement,\s*const int32_t\* given[^;]*,"
                     r"\s*int32_t\* actions_out[^;]*\);", h)
    assert re.search(r"#define ORL_ABI_VERSION 2\b", h) and _lib.ABI_VERSION == 2
    for name, value in (("ORL_BUF_BLOCK_TABLE", "13"), ("ORL_BUF_BLOCK_MASK", "14"), ("ORL_BLOCK_FIRST", "0"), ("ORL_BLOCK_LAST", "1"),
                        ("ORL_BUF_CORE_TABLE", "12")):
        assert re.search(r"#define %s %s\b" % (name, value), h), name
    assert [len(_lib.EXPORTS[n][1]) for n in ("orl_batch_block_table_shape", "orl_batch_block_table", "orl_batch_select_blocks")] == [7, 5, 6]
    from optical_rl_gym_amd.envs import BatchedOpticalEnv as B

    assert B.BLOCK_PLACEMENTS == {"first": 0, "last": 1}
    assert B._BUFFERS["block_table"][0] == 13 and B._BUFFERS["block_mask"][0] == 14 and B._BUFFERS["block_mask"][1] == B._BUFFERS["action_mask"][1]
    assert "block_table()" in B._VIEWS["block_table"][0] and "block_table()" in B._VIEWS["block_mask"][0]
    # what existing tests pin stays as it was
    assert len(B.MASK_LAYOUTS) == 4 and B.ROUTES == {"ksp": 0, "best": 1, "least_loaded": 2} and len(B.CORE_ROUTES) == 5 and len(B.ASSIGN_RULES) == 6
    # the Python-side refusals
    ok = np.zeros(4, np.int32)
    assert B.block_indices(None, 4) is None and B.block_indices(ok + 3, 4).dtype == np.int32
    assert B.block_indices(np.arange(4, dtype=np.int64), 4).tolist() == [0, 1, 2, 3]
    for bad in (ok[:3], ok.astype(np.float64), ok.reshape(4, 1), ok.reshape(2, 2)):
        with pytest.raises(ValueError):
            B.block_indices(bad, 4)
    with pytest.raises(ValueError):
        B._named_id("placement", B.BLOCK_PLACEMENTS, "middle")
    assert B._named_id("placement", B.BLOCK_PLACEMENTS, "last") == 1


def test_facades_offer_the_calls_where_they_should():
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd import gym_api
    from optical_rl_gym_amd.sharding import MultiDeviceBatch

    for cls in (orl.envs.BatchedOpticalEnv, MultiDeviceBatch):
        for name in ("block_table_shape", "block_table", "select_blocks"):
            assert hasattr(cls, name), (cls, name)
    for cls in (gym_api.RMSAEnv, gym_api.RWAEnv, gym_api.RMCSAEnv):
        assert hasattr(cls, "block_action") and hasattr(cls, "block_mask"), cls
    assert not hasattr(gym_api.DeepRMSAEnv, "block_action") and not hasattr(gym_api.DeepRMSAEnv, "block_mask")


def test_vec_env_refuses_block_actions_where_they_do_not_belong():
    from optical_rl_gym_amd.vec_env import OpticalVecEnv

    for fam, kw in (("DeepRMSA", dict(j=2)), ("QoSConstrainedRA", dict(load=10)), ("RMSA", {})):  # (the oracle stand-in has no select_blocks)
        with pytest.raises(ValueError, match="RMSA, RWA and RMCSA"):
            OpticalVecEnv(OracleBackend(fam, TOPOLOGY, [1, 2], **kw), block_actions=2)
    for kw in (dict(spectrum_assignment="first"), dict(action_completion="path")):
        with pytest.raises(ValueError):  # (the stand-in has neither sibling: which refusal comes first is not pinned here)
            OpticalVecEnv(OracleBackend("RMSA", TOPOLOGY, [1, 2]), block_actions=2, **kw)


@needs_hipcc
def test_kernels_exist_for_every_row_width_without_scratch():
    """k_block_table<W> and k_select_blocks<W> for every row width: the selection without spills or scratch, the table with no more of
    either than k_path_features<W> of the parent commit — and than this build's."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs

    from optical_rl_gym_amd import _build

    figures = lambda k: (int(k["vgpr_spill_count"]), int(k["sgpr_spill_count"]), int(k["private_segment_fixed_size"]))
    found = {"k_block_table": {}, "k_select_blocks": {}, "k_path_features": {}}
    for k in kernel_regs.kernels(_build.build()):
        m = re.match(r"(?:void )?(k_block_table|k_select_blocks|k_path_features)<(\d+)>", kernel_regs.demangle(k["name"]))
        if m:
            found[m.group(1)][int(m.group(2))] = k
    for name in found:
        assert sorted(found[name]) == sorted(_build.ROW_WIDTHS), name
    for w in _build.ROW_WIDTHS:
        print(w, {name: figures(found[name][w]) for name in found})
        assert figures(found["k_select_blocks"][w]) == (0, 0, 0), w
        assert int(found["k_select_blocks"][w]["group_segment_fixed_size"]) == 0, w
        assert all(a <= b for a, b in zip(figures(found["k_block_table"][w]), PARENT_PATH_FEATURES[w])), w
        assert all(a <= b for a, b in zip(figures(found["k_block_table"][w]), figures(found["k_path_features"][w]))), w


@needs_hipcc
def test_plan_and_shape():
    """View 9, appended behind VIEW_ROUTE_CORES: the table's row shape and pitch, staged exactly where eight envs' table rows fit 48 KiB
    beside the mask's words, a grid that covers B and not a workgroup more; views 0 - 8 answer as they did."""
    from tests.helpers import VIEW_PLAN_FIELDS

    lib = _lib.lib()
    f = {n: i for i, n in enumerate(VIEW_PLAN_FIELDS)}
    out = (ctypes.c_int32 * len(VIEW_PLAN_FIELDS))()
    L = len(VIEW_PLAN_FIELDS)
    for j in (0, 9, -1):
        assert lib.orl_debug_view_plan(0, 1, 8, 14, 22, 5, 1, 64, 1, 6, 9, j, out) == 0
    assert lib.orl_debug_view_plan(4, 1, 8, 14, 22, 5, 1, 64, 1, 6, 9, 1, out) == 0  # QoSConstrainedRA has no slot maps
    assert lib.orl_debug_view_plan(0, 1, 8, 14, 22, 5, 1, 64, 1, 6, 10, 1, out) == 0  # no view 10
    staged_seen = set()
    for env in (0, 1, 2, 3):
        for W, S in ((1, 64), (2, 128), (5, 320), (8, 512)):
            for K_, C in ((1, 1), (5, 1), (9, 1), (64, 1)) if env != 3 else ((5, 7), (5, 31), (5, 2), (8, 31)):
                for j in (1, 3, 4, 8):
                    R = K_ * C
                    dim = R * (2 + 2 * j)
                    pitch = (dim + 3) // 4 * 4
                    mask_bytes, table_bytes = 8 * (R + 2) * 4, 8 * pitch * 4
                    for B in (1, 31, 32, 33, 65536):
                        assert lib.orl_debug_view_plan(env, W, B, 14, 22, K_, C, S, 1, 6, 9, j, out) == L
                        r = list(out)
                        assert (r[f["dim"]], r[f["rows"]], r[f["width"]], r[f["pitch"]], r[f["elem_bytes"]]) == (dim, R, 2 + 2 * j, pitch, 4)
                        staged = mask_bytes + table_bytes <= 48 * 1024
                        per_wave = mask_bytes + (table_bytes if staged else 0)
                        waves = max(w for w in (1, 2, 4) if w * per_wave <= 48 * 1024)
                        assert (r[f["ok"]], r[f["staged"]], r[f["waves"]], r[f["block"]], r[f["lds_bytes"]]) == (1, int(staged), waves, 64 * waves, waves * per_wave)
                        assert r[f["lds_bytes"]] <= 48 * 1024 and r[f["chunk"]] == 0 and r[f["counted"]] == 0
                        assert (r[f["grid"]] - 1) * 8 * waves < B <= r[f["grid"]] * 8 * waves
                        staged_seen.add(staged)
    assert staged_seen == {True, False}  # (31 cores at j = 8: the direct form)
    # more rows than one wavefront's mask words fit: refused
    assert lib.orl_debug_view_plan(3, 1, 8, 14, 22, 64, 31, 64, 1, 6, 9, 1, out) == L and list(out)[f["ok"]] == 0
    # the path features' plan is what it was, whatever this view adds: staged iff 8 rows of floats fit, no mask words
    for j, C in ((1, 7), (8, 31)):
        assert lib.orl_debug_view_plan(3, 1, 64, 14, 22, 5, C, 64, 1, 6, 4, j, out) == L
        r = list(out)
        pitch = (29 + 5 * C * (2 * j + 3) + 3) // 4 * 4
        assert r[f["pitch"]] == pitch and r[f["staged"]] == int(8 * pitch * 4 <= 48 * 1024)


# ---- the restatement -------------------------------------------------------------------------------------------------------
def _pin(env_type, avail, services, topo, tables, modulation, allow_rejection, js=(1, 2, 3, 8)):
    """Table, mask and selection of a state against the per-slot loop; returns the Rows"""
    rows = br.Rows(env_type, avail, services, topo, tables, modulation)
    S = rows.S
    for i in range(rows.n):
        for r in range(rows.R):
            if rows.need[i][r]:
                assert br.blocks_of(rows, i, r) == br.brute_blocks(rows.row[i][r], rows.need[i][r], S), (i, r)
    rng = np.random.default_rng(S)
    for j in js:
        tab, msk = br.table(rows, j), br.mask(rows, j, allow_rejection)
        assert tab.shape == (rows.n, rows.R, 2 + 2 * j) and msk.shape == (rows.n, rows.R * j + 1)
        exists = tab[:, :, 3::2] > 0
        raw = br.mask(rows, j, allow_rejection, fallback=False)
        assert np.array_equal(raw[:, :-1], exists.reshape(rows.n, -1)) and (raw[:, -1] == allow_rejection).all()
        assert (tab[:, :, 2::2][~exists] == S).all() and (np.diff(exists.astype(int), axis=2) <= 0).all()  # the listed blocks come first
        for a in (br.draw_indices(rows, j, rng), np.arange(rows.n, dtype=np.int32) % (rows.R * j)):
            first, last = br.select(rows, j, a, "first"), br.select(rows, j, a, "last")
            for i in range(rows.n):
                ok = 0 <= a[i] < rows.R * j and raw[i, a[i]]
                assert (tuple(first[i]) != rows.reject) == (tuple(last[i]) != rows.reject) == bool(ok), (j, i, a[i])
                if ok:
                    r, b = int(a[i]) // j, int(a[i]) % j
                    st, L = int(tab[i, r, 2 + 2 * b]), int(tab[i, r, 3 + 2 * b])
                    n = rows.need[i][r]
                    assert first[i, -1 if env_type == 3 else 1] == st and last[i, -1 if env_type == 3 else 1] == st + L - n
                    assert all(rows.row[i][r][st:st + L]) and (st == 0 or not rows.row[i][r][st - 1]) and (st + L == S or not rows.row[i][r][st + L])
    return rows


def _single_core(fam, shape, avail, services, seen):
    """One RMSA / RWA state [n, links, S]: the per-slot loop, mask_restate's DeepRMSA block list, route_restate's first-fit table"""
    topo = ac.topology(shape.topology)
    env_type, S = ac.ENV_TYPE[fam], shape.S
    rows = _pin(env_type, avail[:, None], services, topo, None, None, True)
    br.count_kinds(rows, J_KINDS, seen)
    prep, links = route_cases.prepared(fam, topo, K, S, avail, services)
    first = route_restate.table(prep, links, "first")
    tab = br.table(rows, 1)
    fits = first[:, :, 1] != route_restate.NO_FIT
    assert np.array_equal(tab[:, :, 0], first[:, :, 2]) and np.array_equal(tab[:, :, 1], first[:, :, 3])
    assert np.array_equal(tab[:, :, 2], first[:, :, 0]) and np.array_equal(tab[:, :, 3] > 0, fits)
    if fam == "RMSA":  # the same numbers under DeepRMSA's rule: its joint mask is the block list's
        for j in (1, 2, 3, 8):
            deep = br.Rows(1, avail[:, None], services, topo)
            for allow in (False, True):
                assert np.array_equal(br.mask(deep, j, allow), mr.restate(1, avail, services, topo, K, S, j=j, allow_rejection=allow)), j


@functools.lru_cache(maxsize=None)
def _single_core_kinds(name):
    shape = ac.SHAPE_BY_NAME[name]
    ora = OracleBackend(shape.fam, shape.topology, ac.seeds_of(shape), **shape.kw)
    ac.agent_steps(ora, shape, ac.AGENT_STEPS, np.random.RandomState(shape.S))
    avail, services = ac.state_of(ora, shape)
    avail, services = avail[:CPU_ENVS], services[:CPU_ENVS]
    seen = {}
    for maps in (avail, ac.crowd(shape, avail, services), br.craft(ac.ENV_TYPE[shape.fam], avail[:, None], services, ac.topology(shape.topology))[:, 0]):
        _single_core(shape.fam, shape, maps, services, seen)
    return seen


@functools.lru_cache(maxsize=None)
def _rmcsa_kinds(name):
    from tests.test_rmcsa_complete_gpu import crowd

    case = slot_agent.CASE_BY_NAME[name]
    topo, tab = slot_agent.topology(), slot_agent.rmcsa_tables(name)
    C, S = slot_agent.cores_of(case), case.S
    n = 24
    ora = OracleBackend("RMCSA", TOPOLOGY, list(range(1000, 1000 + n)), **case.kw)
    rng = np.random.RandomState(S)
    state = lambda: (rr.unpack_cores(ora.slots_packed(), C, ora.E, S), ora.services().copy())
    for t in range(RMCSA_STEPS):
        avail, services = state()
        ora.step(slot_agent.rmcsa_agent_actions(avail, services, topo, tab, t, rng, S, C)[0], auto_reset=True)
    avail, services = state()
    fixed = cc.fixed_modulation(services, topo, tab)
    seen = {}
    for maps in (avail, crowd(avail, services, topo, tab), br.craft(3, avail, services, topo, tab)):
        for mod in (None, fixed):
            rows = _pin(3, maps, services, topo, tab, mod, True, js=(1, 3, 8))
            if mod is None:
                br.count_kinds(rows, J_KINDS, seen)
            else:
                seen["fixed_beyond_reach"] = seen.get("fixed_beyond_reach", 0) + rows.fixed_beyond_reach
            # block 0 is the first-fit row of the (path, core) table; n and free its columns 2 and 3
            first = rcr.table(rcr.Prepared(maps, services, topo, tab, mod), "first")
            got = br.table(rows, 1)
            assert np.array_equal(got[:, :, 0], first[:, :, 2]) and np.array_equal(got[:, :, 1], first[:, :, 3]), (name, mod)
            assert np.array_equal(got[:, :, 2], first[:, :, 0]) and np.array_equal(got[:, :, 3] > 0, first[:, :, 1] != rcr.NO_FIT), (name, mod)
    return seen


@pytest.mark.parametrize("fam,names", [("RMSA", RMSA_SHAPES), ("RWA", RWA_SHAPES), ("RMCSA", RMCSA_SHAPES)])
def test_restatement_is_the_slot_loop_and_its_siblings_and_the_states_hold_every_kind(fam, names):
    """Per family over the walked, crowded and crafted states: rows with 0, 1 .. j - 1, exactly j and more than j blocks (j = 3), a block
    that ends at S - 1, one that starts at 0, one of exactly n slots, one across a 64-bit word edge, a run shorter than n between two
    blocks (not RWA, where n = 1); RMCSA: a path without a usable modulation and a fixed modulation beyond reach.  A condition on the inputs."""
    total = {}
    for name in names:
        for kind, c in (_rmcsa_kinds(name) if fam == "RMCSA" else _single_core_kinds(name)).items():
            total[kind] = total.get(kind, 0) + c
    print(fam, total)
    missing = [kind for kind in {"RMSA": br.KINDS, "RWA": br.RWA_KINDS, "RMCSA": br.RMCSA_KINDS}[fam] if total.get(kind, 0) == 0]
    assert not missing, (missing, total)


@pytest.mark.parametrize("j", [1, 2, 3])
def test_deeprmsa_oracle_stepped_with_indices_keeps_the_maps_of_rmsa_stepped_with_the_restated_actions(j):
    """The oracle's own DeepRMSA decode (deeprmsa_env.py:48-58) against select(): same configuration and seeds, 300 steps; half the envs
    take a block that exists where there is one, the others a uniformly random index (absent blocks and the reject action included)."""
    n, S = 16, 129
    kw = dict(load=130, mean_service_holding_time=10.0, num_spectrum_resources=S, allow_rejection=True, episode_length=50)
    seeds = list(range(300, 300 + n))
    deep_kw = dict({k_: v for k_, v in kw.items() if k_ != "load"}, j=j, mean_service_inter_arrival_time=10.0 / 130)  # (DeepRMSA takes the inter-arrival time)
    deep, rmsa = OracleBackend("DeepRMSA", TOPOLOGY, seeds, **deep_kw), OracleBackend("RMSA", TOPOLOGY, seeds, **kw)
    topo = slot_agent.topology()
    rng = np.random.default_rng(j)
    absent = rejected = placed = 0
    for t in range(300):
        avail = mr.unpack_slots(rmsa.slots_packed(), topo.n_links, S, mr.row_words(S))
        services = rmsa.services()
        assert np.array_equal(services, deep.services()), t
        rows = br.Rows(0, avail[:, None], services, topo)
        msk = br.mask(rows, j, True, fallback=False)
        a = rng.integers(0, K * j + 1, size=n)
        for i in range(0, n, 2):
            have = np.flatnonzero(msk[i, :-1])
            if len(have):
                a[i] = have[rng.integers(len(have))]
        acts = br.select(rows, j, a, "first")
        absent += int((~msk[np.arange(n), a] & (a < K * j)).sum())
        rejected += int((a == K * j).sum())
        placed += int((acts[:, 0] < K).sum())
        _, _, done_d, _ = deep.step(a.reshape(n, 1), auto_reset=True)
        _, _, done_r, _ = rmsa.step(acts, auto_reset=True)
        assert np.array_equal(done_d, done_r), t
        assert np.array_equal(deep.slots_packed(), rmsa.slots_packed()), t
        assert np.array_equal(deep.counters(), rmsa.counters()), t
    print(j, dict(absent=absent, rejected=rejected, placed=placed))
    assert absent > 0 and rejected > 0 and placed > 300
    assert rmsa.counters()[:, 1].sum() == placed  # every selection that is not the reject row provisions
