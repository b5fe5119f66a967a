"""Release horizons (include/orl.h, orl_batch_release_horizons) without a GPU: the release-time model the GPU test compares with
(tests/horizon_model.py) against the oracle, the restatement (tests/horizon_restate.py) against the oracle's slot maps and the block
restatement, the kinds the walked states must hold, the ABI surface and the facades, the launch plan, and the kernel's registers.

Seeds: env e of every walk is seeded horizon_model.SEED0 + e = 4100 + e, 24 envs per shape; loads and steps: horizon_model.WALKS."""
import ctypes
import functools
import os
import re
import shutil
import sys

import numpy as np
import pytest

from optical_rl_gym_amd import _lib
from tests import block_restate as br
from tests import horizon_model as hm
from tests import horizon_restate as hr
from tests import route_cores_cases as cc
from tests import slot_agent
from tests.oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
ENV_TYPE = {"RMSA": 0, "RWA": 2, "RMCSA": 3}
SHAPES = {"RMSA": ("rmsa_nsf_s65", "rmsa_nsf_s129"), "RWA": ("rwa_nsf_s129",), "RMCSA": ("rmcsa_c7_s64", "rmcsa_c2_s129")}
J_KINDS = 3
PLAN_FIELDS = ("dim", "rows", "width", "pitch", "ok", "waves", "block", "grid", "lds_bytes", "rows_per_round")


def and_rows(avail, services, topo):
    """bool [n, K C, S]: the AND of the hops' free rows per candidate row; a missing path's row all True"""
    n, C, _, S = avail.shape
    K = topo.k_paths
    out = np.ones((n, K * C, S), bool)
    for e in range(n):
        src, dst = int(services[e, 2]), int(services[e, 3])
        for p in range(int(topo.n_paths[src, dst])):
            links = topo.path_links[src, dst, p, :int(topo.path_hops[src, dst, p])]
            out[e, p * C:(p + 1) * C] = avail[e][:, links, :].all(axis=1)
    return out


def check_restatement(fam, tab, avail, services, pending, topo, seen):
    """The restatement on one state: H > 0 exactly on the AND-row's busy slots, -1 rows for missing paths, the BLOCKS rows in step with
    block_restate.table, every finite value > 0.  Returns {(layout, j, modulation): rows} — what the GPU test compares the device with."""
    n, C, _, S = avail.shape
    K = topo.k_paths
    H = hr.slots_layout(pending, services, topo, C, S, seen)
    body = H[:, :-1].reshape(n, K * C, S)
    free = and_rows(avail, services, topo)
    n_paths = topo.n_paths[services[:, 2].astype(int), services[:, 3].astype(int)]
    for e in range(n):
        live = int(n_paths[e]) * C
        assert np.array_equal(body[e, :live] > 0, ~free[e, :live]), e
        assert (body[e, :live] >= 0).all() and (body[e, live:] == -1.0).all(), e
    assert np.array_equal(H[:, -1], services[:, 1].astype(np.float32))
    out = {("slots", 1, None): H}
    mods = (None, cc.fixed_modulation(services, topo, tab)) if fam == "RMCSA" else (None,)
    for mod in mods:
        rows = br.Rows(ENV_TYPE[fam], avail, services, topo, tab, mod)
        if mod is not None:
            seen["fixed_beyond_reach"] = seen.get("fixed_beyond_reach", 0) + rows.fixed_beyond_reach
        else:
            seen["no_modulation"] = seen.get("no_modulation", 0) + int(fam == "RMCSA" and any(0 in need for need in rows.need))
        for j in (1, 3, 8):
            B = hr.blocks_layout(H, rows, j, services, seen if (mod is None and j == J_KINDS) else None)
            pairs = B[:, :-1].reshape(n, K * C, j, 2)
            exists = br.table(rows, j)[:, :, 3::2] > 0
            assert np.array_equal((pairs != -1.0).all(axis=3), exists) and np.array_equal((pairs == -1.0).all(axis=3), ~exists), (j, mod)
            assert (pairs[exists] > 0).all(), (j, mod)  # finite or +inf: both neighbours of a listed block are busy slots or the edge
            out["blocks", j, mod] = B
    return out


@functools.lru_cache(maxsize=None)
def walked(name):
    """The named walk on the oracle with the model beside it: at every checkpoint the model's count is the oracle's active(), its records
    laid into an empty map are the oracle's slot map, and the restatement holds; returns the kinds seen"""
    fam, kw, S, n, seeds = hm.walk_config(name)
    C = kw.get("num_spatial_resources", 1)
    ora = OracleBackend(fam, slot_agent.TOPOLOGY, seeds, **kw)
    tab = slot_agent.rmcsa_tables(name) if fam == "RMCSA" else None
    model = hm.Model(fam, ora.topology, n, tab)
    seen = {"checkpoints": 0}

    def checkpoint(tag):
        active, avail, services = ora.active(), hm.avail_of(ora, C, S), ora.services()
        for e in range(n):
            assert len(model.ev[e]) == active[e], (name, tag, e, len(model.ev[e]), int(active[e]))
            assert np.array_equal(model.busy(e, C, S), (~avail[e]).astype(np.int64)), (name, tag, e)
        check_restatement(fam, tab, avail, services, [(model.times(e), model.records(e)) for e in range(n)], ora.topology, seen)
        seen["checkpoints"] += 1
        seen["hole"] = seen.get("hole", 0) + sum(model.out_of_order)

    acc, ref = hm.walk(name, ora, model, checkpoint)
    assert acc > 0 and ref > 0, (name, acc, ref)  # the agent walks accept services and are refused some
    ora.reset(full=True)
    model.reset_full()
    checkpoint("reset")
    return seen


@pytest.mark.parametrize("name", [n for names in SHAPES.values() for n in names])
def test_model_is_the_oracle_and_the_restatement_holds(name):
    seen = walked(name)
    print(name, seen)
    assert seen["checkpoints"] >= 7


@pytest.mark.parametrize("fam", list(SHAPES))
def test_the_walked_states_hold_every_kind(fam):
    """What the GPU test's states (the same walks and seeds) therefore hold, per family: a slot under two services with different release
    times (on different links: one link's slot has one holder); a row without a busy slot and one without a free slot; busy slots 63 and
    64 of a row with different horizons; a release that shares no link with any candidate path; an env with more than 128 releases and one
    with none (after the full reset); a record that left while an older one stayed (a hole in the release table, or its reuse); a block
    at slot 0, one that ends at S, a row with fewer than j = 3 blocks; RMCSA: a release on another core of a shared link, a row the
    service cannot use (no modulation within reach) and a fixed modulation beyond reach.  A condition on the inputs."""
    total = {}
    for name in SHAPES[fam]:
        for kind, c in walked(name).items():
            total[kind] = total.get(kind, 0) + c
    kinds = ["two_services_one_slot", "row_all_free", "row_all_busy", "edge_63_64_differ", "shares_no_link", "over_128", "none_pending", "hole",
             "block_at_0", "block_ends_at_S", "fewer_than_j"]
    if fam == "RMCSA":
        kinds += ["other_core", "unusable_row", "no_modulation", "fixed_beyond_reach"]
    print(fam, total)
    missing = [k for k in kinds if total.get(k, 0) == 0]
    assert not missing, (missing, total)


def test_restatement_marks_missing_paths_and_takes_the_later_release():
    """A hand-made state on a pair: two releases over one slot on different links of path 0 (the later one wins), one that shares no
    link, and a pair given fewer paths than k (its rows -1)."""
    import copy

    topo = copy.copy(slot_agent.topology())
    S, N = 16, topo.n_nodes
    src, dst = 0, N - 1
    hops = int(topo.path_hops[src, dst, 0])
    assert hops >= 2
    l0, l1 = (int(x) for x in topo.path_links[src, dst, 0, :2])
    # one-hop paths over those two links, and one over a link path 0 does not use
    single = {}
    for a in range(N):
        for b in range(N):
            for p in range(int(topo.n_paths[a, b])):
                if int(topo.path_hops[a, b, p]) == 1:
                    single.setdefault(int(topo.path_links[a, b, p, 0]), (a * N + b, p))
    cand = set()
    for p in range(int(topo.n_paths[src, dst])):
        cand |= hr.link_set(topo, src, dst, p)
    off = next(l for l in single if l not in cand)
    times = np.array([7.5, 9.25, 30.0])
    recs = np.array([single[l0] + (3, 2, 0), single[l1] + (4, 3, 0), single[off] + (0, 16, 0)], np.int64)
    service = np.array([5.0, 2.5, src, dst, 100, 0], np.float64)
    topo.n_paths = topo.n_paths.copy()
    topo.n_paths[src, dst] = 2
    seen = {}
    H = hr.slots_rows(times, recs, service, topo, 1, S, seen)
    assert H.shape == (topo.k_paths, S) and (H[2:] == -1.0).all()
    assert H[0, 3] == np.float32(2.5) and H[0, 4] == np.float32(4.25) and H[0, 5] == np.float32(4.25) and H[0, 6] == np.float32(4.25) and H[0, 7] == 0
    assert seen["two_services_one_slot"] == 1 and seen["shares_no_link"] == 1 and seen["missing_path"] == 1


def test_header_and_binding_declare_the_exports():
    h = open(os.path.join(ROOT, "include", "orl.h")).read()
    assert re.search(r"int orl_batch_release_horizons_shape\(const orl_batch\* b, int layout, int j, int32_t\* rows, int32_t\* width, int64_t\* dim, "
                     r"int64_t\* pitch\);", h)
    assert re.search(r"int orl_batch_release_horizons\(orl_batch\* b, int layout, int j, int modulation, float\* out[^;]*\);", h)
    assert re.search(r"int orl_debug_horizon_plan\(int env_type, int W, int64_t B, int N, int E, int K, int C, int S, int M, int layout, int j, int32_t\* out\);", h)
    assert re.search(r"int orl_debug_set_horizon_rows\(orl_batch\* b, int rows\);", h)
    assert re.search(r"#define ORL_ABI_VERSION 2\b", h) and _lib.ABI_VERSION == 2
    for name, value in (("ORL_BUF_RELEASE_HORIZONS", "15"), ("ORL_HORIZON_SLOTS", "0"), ("ORL_HORIZON_BLOCKS", "1"), ("ORL_BUF_BLOCK_MASK", "14")):
        assert re.search(r"#define %s %s\b" % (name, value), h), name
    assert [len(_lib.EXPORTS[n][1]) for n in ("orl_batch_release_horizons_shape", "orl_batch_release_horizons", "orl_debug_horizon_plan",
                                              "orl_debug_set_horizon_rows")] == [7, 5, 12, 2]
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "orl_debug_set_horizon_rows" in integration and "orl_debug_horizon_plan" in integration
    from optical_rl_gym_amd.envs import BatchedOpticalEnv as B

    assert B.HORIZON_LAYOUTS == {"slots": 0, "blocks": 1}
    assert B._BUFFERS["release_horizons"] == (15, "<f4", None) and "call release_horizons()" in B._VIEWS["release_horizons"][0]
    assert B._BUFFERS["block_mask"][0] == 14 and len(B._BUFFERS) == 16  # what was there stays
    # the Python-side refusals
    assert B.horizon_args("slots") == (0, 1, -1) and B.horizon_args("blocks", 8, 2) == (1, 8, 2) and B.horizon_args(1, 3) == (1, 3, -1)
    for bad in (("rows",), ("blocks", 0), ("blocks", 9), ("slots", 2), ("slots", 1, 0), ("slots", 1, 3)):
        with pytest.raises(ValueError):
            B.horizon_args(*bad)


def test_facades_offer_the_calls_where_they_should():
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd import gym_api
    from optical_rl_gym_amd.sharding import MultiDeviceBatch

    for cls in (orl.envs.BatchedOpticalEnv, MultiDeviceBatch):
        for name in ("release_horizons_shape", "release_horizons"):
            assert hasattr(cls, name), (cls, name)
    for cls in (gym_api.RMSAEnv, gym_api.DeepRMSAEnv, gym_api.RWAEnv, gym_api.RMCSAEnv):
        assert hasattr(cls, "release_horizons"), cls
    from optical_rl_gym_amd.qos import QoSConstrainedRA

    assert not hasattr(QoSConstrainedRA, "release_horizons")


@needs_hipcc
def test_plan_and_shape():
    """orl_debug_horizon_plan over the families, row widths, (k, cores), layouts, j and batch sizes: the rows' shape as defined; one
    wavefront per env, 4, 2 or 1 per workgroup; LDS within 48 KiB; the rounds cover R; a grid that covers B and not a workgroup more; and
    orl_debug_view_plan still answers for views 0 - 9 alone."""
    lib = _lib.lib()
    f = {n: i for i, n in enumerate(PLAN_FIELDS)}
    out = (ctypes.c_int32 * len(PLAN_FIELDS))()
    L = len(PLAN_FIELDS)
    rounds_seen, waves_seen, refused = set(), set(), 0
    for env in (0, 1, 2, 3):
        for W, S in ((1, 64), (2, 128), (5, 320), (8, 512)):
            for K_, C in ((1, 1), (5, 1), (64, 1)) if env != 3 else ((5, 7), (5, 2), (8, 31)):
                R = K_ * C
                for layout in (0, 1):
                    for j in (1, 8):
                        for B in (1, 31, 32, 33, 65536):
                            assert lib.orl_debug_horizon_plan(env, W, B, 14, 22, K_, C, S, 6, layout, j, out) == L
                            r = list(out)
                            if layout == 0 and j != 1:
                                assert r == [0] * L
                                continue
                            width = S if layout == 0 else 2 * j
                            dim = R * width + 1
                            pitch = (dim + 3) // 4 * 4
                            assert (r[f["dim"]], r[f["rows"]], r[f["width"]], r[f["pitch"]]) == (dim, R, width, pitch)
                            assert r[f["ok"]] == 1, (env, W, K_, C, layout, j)
                            waves, rows = r[f["waves"]], r[f["rows_per_round"]]
                            assert waves in (1, 2, 4) and r[f["block"]] == 64 * waves and 0 < r[f["lds_bytes"]] <= 48 * 1024
                            assert 1 <= rows <= R and (rows == R or waves == 1)
                            # the wavefront's share holds the link table (22 links), the BLOCKS output row and the round's window
                            need = 22 * 8 + 4 * ((pitch if layout else 0) + rows * S + 1)
                            assert r[f["lds_bytes"]] >= waves * need and r[f["lds_bytes"]] % 16 == 0
                            assert (r[f["grid"]] - 1) * waves < B <= r[f["grid"]] * waves
                            rounds_seen.add(-(-R // rows) > 1)
                            waves_seen.add(waves)
    assert rounds_seen == {False, True} and waves_seen == {1, 2, 4}
    for layout in (0, 1):
        assert lib.orl_debug_horizon_plan(4, 1, 8, 14, 22, 5, 1, 64, 6, layout, 1, out) == L and list(out) == [0] * L  # QoSConstrainedRA
    for layout, j in ((2, 1), (-1, 1), (1, 0), (1, 9)):
        assert lib.orl_debug_horizon_plan(0, 1, 8, 14, 22, 5, 1, 64, 6, layout, j, out) == L and list(out) == [0] * L
    # an output row that no workgroup's LDS holds: refused
    assert lib.orl_debug_horizon_plan(3, 1, 8, 14, 22, 64, 31, 64, 6, 1, 8, out) == L and list(out)[f["ok"]] == 0
    # the views' own plan is what it was
    from tests.helpers import VIEW_PLAN_FIELDS

    vout = (ctypes.c_int32 * len(VIEW_PLAN_FIELDS))()
    for view in range(10):
        fam = 3 if view in (1, 2, 8) else (4 if view == 6 else 0)
        assert lib.orl_debug_view_plan(fam, 1, 8, 14, 22, 5, 2, 64, 1, 6, view, 1 if view != 1 else 2, vout) == len(VIEW_PLAN_FIELDS), view
    assert lib.orl_debug_view_plan(0, 1, 8, 14, 22, 5, 1, 64, 1, 6, 10, 1, vout) == 0  # no view 10


@needs_hipcc
def test_kernel_exists_for_every_row_width_without_scratch_or_vgpr_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs

    from optical_rl_gym_amd import _build

    found = {}
    for k in kernel_regs.kernels(_build.build()):
        m = re.match(r"(?:void )?k_release_horizons<(\d+)>", kernel_regs.demangle(k["name"]))
        if m:
            found[int(m.group(1))] = k
    assert sorted(found) == sorted(_build.ROW_WIDTHS)
    for w, k in found.items():
        print(w, {x: k[x] for x in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")})
        assert int(k["vgpr_spill_count"]) == 0 and int(k["private_segment_fixed_size"]) == 0, w
        assert int(k["group_segment_fixed_size"]) == 0, w  # (its LDS is the launch's: horizon_plan)
