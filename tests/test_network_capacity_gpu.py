"""The network capacity view on the device (include/orl.h, orl_batch_network_capacity; k_network_capacity in csrc/orl_capacity.h) against
the numpy restatement (tests/capacity_restate.py, pinned to the oracle in tests/test_network_capacity.py): all three layouts on every env
with ==, from slots_packed() of that moment — at construction, after a warm-up under the family's heuristic and after slot_agent's
boundary-seeking agent steps, over the row widths, core counts and topologies at which the kernel can go wrong; against the existing
views on the same state; after every way of stepping; under graph capture; over two shards; the facades; and the refusals.  The shapes of
tests/capacity_cases.py add k = 8 / 9 / 16 / 64, the stars (N > 64, n_paths < k), 30 hops, 1 / 2 / 63 / 64 / 65 classes, the slot maps left
in global memory (germany50 RMCSA, 10 cores of 512 slots) and the refusal of the per-path array on a real batch (star129)."""
import functools
import os

import numpy as np
import pytest

from tests import assign_cases as ac
from tests import capacity_cases as cc
from tests import capacity_restate as cap
from tests import envelope
from tests import horizon_model as hm
from tests import slot_agent

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY_KW = dict(load=40, mean_service_holding_time=10.0, episode_length=50, num_spectrum_resources=64, allow_rejection=True)
# name -> (envs, warm-up steps under the heuristic, load where the shape's own leaves the maps too empty for blocked cells)
SHAPES = {"rmsa_nsf_s64": (24, 150, None), "rmsa_nsf_s65": (24, 150, None), "rmsa_nsf_s129": (24, 700, 220), "rmsa_nsf_s321": (24, 900, 500),
          "rmsa_nsf_s512": (24, 500, 600), "rwa_nsf_s129": (24, 1100, 1500), "rwa_nsf_s512": (24, 1500, 1500), "rmsa_ger_s128": (4, 600, 500),
          "rmcsa_c7_s64": (24, 200, None), "rmcsa_c2_s129": (20, 900, 1200), "rmcsa_c31_s64": (24, 300, None), "tiny5_k3": (24, 200, None)}
AGENT_STEPS = 6
# the shapes at the edges of the accepted range and the unstaged one: name -> tests/capacity_cases.py's (family, topology, k, keywords,
# envs, heuristic, warm-up steps, what it is there for, the blocked cells the oracle showed)
ENVELOPE_SHAPES = cc.SHAPE_BY_NAME
LAYOUTS = ("paths", "serviceable", "counts")


def config(name):
    """(family, topology, keywords, S) of a named shape: tests/assign_cases.py's, tests/slot_agent.py's, or the 5-node topology"""
    if name == "tiny5_k3":
        return "RMSA", os.path.join(GOLDEN, "tiny5_k3.npz"), dict(TINY_KW), 64
    if name in ac.SHAPE_BY_NAME:
        s = ac.SHAPE_BY_NAME[name]
        fam, topo, kw, S = s.fam, s.topology, dict(s.kw), s.S
    else:
        c = slot_agent.CASE_BY_NAME[name]
        fam, topo, kw, S = c.fam, slot_agent.TOPOLOGY, dict(c.kw), c.S
    if SHAPES[name][2] is not None:
        kw["load"] = SHAPES[name][2]
    return fam, topo, kw, S


@functools.lru_cache(maxsize=None)
def need_of(name):
    """The need table of a shape, computed once and left unchanged"""
    from optical_rl_gym_amd.topology import Topology

    fam, topo, kw, _ = config(name)
    tab = slot_agent.rmcsa_tables(name) if fam == "RMCSA" else None
    need = cap.need_table(fam, Topology.load(topo), cap.class_rates(fam, kw), tab)
    need.setflags(write=False)
    return need


def make(name, n=None, **over):
    import optical_rl_gym_amd as orl

    fam, topo, kw, S = config(name)
    kw.update(over)
    n = SHAPES[name][0] if n is None else n
    env = orl.make(fam, topology=topo, num_envs=n, seeds=[hm.SEED0 + e for e in range(n)], **kw)
    return env, fam, (slot_agent.rmcsa_tables(name) if fam == "RMCSA" else None), kw.get("num_spatial_resources", 1), S


def shape_of(env, fam, C, need):
    N, K, n_cls = env.topology.n_nodes, env.k_paths, need.shape[3]
    cores = C if fam == "RMCSA" else 1
    return {"paths": (N * N * K * cores, 2), "serviceable": (N * N, n_cls), "counts": (1, n_cls + N * N)}


_ONE_ENV = {}  # restatements of single envs by their packed maps (germany50 at 10 cores of 512 slots: most of a second each)


def restate_each(env, C, S, need):
    """cap.restate one env at a time, each distinct slot map once"""
    packed, avail = env.slots_packed(), hm.avail_of(env, C, S)
    parts = []
    for e in range(env.num_envs):
        key = (id(need), packed[e].tobytes())
        if key not in _ONE_ENV:
            _ONE_ENV[key] = cap.restate(avail[e:e + 1], env.topology, need)
        parts.append(_ONE_ENV[key])
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


def compare(env, fam, C, S, need, what, state_untouched=False, layouts=LAYOUTS, each=False):
    """All three layouts of the present state against the restatement from slots_packed(), on every env, with ==; the shapes as defined"""
    cores = C if fam == "RMCSA" else 1
    want = dict(zip(LAYOUTS, restate_each(env, cores, S, need) if each else cap.restate(hm.avail_of(env, cores, S), env.topology, need)))
    before = (env.get_state(), env.flags().copy()) if state_untouched else None
    for layout, (rows, width) in shape_of(env, fam, C, need).items():
        if layout not in layouts:
            continue
        dim = rows * width
        pitch = (dim + 15) // 16 * 16 if layout == "serviceable" else (dim + 3) // 4 * 4
        assert env.network_capacity_shape(layout) == (rows, width, dim, pitch), (what, layout)
        got = env.network_capacity(layout)
        assert got.shape == (env.num_envs, dim) and got.dtype == (np.bool_ if layout == "serviceable" else np.int32), (what, layout)
        bad = np.flatnonzero((got != want[layout]).any(axis=1))
        if len(bad):
            e = int(bad[0])
            col = int(np.flatnonzero(got[e] != want[layout][e])[0])
            raise AssertionError("%s, %s: %d envs differ; env %d column %d (row %d, %d): got %r, want %r"
                                 % (what, layout, len(bad), e, col, col // width, col % width, got[e, col], want[layout][e, col]))
    if before is not None:
        assert np.array_equal(env.get_state(), before[0]) and np.array_equal(env.flags(), before[1]), what
    return want


def agent_steps(env, fam, tab, C, S, steps, rng):
    for t in range(steps):
        acts = hm.agent_actions(fam, hm.avail_of(env, C, S), env.services(), env.topology, tab, t, rng, S, C)
        env.step(np.ascontiguousarray(acts, np.int32), auto_reset=True)


@pytest.mark.parametrize("name", list(SHAPES))
def test_all_layouts_equal_the_restatement_on_the_shapes(name):
    """At construction every existing path has L = F = S and every cell within reach is 1; then the warm-up under the heuristic, which must
    leave blocked and serviceable cells; then slot_agent's boundary-seeking agents (the 5-node topology, whose k = 3 they are not written
    for, steps the heuristic instead)."""
    env, fam, tab, C, S = make(name)
    need = need_of(name)
    n, (N, K, n_cls) = env.num_envs, (env.topology.n_nodes, env.k_paths, need.shape[3])
    want = compare(env, fam, C, S, need, name + ", construction", state_untouched=True)
    P = want["paths"].reshape(n, N, N, K, -1, 2)
    exists = np.arange(K)[None, None, :] < env.topology.n_paths[:, :, None]
    assert (P[:, exists] == S).all() and (P[:, ~exists] == -1).all()
    reach = (exists[:, :, :, None] & (need >= 1) & (need <= S)).any(axis=2)
    assert np.array_equal(want["serviceable"].reshape(n, N, N, n_cls), np.broadcast_to(reach, (n, N, N, n_cls)))
    pol = hm.HEURISTIC[fam]
    env.run(pol, SHAPES[name][1])
    want = compare(env, fam, C, S, need, name + ", warm-up", state_untouched=True)
    blocked, served = want["counts"][:, :n_cls].sum(axis=1), want["counts"][:, n_cls:].sum(axis=1)
    print(name, "blocked cells per env", blocked.min(), blocked.max(), "of", int((env.topology.n_paths > 0).sum()) * n_cls)
    # (512 wavelengths on 22 links block a pair from some 4 500 services in flight, beyond the release table of the batches tested here:
    # rwa_nsf_s512 covers the row width, rwa_nsf_s129 the blocked pairs)
    assert ((blocked > 0).any() or name == "rwa_nsf_s512") and (served > 0).all(), (name, blocked)
    assert (want["paths"].reshape(n, -1, 2)[:, :, 0] == 0).any() or name != "rwa_nsf_s129"  # RWA blocks a pair only with every path full
    if name == "tiny5_k3":
        for _ in range(AGENT_STEPS):
            env.policy_step(pol, auto_reset=True, fetch=False)
        between = want["paths"].reshape(n, N, N, K, 2)
        assert ((between[:, :, :, 0, 0] >= 0) & (between[:, :, :, 2, 0] == -1)).any()  # rows of (-1, -1) behind real ones
    else:
        agent_steps(env, fam, tab, C, S, AGENT_STEPS, np.random.RandomState(S + C))
    compare(env, fam, C, S, need, name + ", agent steps")
    assert not (env.flags() & 2).any()
    env.check()
    env.close()


@pytest.mark.parametrize("n", [1, 9, 24])
@pytest.mark.parametrize("name", ["rmsa_nsf_s65", "rmcsa_c7_s64"])
def test_batch_sizes_with_a_partly_empty_last_workgroup(name, n):
    env, fam, tab, C, S = make(name, n=n)
    env.run(hm.HEURISTIC[fam], SHAPES[name][1])
    compare(env, fam, C, S, need_of(name), "%s, %d envs" % (name, n))
    env.close()


def test_one_wavefront_with_more_than_the_default_lds():
    """31 cores of 512 slots: 49 104 bytes of slot maps in LDS beside the longest runs, one wavefront per workgroup with the limit raised
    for the kernel (4 envs: the restatement's path rows are what costs the time)"""
    name = "rmcsa_c31_s64"
    env, fam, tab, C, S = make(name, n=4, num_spectrum_resources=512)
    S = 512
    need = need_of(name)  # (the needs do not depend on S)
    compare(env, fam, C, S, need, "c31 s512, construction")
    env.run(hm.HEURISTIC[fam], 400)
    want = compare(env, fam, C, S, need, "c31 s512, run", state_untouched=True)
    assert (want["paths"].reshape(4, -1, 2)[:, :, 1] < S)[want["paths"].reshape(4, -1, 2)[:, :, 0] >= 0].any()
    env.check()
    env.close()


def make_envelope(shape, tmp_path, n=None):
    """A batch of a shape of tests/capacity_cases.py -> (env, need, C, S)"""
    import optical_rl_gym_amd as orl

    topo = envelope.topology_npz(shape.topo, shape.k, tmp_path)
    env = orl.make(shape.fam, topology=topo, num_envs=shape.envs if n is None else n, seeds=cc.seeds_of(shape, n), **shape.kw)
    return env, cc.need_of(shape, topo)[0], cc.cores_of(shape), cc.spectrum_of(shape)


def assert_a_path_of_index_8_or_more_decides(shape, env, need, want):
    """k > 8: some pair's "serviceable" row has a 1 that only a path of index >= 8 explains — every row of paths 0 .. 7 of the pair has
    L < need (want: what compare() found the device's rows equal to)"""
    second = cc.only_through_second_word(want["paths"], need, env.topology, env.num_envs)
    M = want["serviceable"].reshape(second.shape)
    assert second.any() and M[second].all(), shape.name
    print(shape.name, "cells only a path >= 8 serves:", int(second.sum()), "in", int(second.any(axis=(1, 2, 3)).sum()), "envs")
    assert int(second.any(axis=(1, 2, 3)).sum()) == shape.second_word  # (what the oracle showed)


@pytest.mark.parametrize("name", list(ENVELOPE_SHAPES))
def test_envelope_shapes_equal_the_restatement_at_three_moments(name, tmp_path):
    """Every shape of tests/capacity_cases.py at construction, after its warm-up under its heuristic and after a few policy_steps; the
    blocked cells after the warm-up are the oracle's (tests/test_network_capacity.py); star129 in "paths" alone, the other two layouts
    being refused for it (test_the_per_path_array_is_refused_on_a_real_batch)."""
    shape = ENVELOPE_SHAPES[name]
    env, need, C, S = make_envelope(shape, tmp_path)
    fam, n_cls = cc.need_family(shape), need.shape[3]
    kw = dict(layouts=("paths",) if name == "star129_rmsa" else LAYOUTS, each=name == cc.UNSTAGED)
    want = compare(env, fam, C, S, need, name + ", construction", state_untouched=True, **kw)
    got = want["paths"].reshape(env.num_envs, -1, 2)
    assert ((got == S) | (got == -1)).all() and (got == S).any()
    env.run(shape.policy, shape.warm)
    want = compare(env, fam, C, S, need, name + ", warm-up", state_untouched=True, **kw)
    blocked, served = cc.blocked_of(want["counts"], n_cls), want["counts"][:, n_cls:].sum(axis=1)
    assert (int(blocked.min()), int(blocked.max())) == shape.blocked and (blocked > 0).any() and (served > 0).all(), (name, blocked)
    if shape.k > 8:
        assert_a_path_of_index_8_or_more_decides(shape, env, need, want)
    if name == "ring31_rmsa":  # rows of 30-hop paths that the warm-up has changed
        assert (want["paths"].reshape(env.num_envs, -1, 2)[:, env.topology.path_hops.reshape(-1) == 30, 1] < S).any()
    for _ in range(cc.AFTER_STEPS):
        env.policy_step(shape.policy, auto_reset=True, fetch=False)
    later = compare(env, fam, C, S, need, name + ", policy_steps", **kw)
    assert not np.array_equal(later["paths"], want["paths"])
    assert not (env.flags() & 2).any()
    env.check()
    env.close()


@pytest.mark.parametrize("n", [1, 3])
def test_slot_maps_left_in_global_memory_at_batch_sizes_with_a_partly_empty_workgroup(n, tmp_path):
    """germany50 RMCSA at 10 cores of 512 slots: "serviceable" runs two wavefronts per workgroup on the maps in global memory — one env
    is half a workgroup, three are one and a half — and "counts" one; "paths" stages them.  Then the layouts in alternation on
    junk-filled buffers: each keeps its own rows and zero pad columns."""
    shape = ENVELOPE_SHAPES[cc.UNSTAGED]
    env, need, C, S = make_envelope(shape, tmp_path, n=n)
    env.run(shape.policy, shape.warm)
    want = compare(env, "RMCSA", C, S, need, "%s, %d envs" % (shape.name, n), state_untouched=True, each=True)
    views = {lay: env.device_tensor(dev) for lay, dev in (("paths", "path_capacity"), ("serviceable", "serviceable"), ("counts", "capacity_counts"))}
    junk_then_alternate(env, views, want, order=("counts", "serviceable", "paths", "serviceable", "counts"))
    assert (want["paths"].reshape(n, -1, 2)[:, :, 1] < S)[want["paths"].reshape(n, -1, 2)[:, :, 0] >= 0].any()
    env.check()
    env.close()


def test_the_per_path_array_is_refused_on_a_real_batch(tmp_path):
    """star129: 129 x 129 pairs x 8 bytes of longest runs exceed a workgroup's LDS, so "serviceable" and "counts" are refused — the
    call, the queued call and the shape — with the batch left as it was, no buffer made, and "paths" still served"""
    from optical_rl_gym_amd._lib import OrlError

    shape = ENVELOPE_SHAPES["star129_rmsa"]
    env, need, C, S = make_envelope(shape, tmp_path, n=4)
    env.run(shape.policy, 200)
    snap, flags = env.get_state(), env.flags().copy()
    for call in (lambda: env.network_capacity("serviceable"), lambda: env.network_capacity("counts", fetch=False), lambda: env.network_capacity_shape("counts"),
                 lambda: env.network_capacity("counts"), lambda: env.network_capacity_shape("serviceable")):
        with pytest.raises(OrlError, match="per-path array of 129 x 129 pairs x 5 paths"):
            call()
    for dev in ("serviceable", "capacity_counts"):
        with pytest.raises(OrlError, match=r"call network_capacity\("):
            env.device_tensor(dev)
    assert np.array_equal(env.get_state(), snap) and np.array_equal(env.flags(), flags)
    assert env.network_capacity_shape("paths") == (83205, 2, 166410, 166412)
    want = compare(env, "RMSA", C, S, need, "star129 after the refusals", state_untouched=True, layouts=("paths",))
    assert (want["paths"].reshape(4, -1, 2)[:, :, 1] < S)[want["paths"].reshape(4, -1, 2)[:, :, 0] >= 0].any()
    for dev in ("serviceable", "capacity_counts"):  # (still none)
        with pytest.raises(OrlError, match=r"call network_capacity\("):
            env.device_tensor(dev)
    env.check()
    env.close()


def pending_rows(env, fam, C, need, paths, rates):
    """(L, F) of the pending pair's rows [n, K C', 2], the need of the pending class on them [n, K C'], and the pending (src, dst, class)"""
    sv = env.services()
    n, N, K = env.num_envs, env.topology.n_nodes, env.k_paths
    src, dst = sv[:, 2].astype(np.int64), sv[:, 3].astype(np.int64)
    r = np.zeros(n, np.int64) if fam == "RWA" else np.array([rates.index(int(b)) for b in sv[:, 4]], np.int64)
    cores = C if fam == "RMCSA" else 1
    rows = paths.reshape(n, N, N, K * cores, 2)[np.arange(n), src, dst]
    nd = np.repeat(need[src, dst, :, r], cores, axis=1)
    return rows, nd, src, dst, r


@pytest.mark.parametrize("name", ["rmsa_nsf_s129", "rmsa_nsf_s512", "rwa_nsf_s129", "rmcsa_c7_s64", "deep_s129_j4", "ring10c8_k9_rmsa", "k6full_k64_rwa"])
def test_consistent_with_the_existing_views_of_the_pending_service(name, tmp_path):
    """On one device state, for the pending pair and class: F of the pair's rows is column 1 of block_table(1) and L >= need exactly where
    that table lists a block (rows the service can use); the pair's "serviceable" cell is the path-level action mask's any()."""
    import optical_rl_gym_amd as orl

    if name == "deep_s129_j4":
        case = slot_agent.CASE_BY_NAME[name]
        env = orl.make("DeepRMSA", topology=slot_agent.TOPOLOGY, num_envs=24, seeds=list(range(100, 124)), **dict(case.kw, mean_service_inter_arrival_time=10.0 / 260))
        fam, C, S, pol, steps = "DeepRMSA", 1, 129, "SAP", 700
        rates = cap.class_rates("RMSA", {})
        need = cap.need_table("RMSA", env.topology, rates)
    elif name in ENVELOPE_SHAPES:  # k = 9 and k = 64: the pending pair's rows past the first eight
        shape = ENVELOPE_SHAPES[name]
        env, need, C, S = make_envelope(shape, tmp_path)
        fam, pol, steps, rates = shape.fam, shape.policy, shape.warm, cap.class_rates(shape.fam, shape.kw)
    else:
        env, fam, tab, C, S = make(name)
        need, pol, steps, rates = need_of(name), hm.HEURISTIC[fam], SHAPES[name][1], cap.class_rates(fam, config(name)[2])
    env.run(pol, steps)
    n, K = env.num_envs, env.k_paths
    paths, svc = env.network_capacity("paths"), env.network_capacity("serviceable")
    rows, nd, src, dst, r = pending_rows(env, fam, C, need, paths, rates)
    table = env.block_table(1)[0]
    usable = table[:, :, 0] > 0
    assert usable.any() and np.array_equal(table[:, :, 0][usable], nd[usable])
    assert np.array_equal(rows[:, :, 1][usable], table[:, :, 1][usable])
    assert np.array_equal((rows[:, :, 0] >= nd)[usable], (table[:, :, 3] > 0)[usable])
    assert not (usable & (rows[:, :, 0] < 0)).any()
    layout = {"RMCSA": "path_modulation", "DeepRMSA": "joint"}.get(fam, "path")
    says = env.action_mask(layout)[:, :-1].any(axis=1)
    assert env.allow_rejection
    cell = svc.reshape(n, env.topology.n_nodes ** 2, need.shape[3])[np.arange(n), src * env.topology.n_nodes + dst, r]
    # ORL_MASK_PATH of RMSA searches range(0, S - n): a service whose only room is a path's last n slots has no column there
    differ = np.flatnonzero(cell != says)
    for e in differ:
        assert fam == "RMSA" and cell[e] and not ((table[e, :, 3] > 0) & (table[e, :, 2] + nd[e] < S)).any(), (name, e)
    print(name, "pending cells", int(cell.sum()), "of", n, "differ at the last start:", len(differ))
    assert cell.any() and (name not in ("rmsa_nsf_s129", "rmcsa_c7_s64") or not cell.all())  # (on the oracle 2 and 3 of the first 8 envs are 0)
    env.close()


@pytest.mark.parametrize("name", ["rmsa_nsf_s65", "rwa_nsf_s129", "rmcsa_c7_s64"])
def test_the_view_follows_every_way_of_stepping(name):
    """After a device-resident run, policy_step, seed, set_state to an earlier snapshot and copy_envs the view equals the restatement of
    that moment: it reads the maps, not a cache."""
    env, fam, tab, C, S = make(name)
    need, pol = need_of(name), hm.HEURISTIC[fam]
    here = lambda what: compare(env, fam, C, S, need, "%s, %s" % (name, what))
    env.run(pol, SHAPES[name][1])
    early = here("run")
    snap = env.get_state()
    for _ in range(5):
        env.policy_step(pol, auto_reset=True, fetch=False)
    here("policy_step")
    env.run(pol, 60)
    later = here("second run")
    assert not np.array_equal(early["paths"], later["paths"])
    env.set_state(snap)
    back = here("set_state")
    assert all(np.array_equal(back[k], early[k]) for k in back)
    env.run(pol, 25)
    env.copy_envs(np.array([0, 0, 3]), np.array([1, 2, 4]))
    forked = here("copy_envs")["paths"]
    assert np.array_equal(forked[1], forked[0]) and np.array_equal(forked[4], forked[3])
    env.seed(np.arange(900, 900 + env.num_envs))
    here("seed")
    for _ in range(8):
        env.policy_step(pol, auto_reset=True, fetch=False)
    here("seed, stepped")
    env.check()
    env.close()


def junk_then_alternate(env, views, want, order=("counts", "paths", "serviceable", "paths", "counts")):
    """The layouts' buffers (views: layout -> device_tensor) filled with junk to their last pad column, then one call of each layout in
    alternation: every buffer holds its own rows of `want`, pad columns are 0"""
    import torch

    from optical_rl_gym_amd.envs import _RawDeviceArray

    n, flats = env.num_envs, {}
    for lay, v in views.items():
        typestr = "|u1" if lay == "serviceable" else "<i4"
        cap_items = n * env.network_capacity_shape(lay)[3]
        flats[lay] = torch.as_tensor(_RawDeviceArray({"shape": (cap_items,), "typestr": typestr, "data": (v.data_ptr(), False), "version": 2, "strides": None}),
                                     device=v.device)
    with torch.cuda.stream(env.torch_stream()):
        for f in flats.values():
            f.fill_(77)
        for lay in order:
            assert env.network_capacity(lay, fetch=False) is None
    env.sync()
    for lay, f in flats.items():
        _, _, dim, pitch = env.network_capacity_shape(lay)
        body = f.cpu().numpy().reshape(n, pitch)
        assert np.array_equal(body[:, :dim], want[lay].astype(body.dtype)), lay
        assert (body[:, dim:] == 0).all(), lay


def test_layouts_in_alternation_keep_their_own_buffers_and_pad_columns():
    """Each layout's device_array shows its own rows whatever was called since; pad columns are 0 and nothing is written past B * pitch:
    the buffers are filled with junk first."""
    import torch

    from optical_rl_gym_amd._lib import OrlError

    name = "rmsa_nsf_s512"  # three classes: 588 byte columns at a pitch of 592, 199 int32 columns at a pitch of 200
    env, fam, tab, C, S = make(name, n=9)
    need = need_of(name)
    names = {"paths": "path_capacity", "serviceable": "serviceable", "counts": "capacity_counts"}
    for dev in names.values():
        with pytest.raises(OrlError, match=r"call network_capacity\("):
            env.device_tensor(dev)
    env.run("SAP_FF", SHAPES[name][1])
    want = compare(env, fam, C, S, need, name)
    views = {lay: env.device_tensor(dev) for lay, dev in names.items()}
    assert len({v.data_ptr() for v in views.values()}) == 3
    for lay, v in views.items():
        rows, width, dim, pitch = env.network_capacity_shape(lay)
        assert v.shape == (9, dim) and v.stride() == (pitch, 1) and (dim, pitch) != (0, 0), lay
        assert v.dtype == (torch.bool if lay == "serviceable" else torch.int32)
    assert env.network_capacity_shape("serviceable")[2:] == (588, 592) and env.network_capacity_shape("counts")[2:] == (199, 200)
    junk_then_alternate(env, views, want)
    # a step, then one layout alone: the other two still show the rows of the state before
    env.policy_step("SAP_FF", auto_reset=True, fetch=False)
    env.run("SAP_FF", 40)
    fresh = cap.restate(hm.avail_of(env, 1, S), env.topology, need)
    env.network_capacity("paths", fetch=False)
    env.sync()
    assert np.array_equal(views["paths"].cpu().numpy(), fresh[0]) and not np.array_equal(fresh[0], want["paths"])
    assert np.array_equal(views["serviceable"].cpu().numpy(), want["serviceable"]) and np.array_equal(views["counts"].cpu().numpy(), want["counts"])
    out = np.empty((9, 588), np.uint8)
    assert env.network_capacity("serviceable", out=out).dtype == np.bool_ and np.array_equal(out.view(np.bool_), fresh[1])
    with pytest.raises(ValueError):
        env.network_capacity("counts", out=out)
    env.close()


@pytest.mark.parametrize("name", ["rmsa_nsf_s65", "rmcsa_c7_s64"])
def test_views_and_steps_captured_in_one_graph(name):
    """{step(None, fetch=False); network_capacity(layout, fetch=False) x 3} captured on the batch's stream after a first pass outside the
    capture (which allocates the buffers and, RMCSA, builds the need table) and replayed: the tensors are the restatement of the state
    after the last replay; no flag is raised."""
    import torch

    env, fam, tab, C, S = make(name, n=40)
    need, pol = need_of(name), hm.HEURISTIC[fam]
    env.run(pol, SHAPES[name][1])
    s = env.torch_stream()

    def chain(e):
        e.step(None, auto_reset=True, fetch=False)
        for lay in ("paths", "serviceable", "counts"):
            e.network_capacity(lay, fetch=False)

    env.policy(pol)  # the action every replay steps: accepted at first, refused once its slots are taken
    with torch.cuda.stream(s):
        chain(env)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=s):
        chain(env)
    torch.cuda.synchronize()
    for _ in range(12):
        g.replay()
    torch.cuda.synchronize()
    want = cap.restate(hm.avail_of(env, C, S), env.topology, need)
    for lay, dev, w in zip(("paths", "serviceable", "counts"), ("path_capacity", "serviceable", "capacity_counts"), want):
        assert np.array_equal(env.device_tensor(dev).cpu().numpy(), w), (name, lay)
    assert not (env.flags() & 2).any()
    env.check()
    env.close()


def test_two_shards_on_one_device():
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd.sharding import MultiDeviceBatch

    name, n, cut = "rmsa_nsf_s65", 40, 13
    whole = make(name, n=n)[0]
    fam, topo, kw, S = config(name)
    seeds = [hm.SEED0 + e for e in range(n)]
    mk = lambda sd: orl.make(fam, topology=topo, num_envs=len(sd), seeds=sd, **kw)
    multi = MultiDeviceBatch.from_shards([mk(seeds[:cut]), mk(seeds[cut:])])
    for _ in range(150):
        a = whole.policy("SAP_FF")
        whole.step(a, auto_reset=True)
        multi.step(a, auto_reset=True)
    want = compare(whole, fam, 1, S, need_of(name), "unsharded")
    for lay in ("paths", "serviceable", "counts"):
        assert multi.network_capacity_shape(lay) == whole.network_capacity_shape(lay)
        got = multi.network_capacity(lay)
        assert got.dtype == want[lay].dtype and np.array_equal(got, want[lay]), lay
        assert multi.network_capacity(lay, fetch=False) is None
    assert (want["counts"][:, :76] > 0).any()
    multi.close()
    whole.close()


def test_the_one_env_facades_return_the_reshaped_arrays():
    import optical_rl_gym_amd as orl

    topo = slot_agent.topology()
    N, K = topo.n_nodes, topo.k_paths
    for cls, fam, kw, C, S in ((orl.RMSAEnv, "RMSA", dict(num_spectrum_resources=65, load=200), 1, 65),
                               (orl.DeepRMSAEnv, "RMSA", dict(num_spectrum_resources=65, mean_service_holding_time=10.0, mean_service_inter_arrival_time=0.05), 1, 65),
                               (orl.RWAEnv, "RWA", dict(num_spectrum_resources=64, load=400), 1, 64),
                               (orl.RMCSAEnv, "RMCSA", dict(slot_agent.CASE_BY_NAME["rmcsa_c7_s64"].kw), 7, 64)):
        one = cls(topology=slot_agent.TOPOLOGY, seed=3, **kw)
        one.reset()
        one.batch.run(one.POLICY_SAP if hasattr(one, "POLICY_SAP") else "SAP_FF", 200)
        tab = slot_agent.rmcsa_tables("rmcsa_c7_s64") if fam == "RMCSA" else None
        need = cap.need_table(fam, topo, cap.class_rates(fam, kw), tab)
        n_cls = need.shape[3]
        paths, svc, counts = cap.restate(hm.avail_of(one.batch, C, S), topo, need)
        P, M, (blocked, classes) = one.network_capacity("paths"), one.network_capacity("serviceable"), one.network_capacity("counts")
        assert P.shape == (N, N, K, C, 2) and P.dtype == np.int32 and np.array_equal(P.ravel(), paths[0]), cls
        assert M.shape == (N, N, n_cls) and M.dtype == np.bool_ and np.array_equal(M.ravel(), svc[0]), cls
        assert blocked.shape == (n_cls,) and classes.shape == (N, N) and np.array_equal(np.concatenate([blocked, classes.ravel()]), counts[0]), cls
        assert (P[..., 1] < S)[P[..., 0] >= 0].any(), cls
        with pytest.raises(ValueError, match="layout must be one of"):
            one.network_capacity("cells")
        one.close()


def test_refusals_leave_the_batch_as_it_was():
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd._lib import OrlError

    qos = orl.make("QoSConstrainedRA", topology=slot_agent.TOPOLOGY, num_envs=16, seeds=list(range(16)), load=10)
    snap, flags = qos.get_state(), qos.flags().copy()
    for call in (lambda: qos.network_capacity(), lambda: qos.network_capacity("counts", fetch=False), lambda: qos.network_capacity_shape("serviceable")):
        with pytest.raises(OrlError, match="QoSConstrainedRA"):
            call()
    for dev in ("path_capacity", "serviceable", "capacity_counts"):
        with pytest.raises(OrlError, match=r"call network_capacity\("):
            qos.device_tensor(dev)
    assert np.array_equal(qos.get_state(), snap) and np.array_equal(qos.flags(), flags)
    qos.close()
    env = make("rmcsa_c7_s64")[0]
    env.run("SAP_BM_FC_FF", 30)
    snap = env.get_state()
    for layout in (3, -1, 17):
        assert env.lib.orl_batch_network_capacity(env._h, layout, None) != 0, layout  # (ORL_E_INVALID, past the Python-side check)
        with pytest.raises(OrlError, match="unknown network-capacity layout"):
            env.network_capacity(layout)
    with pytest.raises(ValueError, match="layout must be one of"):
        env.network_capacity("cells")
    for dev in ("path_capacity", "serviceable", "capacity_counts"):  # nothing was queued, no buffer exists
        with pytest.raises(OrlError, match=r"call network_capacity\("):
            env.device_tensor(dev)
    assert np.array_equal(env.get_state(), snap)
    env.network_capacity("counts", fetch=False)  # one layout's first call allocates that layout's buffer alone
    env.sync()
    assert env.device_tensor("capacity_counts").shape == (24, 76 + 196)
    with pytest.raises(OrlError, match=r"call network_capacity\("):
        env.device_tensor("serviceable")
    env.close()
