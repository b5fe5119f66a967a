"""Core and spectrum rules with a (path, core) table for RMCSA on the device (include/orl.h, orl_batch_route_cores; k_route_cores in
csrc/orl_route_cores.h) against the plain-Python restatement (tests/route_cores_restate.py, pinned to brute force, to the completion's
restatement and to the oracle's step in tests/test_route_cores.py): every env, every rule x route, each path's best and one fixed
modulation, every source of the prefix, against the completion kernel, against the oracle step by step, under graph capture, over a
sharded batch, and the refusals."""
import numpy as np
import pytest

from tests import envelope
from tests import rmcsa_mask_restate as rr
from tests import route_cores_cases as cc
from tests import route_cores_restate as rc
from tests import slot_agent
from tests.test_rmcsa_complete_gpu import _agent_steps, _make, _state, crowd, set_maps

pytestmark = pytest.mark.gpu

TOPOLOGY = slot_agent.TOPOLOGY
K, M = 5, 6
# the shapes of tests/test_rmcsa_complete_gpu.py, the smallest at which the kernel can go wrong: case -> envs
SLOT_SHAPES = {"rmcsa_c7_s64": 512,   # W = 1: the last bit of the word
               "rmcsa_c7_s65": 512,   # W = 2: one slot in the second word; every env restated
               "rmcsa_c3_s128": 24,   # worst_xt = -54.8: the crosstalk limit binds
               "rmcsa_c2_s129": 20,   # W = 5, 20 envs: the third group of 8 is half empty
               "rmcsa_c31_s64": 24,   # 155 (path, core) pairs: 20 chunks of 8
               "rmcsa_c2_s512": 24}   # W = 8, discrete rates (40, 100, 400): services of up to 33 slots
# of tests/envelope.py, warmed with run("SAP_BM_FC_FF", warm): one core (chunks hold 5 pairs), S = 12 at load 600 (maps that fill by
# themselves), 8 envs (one group)
ENVELOPE_SHAPES = ("rmcsa_c1", "rmcsa_c17", "rmcsa_hiocc")
SHAPES = tuple(SLOT_SHAPES) + ENVELOPE_SHAPES
POINTS = ("construction", "walk", "crowded", "crafted", "reset")
ALL_ENVS = "rmcsa_c7_s65"  # the 512-env shape restated on every env; the other one on its first 64
SMALL = tuple(n for n in SHAPES if (SLOT_SHAPES.get(n) or envelope.CASE_BY_NAME[n].batch) <= 24)


def _open(name, **extra):
    """(env, seeds, oracle kwargs, topology name) of a shape"""
    import optical_rl_gym_amd as orl

    if name in SLOT_SHAPES:
        n = SLOT_SHAPES[name]
        kw = slot_agent.CASE_BY_NAME[name].kw
        return _make(kw, n, **extra), list(range(1000, 1000 + n)), kw, TOPOLOGY
    case = envelope.CASE_BY_NAME[name]
    assert case.batch <= 64 and case.topo in envelope.SHIPPED
    seeds = envelope.seeds_of(case)
    return (orl.make("RMCSA", topology=case.topo, num_envs=len(seeds), seeds=seeds, **dict(case.kw, **extra)), seeds, envelope.oracle_kwargs(case),
            case.topo)


def _advance(env, name, tab):
    if name in SLOT_SHAPES:
        _agent_steps(env, tab, 30, np.random.RandomState(env.num_spectrum_resources))
        env.run("SAP_BM_FC_FF", 60)
    else:
        env.run("SAP_BM_FC_FF", envelope.CASE_BY_NAME[name].warm)


def _rows(name, env):
    return env.num_envs if env.num_envs <= 64 or name == ALL_ENVS else 64


def _differ(what, got, want):
    bad = np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))
    assert len(bad) == 0, "%s: %d envs differ, first %d: got %r, want %r" % (what, len(bad), bad[0], got[bad[0]], want[bad[0]])


def _check(name, env, tab, what, seen):
    """Every restated env of the present state: every rule x route under each path's best and one fixed modulation, fetched and in
    place; the prefixes from the host and from the actions buffer; device against device.  State and flags stay as they are."""
    import torch

    n, cn = env.num_envs, _rows(name, env)
    C, S = env.num_spatial_resources, env.num_spectrum_resources
    topo = env.topology
    snap, flags = env.get_state(), env.flags().copy()
    avail, services = _state(env)
    avail, services = avail[:cn], services[:cn]
    pv = rr.prov_all(avail, services, topo, tab)
    assert env.core_table_shape() == (K * C, 4, 4 * K * C)
    env.route_cores(fetch=False)  # (the first call allocates the table)
    acts, tabt = env.device_tensor("actions"), env.device_tensor("core_table")
    assert tuple(tabt.shape) == (n, 4 * K * C) and tabt.dtype == torch.int32
    stream = env.torch_stream()
    reject = np.array([K, M, C, S])
    fixed = cc.fixed_modulation(services, topo, tab)
    combo = 0
    for mod in (None, fixed):
        prep = rc.Prepared(avail, services, topo, tab, mod, pv)
        if mod is None:
            rc.count_kinds(prep, seen)
        for rule in rc.RULES:
            want_tab = rc.table(prep, rule)
            for route in rc.ROUTES:
                tag = "%s, %s + %s, modulation %r" % (what, rule, route, mod)
                want = rc.route(prep, want_tab, route)
                got, gtab = env.route_cores(rule, route, modulation=mod, table=True)
                assert got.shape == (n, 4) and got.dtype == np.int32 and gtab.shape == (n, K * C, 4) and gtab.dtype == np.int32
                _differ(tag, got[:cn], want)
                _differ(tag + " (table)", gtab[:cn], want_tab)
                with torch.cuda.stream(stream):
                    acts.fill_(-7)
                    tabt.fill_(-7)
                    assert env.route_cores(rule, route, modulation=mod, fetch=False) is None
                env.sync()
                assert np.array_equal(acts.cpu().numpy(), got) and np.array_equal(tabt.cpu().numpy().reshape(n, K * C, 4), gtab), tag
                # a prefix of one and of two columns, out-of-range and negative entries drawn by env index: from the host, and from
                # columns 0 and 2 of the actions buffer; the table stays complete
                for g in (1, 2):
                    combo += 1
                    if combo % 5:
                        continue
                    given = cc.draw_given(n, K, C, g, shift=combo)
                    want_g = rc.route(prep, want_tab, route, given[:cn])
                    got_g, gtab_g = env.route_cores(rule, route, paths=given[:, 0], cores=given[:, 1] if g == 2 else None, modulation=mod, table=True)
                    _differ(tag + ", host prefix %d" % g, got_g[:cn], want_g)
                    assert np.array_equal(gtab_g, gtab), tag
                    junk = np.full((n, 4), -9, np.int32)
                    junk[:, 0] = given[:, 0]
                    junk[:, 2] = given[:, 1] if g == 2 else C + 3
                    with torch.cuda.stream(stream):
                        acts.copy_(torch.as_tensor(junk, device=acts.device))
                        tabt.fill_(-7)
                        env.route_cores(rule, route, n_given=g, modulation=mod, fetch=False)
                    env.sync()
                    assert np.array_equal(acts.cpu().numpy(), got_g) and np.array_equal(tabt.cpu().numpy().reshape(n, K * C, 4), gtab), tag
                    seen["prefix_reject"] = seen.get("prefix_reject", 0) + int((got_g[:cn] == reject).all(axis=1).sum())
                    seen["prefix_found"] = seen.get("prefix_found", 0) + int((~(got_g[:cn] == reject).all(axis=1)).sum())
    # device against device
    paths, pairs = cc.draw_given(n, K, C, 1, shift=3), cc.draw_given(n, K, C, 2, shift=5)
    assert np.array_equal(env.route_cores("first", "ksp"), env.complete_actions(n_given=0)), what
    assert np.array_equal(env.route_cores("first", "ksp", paths=paths[:, 0]), env.complete_actions(given=paths, n_given=1)), what
    triple = np.stack([pairs[:, 0], np.full(n, fixed, np.int32), pairs[:, 1]], axis=1).astype(np.int32)
    assert np.array_equal(env.route_cores("first", "ksp", paths=pairs[:, 0], cores=pairs[:, 1], modulation=fixed), env.complete_actions(given=triple, n_given=3)), what
    for rule in rc.RULES:
        best, tab_d = env.route_cores(rule, "best", table=True)
        one = env.route_cores(rule, "ksp", paths=pairs[:, 0], cores=pairs[:, 1])
        idx = tab_d[:, :, 1].argmin(axis=1)  # (the first of equal minima: the lowest pair)
        for i in range(n):
            p, c = int(pairs[i, 0]), int(pairs[i, 1])
            row = tab_d[i, p * C + c] if 0 <= p < K and 0 <= c < C else np.array([S, rc.NO_FIT, 0, 0])
            if row[1] == rc.NO_FIT:
                assert tuple(one[i]) == tuple(reject) and row[0] == S, (what, rule, i)
            else:
                assert (one[i, 0], one[i, 2], one[i, 3]) == (p, c, row[0]), (what, rule, i)
            q = int(idx[i])
            if tab_d[i, q, 1] == rc.NO_FIT:
                assert tuple(best[i]) == tuple(reject), (what, rule, i)
            else:
                assert (best[i, 0], best[i, 2], best[i, 3]) == (q // C, q % C, tab_d[i, q, 0]), (what, rule, i)
    assert np.array_equal(env.get_state(), snap) and np.array_equal(env.flags(), flags), what


@pytest.mark.parametrize("point", POINTS)
@pytest.mark.parametrize("name", SHAPES)
def test_actions_and_table_equal_the_restatement(name, point):
    """After construction, after the walk, on crowded and on crafted maps set through a snapshot, and after a full reset."""
    env = _open(name)[0]
    if name in SLOT_SHAPES:
        assert env.lib.orl_batch_row_words(env._h) == {64: 1, 65: 2, 128: 2, 129: 5, 512: 8}[env.num_spectrum_resources]
    tab = rr.tables_of(env)
    seen = {}
    if point != "construction":
        _advance(env, name, tab)
    if point in ("crowded", "crafted"):
        snap = env.get_state()
        avail, services = _state(env)
        maps = (crowd if point == "crowded" else cc.craft)(avail, services, env.topology, tab)
        set_maps(env, snap, maps)
        assert np.array_equal(_state(env)[0], maps)
    if point == "reset":
        env.reset(full=True)
    _check(name, env, tab, "%s, %s" % (name, point), seen)
    print(name, point, seen)
    assert seen["prefix_found"] > 0 and seen["prefix_reject"] > 0
    if point in ("crowded", "crafted"):
        env.set_state(snap)
    assert not (env.flags() & 2).any()
    env.check()
    env.close()


@pytest.mark.parametrize("name", SMALL)
def test_route_cores_then_step_against_the_oracle(name):
    """route_cores(fetch=False); step(None) for 60 steps, rule and route changing per step, against an oracle stepped with the restated
    action: reward, done, counters, maps and services."""
    from oracle.oracle import OracleBatch

    env, seeds, kw, topo_name = _open(name)
    ora = OracleBatch("RMCSA", topo_name, seeds, **kw)
    tab = rr.tables_of(env)
    accepted = 0
    for t in range(60):
        rule, route = rc.RULES[t % 5], rc.ROUTES[(t // 5 + t) % 5]
        avail, services = _state(env)
        prep = rc.Prepared(avail, services, env.topology, tab)
        want = rc.route(prep, rc.table(prep, rule), route)
        assert env.route_cores(rule, route, fetch=False) is None
        _, rew, done, _ = env.step(None, auto_reset=True)
        _, rew_o, done_o, _ = ora.step(want, auto_reset=True)
        tag = (name, t, rule, route)
        assert np.array_equal(env.device_tensor("actions").cpu().numpy(), want), tag
        assert np.array_equal(rew, rew_o) and np.array_equal(np.asarray(done, bool), np.asarray(done_o, bool)), tag
        assert np.array_equal(env.counters(), ora.counters()) and np.array_equal(env.services(), ora.services()), tag
        assert np.array_equal(_state(env)[0], rr.unpack_cores(ora.slots_packed(), ora.C, ora.E, ora.S)), tag
        accepted += int((want[:, 0] < K).sum())
    assert accepted > 0 and not (env.flags() & 2).any()
    env.check()
    env.close()


def test_route_cores_and_step_captured_in_one_graph():
    """{route_cores; step} captured on the batch's stream after a first call outside the capture, replayed 20 times against an eager
    twin and the restatement."""
    import torch

    name = "rmcsa_c2_s129"
    env, twin = _open(name)[0], _open(name)[0]
    tab = rr.tables_of(env)
    env.run("SAP_BM_FC_FF", 40)
    twin.set_state(env.get_state())  # (two batches agree on a snapshot's never-written bytes only when one was copied from the other)
    s = env.torch_stream()
    rule, route = "best", "ksp_least_loaded_core"

    def eager():
        twin.route_cores(rule, route, fetch=False)
        twin.step(None, auto_reset=True, fetch=False)
        twin.sync()

    with torch.cuda.stream(s):
        env.route_cores(rule, route, fetch=False)
        env.step(None, auto_reset=True, fetch=False)
    eager()
    torch.cuda.synchronize()
    assert np.array_equal(env.get_state(), twin.get_state())
    g = torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=s):
        env.route_cores(rule, route, fetch=False)
        env.step(None, auto_reset=True, fetch=False)
    torch.cuda.synchronize()
    eager()  # (the capture ran nothing; the twin takes the step the first replay takes)
    for it in range(20):
        avail, services = _state(env)
        prep = rc.Prepared(avail, services, env.topology, tab)
        want = rc.route(prep, rc.table(prep, rule), route)
        g.replay()
        torch.cuda.synchronize()
        if it:
            eager()
        assert np.array_equal(env.device_tensor("actions").cpu().numpy(), want), it
        assert np.array_equal(env.device_tensor("actions").cpu().numpy(), twin.device_tensor("actions").cpu().numpy()), it
        assert np.array_equal(env.device_tensor("core_table").cpu().numpy(), twin.device_tensor("core_table").cpu().numpy()), it
        assert np.array_equal(env.device_tensor("reward").cpu().numpy(), twin.device_tensor("reward").cpu().numpy()), it
        assert np.array_equal(env.get_state(), twin.get_state()), it
    for e in (env, twin):
        assert not (e.flags() & 2).any()
        e.check()
        e.close()


def test_two_shards_equal_the_unsharded_batch():
    from optical_rl_gym_amd.sharding import MultiDeviceBatch

    case = slot_agent.CASE_BY_NAME["rmcsa_c7_s65"]
    n, cut = 200, 72
    seeds = list(range(40, 40 + n))
    whole = _make(case.kw, n, seeds=seeds)
    multi = MultiDeviceBatch.from_shards([_make(case.kw, cut, seeds=seeds[:cut]), _make(case.kw, n - cut, seeds=seeds[cut:])])
    for t in range(20):
        acts = whole.policy("SAP_BM_FC_FF").copy()
        whole.step(acts, auto_reset=True)
        multi.step(acts, auto_reset=True)
    assert multi.core_table_shape() == whole.core_table_shape() == (K * 7, 4, 4 * K * 7)
    pairs = cc.draw_given(n, K, 7, 2)
    for rule, route, mod in (("first", "ksp", None), ("min_cuts", "best", None), ("exact", "ksp_best_core", 1), ("last", "least_loaded", 3)):
        for kw in (dict(), dict(paths=pairs[:, 0]), dict(paths=pairs[:, 0], cores=pairs[:, 1])):
            a, t = whole.route_cores(rule, route, modulation=mod, table=True, **kw)
            b, u = multi.route_cores(rule, route, modulation=mod, table=True, **kw)
            assert np.array_equal(a, b) and np.array_equal(t, u), (rule, route, mod, sorted(kw))
            assert np.array_equal(multi.route_cores(rule, route, modulation=mod, **kw), a)
            assert multi.route_cores(rule, route, modulation=mod, fetch=False, **kw) is None
            for s in multi.shards:
                s.sync()
            assert np.array_equal(np.concatenate([s.device_tensor("actions").cpu().numpy() for s in multi.shards]), a)
    with pytest.raises(ValueError):
        multi.route_cores(paths=pairs[:cut, 0])
    multi.close()
    whole.close()


@pytest.mark.parametrize("fam,kw", [("RMSA", dict(load=100, mean_service_holding_time=25, episode_length=100, num_spectrum_resources=64)),
                                    ("DeepRMSA", dict(mean_service_holding_time=7.5, mean_service_inter_arrival_time=1.0 / 12.0, j=2, episode_length=50)),
                                    ("RWA", dict(load=450, mean_service_holding_time=25, episode_length=1000, allow_rejection=True)),
                                    ("QoSConstrainedRA", dict(load=10))])
def test_other_families_refuse_the_call(fam, kw):
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd._lib import OrlError

    env = orl.make(fam, topology=TOPOLOGY, num_envs=16, seeds=list(range(16)), **kw)
    snap = env.get_state()
    acts = env.device_tensor("actions").cpu().numpy().copy()
    for fetch in (True, False):
        for rule in rc.RULES:
            with pytest.raises(OrlError, match="RMCSA only"):
                env.route_cores(rule, "best", fetch=fetch)
        with pytest.raises(OrlError, match="RMCSA only"):
            env.route_cores(paths=np.zeros(16, np.int32), fetch=fetch, table=True)
    with pytest.raises(OrlError, match="RMCSA only"):
        env.core_table_shape()
    with pytest.raises(OrlError, match="route_cores"):
        env.device_tensor("core_table")  # nothing was allocated
    env.sync()
    assert np.array_equal(env.get_state(), snap) and np.array_equal(env.device_tensor("actions").cpu().numpy(), acts)  # nothing was queued
    env.close()


def test_arguments_are_checked():
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd._lib import OrlError

    env = _make(dict(load=100, num_spectrum_resources=64, num_spatial_resources=7), 16)
    with pytest.raises(OrlError, match="route_cores"):
        env.device_tensor("core_table")
    env.complete_actions(n_given=0)
    acts = env.device_tensor("actions").cpu().numpy().copy()
    ok = np.zeros(16, np.int32)
    for fetch in (True, False):
        for rule in (4, 5):
            with pytest.raises(OrlError, match="byte counters"):
                env.route_cores(rule, "ksp", fetch=fetch)
        for rule in (7, -1):
            with pytest.raises(OrlError, match="unknown spectrum-assignment rule"):
                env.route_cores(rule, "ksp", fetch=fetch)
        for route in (-1, 5):
            with pytest.raises(OrlError, match="unknown route"):
                env.route_cores("first", route, fetch=fetch)
        for mod in (M, -2):
            with pytest.raises(OrlError, match="modulation"):
                env.route_cores(modulation=mod, fetch=fetch)
        for g in (3, -1):
            with pytest.raises(OrlError, match="outside 0 .. 2"):
                env.route_cores(n_given=g, fetch=fetch)
        with pytest.raises(OrlError, match="n_given == 0"):
            env.route_cores(paths=ok, n_given=0, fetch=fetch)
    env.sync()
    assert np.array_equal(env.device_tensor("actions").cpu().numpy(), acts)  # nothing was queued
    with pytest.raises(OrlError, match="route_cores"):
        env.device_tensor("core_table")  # and nothing allocated
    # unknown names and bad prefixes are Python's to refuse
    for bad in (dict(rule="most_used"), dict(rule="least_used"), dict(rule="worst"), dict(route="shortest"), dict(cores=ok), dict(paths=ok[:15]),
                dict(paths=ok, cores=ok[:15]), dict(paths=ok.astype(np.float64)), dict(paths=ok, cores=ok, n_given=1)):
        with pytest.raises(ValueError):
            env.route_cores(**bad)
    a, t = env.route_cores(table=True)
    assert a.shape == (16, 4) and t.shape == (16, K * 7, 4) and tuple(env.device_tensor("core_table").shape) == (16, 4 * K * 7)
    env.close()
    one = orl.RMCSAEnv(topology=TOPOLOGY, seed=3, load=100, num_spectrum_resources=64, num_spatial_resources=7)
    one.reset()
    for rule, route in (("first", "ksp"), ("best", "best"), ("min_cuts", "ksp_least_loaded_core")):
        full = one.route_cores(rule, route)
        assert isinstance(full, tuple) and len(full) == 4 and all(isinstance(v, int) for v in full)
        assert full == tuple(int(v) for v in one.batch.route_cores(rule, route)[0])
    assert one.route_cores("first", "ksp") == one.complete_action()
    full = one.route_cores("first", "ksp")
    if full != (K, M, 7, 64):
        assert one.route_cores("first", "ksp", path=full[0]) == full and one.route_cores("first", "ksp", path=full[0], core=full[2]) == full
    assert one.route_cores(path=K) == (K, M, 7, 64) and one.route_cores(path=0, core=7) == (K, M, 7, 64)
    with pytest.raises(ValueError):
        one.route_cores(core=0)
    one.close()
