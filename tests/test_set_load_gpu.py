"""Per-env traffic load and set_load on the GPU.  Construction with one load per env against one oracle batch per load; set_load
against traces of the reference's own set_load (tests/golden/s1_*.npz, tools/gen_golden_set_load.py).  Every comparison is ==
on integers and float64."""

import numpy as np
import pytest

from tests.helpers import S1, _replay_with_schedule, _schedule, crc_slots, load_golden
from tests.test_gpu_parity import DEVICE_PAIRS, _exact, _need_devices, _ran_pair_form, force_impl

pytestmark = pytest.mark.gpu


def event_capacity_for(load):
    """The library's own sizing of the pending-release arrays (include/orl.h, event_capacity == 0)."""
    return int(load + 10.0 * np.sqrt(load) + 64.0)


def _max_load(g):
    """The largest load the trace reaches (initial kwargs, then set_load's rule per change)."""
    kw = g["meta"]["kwargs"]
    mht = kw["mean_service_holding_time"]
    load = kw["load"] if "load" in kw else mht / kw["mean_service_inter_arrival_time"]
    top = load
    for t, ch in sorted(_schedule(g).items()):
        load = ch.get("load", load)
        top = max(top, load)
    return top


def _product(g, num_envs=1, seeds=None, **extra):
    import optical_rl_gym_amd as orl

    kw = dict(g["meta"]["kwargs"])
    seed = kw.pop("seed")
    kw.update(extra)
    return orl.make(g["meta"]["env"], topology=g["meta"]["topology"], num_envs=num_envs, seeds=[seed] * num_envs if seeds is None else seeds,
                    **kw)


# ---- 1. sweep at construction: every family, every step form --------------------------------------------------------------
SWEEP = {
    "RMSA": (dict(mean_service_holding_time=25, episode_length=100, num_spectrum_resources=320, allow_rejection=True), [100, 400, 250, 175], "SAP_FF"),
    "DeepRMSA": (dict(j=1, episode_length=50), [60, 140, 90, 110], "SAP"),
    "RWA": (dict(mean_service_holding_time=25, episode_length=200, allow_rejection=True), [200, 600, 450, 300], "SAP_FF"),
    "RMCSA": (dict(mean_service_holding_time=25, episode_length=100, num_spectrum_resources=64, num_spatial_resources=7, worst_xt=-84.7,
                   allow_rejection=True), [120, 400, 250, 180], "SAP_BM_FC_FF"),
    "QoSConstrainedRA": (dict(mean_service_holding_time=25, episode_length=200, num_spectrum_resources=40, num_service_classes=3,
                              classes_arrival_probabilities=[0.2, 0.5, 0.3], classes_reward=[10.0, 2.0, 1.0], allow_rejection=True),
                         [500, 1400, 1000, 700], "SAP_FF"),
}


def _sweep_batches(fam, per_env_mht=False, omp=False, n_seeds=8, loads=None, kw=None, topo="nsfnet_chen", **dev_extra):
    """A device batch of len(loads) x n_seeds envs with the loads interleaved over the env index, and one oracle batch per load
    holding that load's envs; returns (dev, [(env indices, oracle)])."""
    import optical_rl_gym_amd as orl
    from oracle.oracle import OracleBatch

    kw0, loads0, _pol = SWEEP[fam]
    kw = dict(kw0 if kw is None else kw)
    loads = loads0 if loads is None else loads
    L = len(loads)
    n = L * n_seeds
    seeds = [100 + i for i in range(n)]
    env_load = [loads[i % L] for i in range(n)]
    mhts = [25.0, 10.0, 40.0, 7.5]
    env_mht = [mhts[i % L] for i in range(n)] if per_env_mht else None
    if fam == "DeepRMSA":  # its constructor takes the two means: load = holding time / inter-arrival time (deeprmsa_env.py:25)
        h = env_mht if per_env_mht else [7.5] * n
        args = dict(mean_service_holding_time=h if per_env_mht else 7.5, mean_service_inter_arrival_time=[h[i] / env_load[i] for i in range(n)])
    else:
        args = dict(load=env_load)
        if per_env_mht:
            kw.pop("mean_service_holding_time")
            args["mean_service_holding_time"] = env_mht
    dev = orl.make(fam, topology=topo, num_envs=n, seeds=seeds, **kw, **args, **dev_extra)
    oracles = []
    for li in range(L):
        idx = list(range(li, n, L))
        okw = dict(kw)
        if fam == "DeepRMSA":
            h = mhts[li] if per_env_mht else 7.5
            okw.update(mean_service_holding_time=h, mean_service_inter_arrival_time=h / loads[li])
        else:
            okw["load"] = loads[li]
            if per_env_mht:
                okw["mean_service_holding_time"] = mhts[li]
        oracles.append((idx, OracleBatch(fam, topo, [seeds[i] for i in idx], omp=omp, **okw)))
    return dev, oracles


def _compare_all(tag, dev, oracles, qos=False):
    chk = _exact(tag)
    d_cnt, d_svc, d_act = dev.counters(), dev.services(), dev.active()
    d_ls = None if qos else dev.link_stats_all()
    d_ns = None if qos else dev.net_stats_all()
    d_sl = None if qos else dev.slots_packed()
    for idx, ora in oracles:
        chk(idx[0], "counters", d_cnt[idx], ora.counters())
        chk(idx[0], "services", d_svc[idx], ora.services())
        chk(idx[0], "active", d_act[idx], ora.active())
        if qos:
            for k, i in enumerate(idx):
                chk(i, "spectrum", dev.spectrum(i), ora.spectrum(k))
                chk(i, "link statistics", dev.link_stats(i)[[0, 3]], ora.link_stats(k)[[0, 3]])
        else:
            chk(idx[0], "slot maps", d_sl[idx], ora.slots_packed())
            chk(idx[0], "link statistics", d_ls[idx], ora.link_stats_all())
            chk(idx[0], "network statistics", d_ns[idx], ora.net_stats_all())
    assert not dev.flags().any()


@pytest.mark.parametrize("form", ["run", "run_wave64", "agent1", "agent0", "run_alt"])
@pytest.mark.parametrize("fam,per_env_mht", [("RMSA", False), ("RMSA", True), ("DeepRMSA", False), ("RWA", False), ("RMCSA", False),
                                             ("QoSConstrainedRA", False)])
def test_sweep_at_construction_matches_one_oracle_per_load(fam, per_env_mht, form, monkeypatch):
    from optical_rl_gym_amd import _lib

    qos = fam == "QoSConstrainedRA"
    for k in ("ORL_STEP_IMPL", "ORL_PERSIST", "ORL_AGENT_STEP", "ORL_LIB_VARIANT", "ORL_PERSIST_VARIANT", "ORL_PERSIST_RW"):
        monkeypatch.delenv(k, raising=False)
    if form == "run_wave64":
        monkeypatch.setenv("ORL_STEP_IMPL", "64")
    elif form == "agent1":
        monkeypatch.setenv("ORL_AGENT_STEP", "1")
    elif form == "agent0":
        monkeypatch.setenv("ORL_AGENT_STEP", "0")
    elif form == "run_alt":
        if qos:
            pytest.skip("no persistent kernel serves this family: nothing the two-kernel form would replace")
        if not _lib.lib().orl_build_has_alt() and not _lib.lib("alt").orl_build_has_alt():
            pytest.skip("the two-kernel library is not built")
        force_impl(monkeypatch, "split2")
    policy = SWEEP[fam][2]
    dev, oracles = _sweep_batches(fam, per_env_mht)
    assert isinstance(dev.load, np.ndarray) and dev.load.shape == (dev.num_envs,)
    if form.startswith("run"):
        dev.run(policy, 600)
        for _idx, ora in oracles:
            ora.run(policy, 600)
    else:
        assert int(dev.lib.orl_batch_debug_step_kernel(dev._h)) == (2 if form == "agent1" else 0)
        for _t in range(200):
            dev.policy_step(policy, auto_reset=True, fetch=False)
        dev.check()
        for _idx, ora in oracles:
            ora.run(policy, 200)
    _compare_all("%s %s" % (fam, form), dev, oracles, qos=qos)
    dev.close()


# ---- 2. sweep at size --------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(1800)
@pytest.mark.parametrize("n_seeds,pair", [(1024, False), (256, True)])
def test_sweep_at_size_every_env_matches_oracle(n_seeds, pair):
    """cfg2 with 16 loads from 100 to 400 Erlang interleaved over the env index: 16 384 envs under the specialised persistent kernel
    and 4 096 envs under its two-wavefront form, every env against the OpenMP oracle of its load."""
    from bench import WORKLOADS

    fam, topo, kw, policy = WORKLOADS["cfg2"]
    kw = dict(kw, episode_length=100)
    kw.pop("load")
    loads = [100.0 + 20.0 * i for i in range(16)]
    dev, oracles = _sweep_batches(fam, omp=True, n_seeds=n_seeds, loads=loads, kw=kw, topo=topo)
    assert dev.specialised
    dev.run(policy, 300)
    assert int(dev.lib.orl_batch_debug_persist_spec(dev._h)) == (2 if pair else 1)
    assert _ran_pair_form(dev) == pair
    for _idx, ora in oracles:
        ora.run(policy, 300)
    _compare_all("cfg2 sweep %d" % dev.num_envs, dev, oracles)
    la, lh = dev.rates()
    assert np.array_equal(la, dev._rate_arrays[0]) and np.array_equal(lh, dev._rate_arrays[1])
    dev.close()


# ---- 3. set_load against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("agent", ["0", "1"])
@pytest.mark.parametrize("fam", sorted(S1))
def test_set_load_reproduces_the_reference_trace(fam, agent, monkeypatch):
    monkeypatch.setenv("ORL_AGENT_STEP", agent)
    g = load_golden(S1[fam])
    env = _product(g, event_capacity=event_capacity_for(_max_load(g)))
    assert int(env.lib.orl_batch_debug_step_kernel(env._h)) == (2 if agent == "1" else 0)
    _replay_with_schedule(env, g, _exact(S1[fam]))
    after = g["after_change"][-1]
    assert env.load == after[1] and env.mean_service_holding_time == after[2] and env.mean_service_inter_arrival_time == after[3]
    la, lh = env.rates()
    assert la[0] == 1 / after[3] and lh[0] == 1 / after[2]
    assert not env.flags().any()
    env.close()


@pytest.mark.parametrize("per_env", [False, True])
def test_set_load_between_device_resident_runs(per_env):
    """The RMSA trace through run() in segments between the scheduled steps and the snapshots (the persistent kernel): a 1-env
    batch (one pair for the batch: the kernels divide by scalars) and 8 envs of the same seed built with a load per env (the
    kernels read every env's pair), first and last env compared."""
    g = load_golden(S1["RMSA"])
    meta, sched = g["meta"], _schedule(g)
    if per_env:
        env = _product(g, num_envs=8, load=[float(meta["kwargs"]["load"])] * 8, event_capacity=event_capacity_for(_max_load(g)))
        full = env
        assert isinstance(env.load, np.ndarray)

        class _One:  # env 7 of the batch behind the read-backs used below
            def __getattr__(self, name):
                fn = getattr(full, name)
                if name in ("services", "counters"):
                    return lambda: fn()[7:8]
                if name in ("n_active", "slots", "link_stats", "net_stats"):
                    return lambda i=0: fn(7)
                return fn
        env = _One()
    else:
        env = _product(g, event_capacity=event_capacity_for(_max_load(g)))
    chk = _exact("s1 rmsa run")
    cuts = sorted(set(sched) | set(meta["snapshot_steps"]))
    t = 0
    for c in cuts:
        if c > t:
            env.run(meta["policy"], c - t)
            t = c
        chk(t, "svc", env.services()[0], g["svc"][t])
        chk(t, "counters", env.counters()[0, [0, 1, 4, 5]], g["counters"][t - 1][[0, 1, 4, 5]])
        chk(t, "n_active", env.n_active(0), int(g["n_active"][t - 1]))
        if t in meta["snapshot_steps"]:
            chk(t, "snap_slots", np.packbits(env.slots(0)[0], axis=-1, bitorder="little"), g["snap%d_slots" % t])
            chk(t, "snap_link_stats", env.link_stats(0), g["snap%d_link_stats" % t])
            chk(t, "snap_net_stats", env.net_stats(0), g["snap%d_net_stats" % t])
        if t in sched:
            env.set_load(**sched[t])
    assert t == meta["n_steps"] and not env.flags().any()
    env.close()


# ---- 4. masks and no-ops ------------------------------------------------------------------------------------------------------------
def test_masked_set_load_changes_the_selected_envs_only():
    from oracle.oracle import OracleBatch

    g = load_golden(S1["RMSA"])
    meta, sched = g["meta"], _schedule(g)
    first = min(sched)
    kw = dict(meta["kwargs"])
    seed = kw.pop("seed")
    env = _product(g, num_envs=16, event_capacity=event_capacity_for(_max_load(g)))
    ora = OracleBatch("RMSA", meta["topology"], [seed], **kw)
    mask = (np.arange(16) % 2 == 0).astype(np.uint8)
    T = first + 250
    chk = _exact("masked set_load")
    for t in range(T):
        if g["reset_before"][t]:
            env.reset(full=False)
            ora.reset(full=False)
        if t == first:
            env.set_load(mask=mask, **sched[first])
        env.step(env.policy(meta["policy"]))
        ora.step(ora.policy(meta["policy"]))
        if t % 50 == 49 or t == T - 1:
            svc, cnt = env.services(), env.counters()
            for i in range(16):
                if mask[i]:
                    chk(t, "svc of env %d (fixture)" % i, svc[i], g["svc"][t + 1])
                    chk(t, "counters of env %d (fixture)" % i, cnt[i], g["counters"][t])
                else:
                    chk(t, "svc of env %d (constant load)" % i, svc[i], ora.services()[0])
                    chk(t, "counters of env %d (constant load)" % i, cnt[i], ora.counters()[0])
    load = env.load
    assert list(load[::2]) == [sched[first]["load"]] * 8 and list(load[1::2]) == [meta["kwargs"]["load"]] * 8
    la, lh = env.rates()
    assert len(set(la[::2])) == 1 and len(set(la[1::2])) == 1 and la[0] != la[1] and len(set(lh)) == 1
    env.close()


def _same_everywhere(tag, a, b):
    chk = _exact(tag)
    for what in ("counters", "services", "active", "slots_packed", "link_stats_all", "net_stats_all"):
        chk(0, what, getattr(a, what)(), getattr(b, what)())
    chk(0, "rates", np.stack(a.rates()), np.stack(b.rates()))
    for i in (0, 7, 15):
        (ta, ra), (tb, rb) = a.pending(i), b.pending(i)
        oa, ob = np.lexsort((ra[:, 2], ta)), np.lexsort((rb[:, 2], tb))
        chk(i, "pending release times", ta[oa], tb[ob])
        chk(i, "pending release records", ra[oa], rb[ob])


def test_set_load_to_the_same_values_and_back_changes_nothing():
    """set_load to the values in force, and a change followed by the change back before any step, leave get_state() of the batch
    byte-identical to what it was, and the batch goes on exactly like an untouched twin stepped alike.  The twin is compared
    through every read-back (counters, services, slot maps, link and network statistics, pending releases, rates) and not
    through its raw snapshot: get_state() copies whole arrays, among them bytes the simulation never reads, which differ
    between two batches built and run alike (DESIGN.md 4.7 names the sections)."""
    g = load_golden(S1["RMSA"])
    meta = g["meta"]
    cap = event_capacity_for(400)
    a, b = _product(g, num_envs=16, seeds=list(range(16)), event_capacity=cap), _product(g, num_envs=16, seeds=list(range(16)), event_capacity=cap)
    a.run(meta["policy"], 150)
    b.run(meta["policy"], 150)
    _same_everywhere("twins before", a, b)
    state = a.get_state()
    a.set_load(load=meta["kwargs"]["load"], mean_service_holding_time=meta["kwargs"]["mean_service_holding_time"])
    assert np.array_equal(a.get_state(), state)
    a.set_load(load=400)
    a.set_load(load=meta["kwargs"]["load"])
    assert np.array_equal(a.get_state(), state)
    a.set_load(load=[400.0] * 16, mask=np.arange(16) % 2)
    a.set_load(load=float(meta["kwargs"]["load"]), mask=np.arange(16) % 2)
    assert np.array_equal(a.get_state(), state)
    assert np.array_equal(a.rates()[0], b.rates()[0]) and np.array_equal(a.rates()[1], b.rates()[1])
    for env in (a, b):
        env.run(meta["policy"], 100)
        for _t in range(20):
            env.policy_step(meta["policy"], auto_reset=True, fetch=False)
        env.check()
    _same_everywhere("twins after", a, b)
    a.close()
    b.close()


# ---- 5. refusals leave the batch alone --------------------------------------------------------------------------------------------
def test_refused_set_load_leaves_the_batch_alone():
    from optical_rl_gym_amd import _lib

    g = load_golden(S1["RMSA"])
    meta = g["meta"]
    env = _product(g, num_envs=8, seeds=list(range(8)))  # event_capacity derived from the initial load 150: 336 -> 384
    env.run(meta["policy"], 100)
    state, rates, load = env.get_state(), env.rates(), env.load
    with pytest.raises((ValueError, _lib.OrlError), match="event_capacity"):
        env.set_load(load=400)  # needs 664
    with pytest.raises((ValueError, _lib.OrlError), match="event_capacity"):
        env.set_load(load=[150, 150, 150, 400, 150, 150, 150, 150])
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            env.set_load(load=bad)
        with pytest.raises(ValueError):
            env.set_load(mean_service_holding_time=[25, 25, bad, 25, 25, 25, 25, 25])
    # the ABI itself refuses a bad rate of a selected env (and ignores the entries of unselected ones)
    la, lh = rates[0].copy(), rates[1].copy()
    la[3] = float("nan")
    assert env.lib.orl_batch_set_rates(env._h, la.ctypes.data, lh.ctypes.data, None) == -1
    m = np.ones(8, np.uint8)
    m[3] = 0
    assert env.lib.orl_batch_set_rates(env._h, la.ctypes.data, lh.ctypes.data, m.ctypes.data) == 0
    assert np.array_equal(env.get_state(), state) and env.load == load
    assert np.array_equal(env.rates()[0], rates[0]) and np.array_equal(env.rates()[1], rates[1])
    env.set_load(load=160)  # 160 + 10 sqrt(160) + 64 = 350 <= 384
    assert env.load == 160
    env.close()


# ---- 6. configuration, not state ---------------------------------------------------------------------------------------------------
def test_rates_are_configuration_not_state():
    dev, _oracles = _sweep_batches("RMSA", per_env_mht=True)
    uni, _o2 = _sweep_batches("RMSA", loads=[400, 400, 400, 400])
    import optical_rl_gym_amd as orl

    kw = dict(SWEEP["RMSA"][0])
    plain = orl.make("RMSA", topology="nsfnet_chen", num_envs=dev.num_envs, seeds=list(range(dev.num_envs)), load=400, **kw)
    sb = dev.lib.orl_batch_state_bytes(dev._h)
    assert sb == plain.lib.orl_batch_state_bytes(plain._h) == uni.lib.orl_batch_state_bytes(uni._h)
    la, lh = dev.rates()
    assert np.array_equal(la, dev._rate_arrays[0]) and np.array_equal(lh, dev._rate_arrays[1])
    for i in range(dev.num_envs):
        miat = 1 / float(float(dev.load[i]) / float(dev.mean_service_holding_time[i]))
        assert la[i] == 1 / miat and lh[i] == 1 / float(dev.mean_service_holding_time[i])
    snap = dev.get_state()
    dev.run("SAP_FF", 50)
    dev.reset(full=True)
    dev.set_state(snap)
    dev.reset(full=False)
    assert np.array_equal(dev.rates()[0], la) and np.array_equal(dev.rates()[1], lh)
    dev.set_load(load=120.0, mask=np.arange(dev.num_envs) < 4)
    la2, lh2 = dev.rates()
    for i in range(dev.num_envs):
        miat = 1 / float(float(dev.load[i]) / float(dev.mean_service_holding_time[i]))
        assert dev.load[i] == (120.0 if i < 4 else SWEEP["RMSA"][1][i % 4])
        assert la2[i] == 1 / miat and lh2[i] == lh[i]
    dev.set_state(snap)  # a snapshot carries no rates: the batch keeps the ones it has
    assert np.array_equal(dev.rates()[0], la2)
    dev.seed(7)
    assert np.array_equal(dev.rates()[0], la2) and np.array_equal(dev.rates()[1], lh2)
    pl_a, pl_h = plain.rates()
    assert (pl_a == 1 / (1 / float(400 / float(25)))).all() and (pl_h == 1 / 25).all() and np.isscalar(plain.load)
    for e in (dev, uni, plain):
        e.close()


# ---- 7. Python surface -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devs", [pytest.param((0,), id="one_shard")] + DEVICE_PAIRS)
def test_multi_device_batch_equals_the_single_batch(devs):
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd.sharding import MultiDeviceBatch

    _need_devices(devs)
    kw, loads, policy = SWEEP["RMSA"]
    n = 24
    seeds = list(range(50, 50 + n))
    env_load = [float(loads[i % 4]) for i in range(n)]
    kw = dict(kw, event_capacity=event_capacity_for(400))
    one = orl.make("RMSA", topology="nsfnet_chen", num_envs=n, seeds=seeds, load=env_load, **kw)
    many = MultiDeviceBatch("RMSA", n, seeds=seeds, device_ids=devs, topology="nsfnet_chen", load=env_load, **kw)
    assert np.array_equal(np.asarray(many.load), one.load)
    new = [float(loads[(i + 1) % 4]) for i in range(n)]
    mask = (np.arange(n) % 3 != 0).astype(np.uint8)
    for env in (one, many):
        env.run(policy, 120)
        env.set_load(load=new, mean_service_holding_time=20.0, mask=mask)
        env.run(policy, 120)
    chk = _exact("multi-device set_load")
    chk(0, "counters", many.counters(), one.counters())
    chk(0, "services", many.services(), one.services())
    chk(0, "rates", np.stack(many.rates()), np.stack(one.rates()))
    chk(0, "load", np.asarray(many.load), one.load)
    chk(0, "holding time", np.asarray(many.mean_service_holding_time), one.mean_service_holding_time)
    # a load the LAST shard's capacity is too small for is refused before any shard is changed
    before, too_much = np.stack(many.rates()), np.array(many.load)
    too_much[:] = 120.0
    too_much[n - 1] = 2000.0
    with pytest.raises(ValueError, match="event_capacity"):
        many.set_load(load=too_much)
    chk(0, "rates after the refusal", np.stack(many.rates()), before)
    chk(0, "load after the refusal", np.asarray(many.load), one.load)
    assert many.shards[0].event_capacity_in_force() == -(-event_capacity_for(400) // 64) * 64
    one.close()
    many.close()


def test_facade_set_load_replays_the_reference_trace():
    from optical_rl_gym_amd import gym_api

    g = load_golden(S1["RMSA"])
    kw = dict(g["meta"]["kwargs"])
    env = gym_api.RMSAEnv(topology=g["meta"]["topology"], event_capacity=event_capacity_for(_max_load(g)), **kw)
    assert env.load == kw["load"] and env.mean_service_holding_time == kw["mean_service_holding_time"]
    assert env.mean_service_inter_arrival_time == 1 / float(kw["load"] / float(kw["mean_service_holding_time"]))
    _replay_with_schedule(env.batch, g, _exact("facade"), set_load=env.set_load)
    after = g["after_change"][-1]
    assert env.load == after[1] and env.mean_service_holding_time == after[2] and env.mean_service_inter_arrival_time == after[3]
    env.close()


def test_vec_env_set_load_on_selected_envs():
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd.vec_env import OpticalVecEnv

    kw = dict(mean_service_holding_time=7.5, mean_service_inter_arrival_time=1.0 / 12.0, j=1, episode_length=50,
              event_capacity=event_capacity_for(200))
    batch = orl.make("DeepRMSA", topology="nsfnet_chen", num_envs=8, seeds=list(range(8)), **kw)
    venv = OpticalVecEnv(batch)
    venv.reset()
    la0, lh0 = batch.rates()
    l0 = 7.5 / (1.0 / 12.0)  # deeprmsa_env.py:25
    assert venv.get_attr("load") == [l0] * 8
    # a change of every env with scalars (indices=None) keeps the batch's attributes scalars, as the constructor does
    venv.env_method("set_load", load=95.0)
    assert np.isscalar(batch.load) and batch.load == 95.0 and np.isscalar(batch.mean_service_inter_arrival_time)
    assert (batch.rates()[0] == 1 / (1 / float(95.0 / float(7.5)))).all()
    venv.env_method("set_load", load=l0)
    assert np.isscalar(batch.load) and np.array_equal(batch.rates()[0], la0) and np.array_equal(batch.rates()[1], lh0)
    venv.env_method("set_load", load=150, indices=[1, 4, 5])
    la, lh = batch.rates()
    changed = np.zeros(8, bool)
    changed[[1, 4, 5]] = True
    assert np.array_equal(la[~changed], la0[~changed]) and np.array_equal(lh, lh0)
    assert (la[changed] == 1 / (1 / float(150 / float(7.5)))).all()
    assert venv.get_attr("load") == [150.0 if c else l0 for c in changed]
    assert venv.get_attr("mean_service_inter_arrival_time", indices=[0, 1]) == [1 / float(l0 / 7.5), 1 / float(150 / 7.5)]
    venv.env_method("set_load", None, 10.0, indices=2)
    assert batch.rates()[1][2] == 1 / 10.0 and batch.rates()[0][2] == 1 / (1 / float(l0 / 10.0))
    venv.close()
