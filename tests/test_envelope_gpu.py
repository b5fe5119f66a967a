"""The whole accepted configuration range on the device (tests/envelope.py holds the table): every case against OracleBatch on the
same seeds, exact, on EVERY env — a warm-up run(), host-driven policy() / step(auto_reset=True) over three episodes, run() in two
unequal chunks, then counters, pending services, pending releases, packed slot maps, link and network statistics — under every
step implementation the case admits, with the kernel that served it asserted through the library's debug queries; policy_step at
k = 8 and 9; action masks and MatrixObservationWithPaths beyond 8 paths; the e* reference traces; snapshot / restore on both
sides of k <= 8; and the refusals of batch_create_impl.  Batches are small: this file is about branches, not throughput.  Nothing
here provokes a fault: every refusal is one the host returns before any launch."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import envelope
from tests.helpers import GOLDEN, golden_names, load_golden, replay
from tests.mask_restate import restate_fast, row_words, unpack_slots
from tests.test_gpu_parity import IMPLS, _exact, _ran_pair_form, force_impl, impl_host  # noqa: F401  (impl_host: a fixture)

pytestmark = pytest.mark.gpu

ENV_TYPE = {"RMSA": 0, "DeepRMSA": 1, "RWA": 2, "RMCSA": 3, "QoSConstrainedRA": 4}
# the two-wavefront form exists in specialisation libraries only (~20 s of hipcc per configuration where none is cached): these cases
PAIR_CASES = ("ring10c8_k8_rmsa", "star65_rmsa", "star129_rwa", "ring31_deep", "s512_w63_rmsa", "rmcsa_c17")


def _impls_of(case):
    """The step implementations a case admits.  Served cases: all of test_gpu_parity.IMPLS.  Far-side cases have one device-resident
    loop and one step kernel whatever is asked: asked for the per-env kernel, for the library's choice, for k_agent and for the two-kernel
    form of the alt library (all must run k_step).  QoSConstrainedRA: its two step kernels."""
    if case.fam == "QoSConstrainedRA":
        return ["wave64", "agent8"]
    return list(IMPLS) if case.served else ["wave64", "split2", "persist", "agent8"]


def _params():
    out = []
    for c in envelope.CASES:
        for v in _impls_of(c):
            marks = []
            if v == "persist_pair" and c.name not in PAIR_CASES:
                marks = [pytest.mark.skip(reason="the two-wavefront form needs a specialisation library per configuration: %s" % ", ".join(PAIR_CASES))]
            out.append(pytest.param(c, v, id="%s-%s" % (c.name, v), marks=marks))
    return out


@pytest.fixture(scope="module")
def topo_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("envelope_topologies")


def _pair(case, topo_dir, batch=None, **extra):
    import optical_rl_gym_amd as orl
    from oracle.oracle import OracleBatch

    path = envelope.topology_npz(case.topo, case.k, topo_dir)
    seeds = envelope.seeds_of(case)[:batch or case.batch]
    dev = orl.make(case.fam, topology=path, num_envs=len(seeds), seeds=seeds, **dict(case.kw, **extra))
    ora = OracleBatch(case.fam, path, seeds, **dict(envelope.oracle_kwargs(case), **extra))
    return dev, ora


def _compare_state(chk, t, dev, ora, case):
    chk(t, "counters", dev.counters(), ora.counters())
    chk(t, "services", dev.services(), ora.services())
    chk(t, "active", dev.active(), ora.active())
    if case.fam == "QoSConstrainedRA":
        for e in range(dev.num_envs):
            chk(t, "spectrum of env %d" % e, dev.spectrum(e), ora.spectrum(e))
            chk(t, "link utilisation / last update of env %d" % e, dev.link_stats(e)[[0, 3]], ora.link_stats(e)[[0, 3]])
        return
    chk(t, "slot maps", dev.slots_packed(), ora.slots_packed())
    chk(t, "link statistics", dev.link_stats_all(), ora.link_stats_all())
    chk(t, "network statistics", dev.net_stats_all(), ora.net_stats_all())
    if dev.obs_dim:
        chk(t, "observation", dev.observation(), ora.observation())


def _assert_kernels(case, impl, dev, st, policy=None, ora=None):
    """The kernel the table expects really ran: the device-resident loop of run() `st` and the host-driven step kernel.  A run of the
    persistent kernel names it; any other loop names its kernels only when they are timed one by one (time_kernels=1), so with
    `policy` four more steps are run that way (and by the oracle `ora`)."""
    names = [n for n, _ in st.kernels()]
    step_kernel = int(dev.lib.orl_batch_debug_step_kernel(dev._h))
    form = int(dev.lib.orl_batch_debug_persist_form(dev._h))
    what = (case.name, impl, names, step_kernel, form)
    persistent = case.served and impl not in ("wave64", "split2")
    if not persistent:
        assert names == [] and form == -1, what
        if policy is not None:
            timed = [n for n, _ in dev.run(policy, 4, time_kernels=1).kernels()]
            ora.run(policy, 4)
            what += (timed,)
            assert "k_persist" not in timed, what
            if case.fam != "QoSConstrainedRA":
                if case.served and impl == "split2":
                    assert timed[0] == "k_step_a2", what
                else:
                    assert timed == ["k_step"], what
    if case.fam == "QoSConstrainedRA":
        assert step_kernel == (2 if impl == "agent8" and case.k <= 8 else 0), what  # k_agent_qos serves k <= 8 only
    elif not persistent:
        assert step_kernel == 0, what  # no k_agent without the persistent kernel, even when asked for (ORL_AGENT_STEP=1)
    else:
        assert names == ["k_persist"] and form >= 0, what
        assert step_kernel == (2 if impl == "agent8" else 0), what
        if impl == "persist_pair":
            assert _ran_pair_form(dev) == (case.fam != "RMCSA"), what
        if impl == "persist_rd" and case.topo.startswith("star"):
            # rows-deferred: single-core families with at most 64 links (star65: 64, star66: 65, star129: 128)
            assert (form == 7) == (case.topo == "star65"), what


@pytest.mark.parametrize("case,impl", _params())
def test_every_env_of_every_case_equals_the_oracle(case, impl, topo_dir, monkeypatch):
    force_impl(monkeypatch, impl)
    for policy in case.policies:
        dev, ora = _pair(case, topo_dir)
        chk = _exact("%s %s %s" % (case.name, impl, policy))
        st = dev.run(policy, case.warm)
        ora.run(policy, case.warm)
        _assert_kernels(case, impl, dev, st, policy, ora)
        _compare_state(chk, -1, dev, ora, case)
        dones = np.zeros(dev.num_envs, np.int64)
        for t in range(case.steps):
            a_o, a_d = ora.policy(policy), dev.policy(policy)
            chk(t, "actions", a_d, a_o)
            obs_o, r_o, d_o, i_o = ora.step(a_o, auto_reset=True)
            obs_d, r_d, d_d, i_d = dev.step(a_d, auto_reset=True)
            chk(t, "reward", r_d, r_o)
            chk(t, "done", d_d, d_o)
            chk(t, "info", i_d, i_o)
            if obs_o is not None:
                chk(t, "obs", obs_d, obs_o)
            dones += np.asarray(d_d, np.int64)
        assert (dones >= 3).all()
        _compare_state(chk, case.steps, dev, ora, case)
        for chunk in (41, 23):
            st = dev.run(policy, chunk)
            ora.run(policy, chunk)
        _assert_kernels(case, impl, dev, st)
        _compare_state(chk, case.steps + 64, dev, ora, case)
        assert not dev.flags().any()
        dev.check()
        dev.close()


@pytest.mark.parametrize("name,agent,launches", [("ring10c8_k8_rmsa", "1", 1), ("ring10c8_k9_rmsa", "1", 2), ("ring10c8_k8_deep_j8", "1", 1),
                                                 ("ring10c8_k9_deep_j8", "1", 2), ("k6full_k64_rwa", None, 2)])
def test_policy_step_equals_policy_then_step_on_both_sides_of_8_paths(name, agent, launches, topo_dir, monkeypatch):
    """orl_batch_policy_step is ONE launch (k_agent with the scan as its first phase) where k_agent serves the batch, else k_policy
    and the step kernel: beyond 8 paths always the two, even when k_agent is asked for."""
    case = envelope.CASE_BY_NAME[name]
    force_impl(monkeypatch, "persist")
    if agent is not None:
        monkeypatch.setenv("ORL_AGENT_STEP", agent)
    policy = case.policies[-1]
    a, ora = _pair(case, topo_dir)
    b, _ = _pair(case, topo_dir)
    assert int(a.lib.orl_batch_debug_step_kernel(a._h)) == (2 if launches == 1 else 0)
    chk = _exact(name + " policy_step")
    for env in (a, b, ora):
        env.run(policy, case.warm)
    for t in range(case.steps):
        act_a, o_a, r_a, d_a, i_a = a.policy_step(policy, auto_reset=True)
        act_b = b.policy(policy).copy()
        o_b, r_b, d_b, i_b = b.step(None, auto_reset=True)
        act_o = ora.policy(policy)
        o_o, r_o, d_o, i_o = ora.step(act_o, auto_reset=True)
        chk(t, "actions", act_a, act_b); chk(t, "actions vs oracle", act_a, act_o)
        chk(t, "reward", r_a, r_b); chk(t, "done", d_a, d_b); chk(t, "info", i_a, i_b); chk(t, "info vs oracle", i_a, i_o)
        if o_b is not None:
            chk(t, "obs", o_a, o_b); chk(t, "obs vs oracle", o_a, o_o)
    _compare_state(chk, case.steps, a, ora, case)
    _compare_state(chk, case.steps, b, ora, case)
    a.check(); b.check()
    a.close(); b.close()


MASK_CASES = ["ring10c8_k8_rmsa", "ring10c8_k9_rmsa", "ring10c8_k16_rmsa", "ring10c8_k9_rwa", "ring10c8_k8_deep_j8", "ring10c8_k9_deep_j8_rej",
              "k6full_k64_rmsa", "k6full_k64_deep_j8", "k6full_k64_rwa", "star129_rmsa", "star129_deep", "star129_rwa"]


def _expected_mask(case, ora, topo, layout):
    S = case.kw["num_spectrum_resources"]
    avail = unpack_slots(ora.slots_packed(), topo.n_links, S, row_words(S))
    return restate_fast(ENV_TYPE[case.fam], avail, ora.services(), topo, case.k, S, j=case.kw.get("j", 1),
                        channel_width=50.0 if case.fam == "RWA" else 12.5, allow_rejection=bool(ora.cfg.allow_rejection), layout=layout)


@pytest.mark.parametrize("name", MASK_CASES)
def test_action_masks_beyond_8_paths_equal_the_restatement(name, topo_dir):
    """Lane = path, p = gl, gl + 8, ... for k > 8 (orl_mask.h): k = 8, 9, 16, 64 and the 129-node star, both layouts, from the ORACLE's
    state (slot maps and pending services) after the warm-up and after every 8th of 40 further steps."""
    case = envelope.CASE_BY_NAME[name]
    policy = case.policies[0]
    dev, ora = _pair(case, topo_dir)
    topo = dev.topology
    dev.run(policy, case.warm)
    ora.run(policy, case.warm)
    layouts = ["joint"] if case.fam == "DeepRMSA" else ["joint", "path"]
    seen = 0
    for t in range(41):
        if t % 8 == 0:
            for layout in layouts:
                got = dev.action_mask(layout)
                want = _expected_mask(case, ora, topo, layout)
                assert got.shape == want.shape, (name, layout, got.shape, want.shape)
                bad = np.flatnonzero((got != want).any(axis=1))
                assert len(bad) == 0, "%s %s step %d: %d envs differ, first %d" % (name, layout, t, len(bad), bad[0])
                if case.k > 8:
                    seen += int(got[:, 8 * (got.shape[1] - 1) // case.k:-1].any())
        a = ora.policy(policy)
        dev.step(a, auto_reset=True)
        ora.step(a, auto_reset=True)
    if case.k > 8 and case.topo != "star129":
        assert seen > 0, "%s: no mask ever had a column of a path index >= 8 set" % name
    dev.check()
    dev.close()


def test_action_mask_too_large_for_lds_is_refused_cleanly(topo_dir):
    """64 paths x 320 slots: 32 envs of 64 five-word bit rows exceed the mask kernel's 48 KiB: ORL_E_INVALID before any launch, the
    path layout (one word per path) is served, and the batch steps on as the oracle does."""
    from optical_rl_gym_amd._lib import OrlError

    case = envelope.CASE_BY_NAME["k6full_k64_rmsa"]
    dev, ora = _pair(case, topo_dir, num_spectrum_resources=320)
    with pytest.raises(OrlError, match="action masks of k = 64 paths x 20480 columns exceed the kernel's LDS budget"):
        dev.action_mask("joint")
    topo = dev.topology
    chk = _exact("k = 64, 320 slots")
    for t in range(30):
        a = ora.policy("SAP_FF")
        chk(t, "actions", dev.policy("SAP_FF"), a)
        _, r_d, d_d, i_d = dev.step(a, auto_reset=True)
        _, r_o, d_o, i_o = ora.step(a, auto_reset=True)
        chk(t, "reward", r_d, r_o); chk(t, "info", i_d, i_o)
    avail = unpack_slots(ora.slots_packed(), topo.n_links, 320, 5)
    want = restate_fast(0, avail, ora.services(), topo, 64, 320, allow_rejection=True, layout="path")
    assert np.array_equal(dev.action_mask("path"), want)
    _compare_state(chk, 30, dev, ora, case)
    dev.close()


@pytest.mark.parametrize("name", ["ring10c8_k8_qos", "ring10c8_k9_qos"])
def test_qos_matrix_observation_with_paths_at_9_paths(name, topo_dir):
    from tests.qos_obs_restate import restate_fast as qos_restate

    case = envelope.CASE_BY_NAME[name]
    dev, ora = _pair(case, topo_dir)
    dev.run("SAP_FF", case.warm)
    ora.run("SAP_FF", case.warm)
    for t in range(25):
        if t % 6 == 0:
            spectrum = np.stack([ora.spectrum(e) for e in range(dev.num_envs)])
            pending = ora.services()[:, 2:5].astype(np.int64)
            want = qos_restate(spectrum, pending, dev.topology, case.kw["num_spectrum_resources"], case.k)
            got = dev.matrix_observation_with_paths()
            bad = np.flatnonzero((got != want).any(axis=1))
            assert got.shape == want.shape and len(bad) == 0, "%s step %d: %d envs differ" % (name, t, len(bad))
        a = ora.policy("LLP_FF")
        dev.step(a, auto_reset=True)
        ora.step(a, auto_reset=True)
    dev.check()
    dev.close()


@pytest.mark.parametrize("name", golden_names("e"))
def test_hip_reproduces_reference_trace_at_the_envelope(name, impl_host):  # noqa: F811
    import optical_rl_gym_amd as orl

    g = load_golden(name)
    kw = dict(g["meta"]["kwargs"])
    seed = kw.pop("seed")
    env = orl.make(g["meta"]["env"], topology=os.path.join(GOLDEN, g["meta"]["topology"]), num_envs=1, seeds=[seed], **kw)
    replay(env, g, _exact(name))
    assert not env.flags().any()
    env.close()


@pytest.mark.parametrize("name", ["ring10c8_k9_rmsa", "star129_rmsa"])
def test_snapshot_and_restore_on_both_sides(name, topo_dir):
    case = envelope.CASE_BY_NAME[name]
    policy = case.policies[0]
    dev, ora = _pair(case, topo_dir)
    dev.run(policy, case.warm)
    ora.run(policy, case.warm)
    snap = dev.get_state()
    chk = _exact(name + " snapshot")
    dev.run(policy, 90)
    ora.run(policy, 90)
    _compare_state(chk, 0, dev, ora, case)
    dev.set_state(snap)
    dev.run(policy, 50)
    for _ in range(40):
        dev.step(dev.policy(policy), auto_reset=True)
    _compare_state(chk, 1, dev, ora, case)
    dev.check()
    dev.close()


def test_batch_refusals(topo_dir):
    """Every limit of batch_create_impl from outside: ORL_E_INVALID with its message, no handle, and the next creation with the
    same topology handle succeeds (the half-built batch left nothing behind that a creation would trip over)."""
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd import _lib

    def refused(base, message, **fields):
        cfg = _lib.EnvConfig.from_buffer_copy(base._cfg)
        for k, v in fields.items():
            setattr(cfg, k, v)
        seeds = np.arange(8, dtype=np.int64)
        h = C.c_void_p()
        rc = base.lib.orl_batch_create_seeded(C.byref(cfg), base._topo_h, 8, seeds.ctypes.data, C.byref(h))
        assert rc == -1 and not h.value, (fields, rc)
        assert message in base.lib.orl_last_error(), (fields, base.lib.orl_last_error())
        rc = base.lib.orl_batch_create_seeded(C.byref(base._cfg), base._topo_h, 8, seeds.ctypes.data, C.byref(h))
        assert rc == 0 and h.value, (fields, rc, base.lib.orl_last_error())
        base.lib.orl_batch_destroy(h)

    kw = dict(load=50, mean_service_holding_time=10.0, episode_length=20)
    rmsa = orl.make("RMSA", topology="nsfnet_chen", num_envs=8, seeds=list(range(8)), **kw)
    refused(rmsa, b"num_spectrum_resources must be in [2, 512]", num_spectrum_resources=1)
    refused(rmsa, b"num_spectrum_resources must be in [2, 512]", num_spectrum_resources=513)
    refused(rmsa, b"bad num_spatial_resources", num_spatial_resources=2)  # C > 1 for a single-core family
    refused(rmsa, b"bad num_spatial_resources", num_spatial_resources=0)
    rmsa.close()
    rmcsa = orl.make("RMCSA", topology="nsfnet_chen", num_envs=8, seeds=list(range(8)), num_spectrum_resources=64, **kw)
    refused(rmcsa, b"bad num_spatial_resources", num_spatial_resources=0)
    refused(rmcsa, b"bad num_spatial_resources", num_spatial_resources=32)
    rmcsa.close()
    deep = orl.make("DeepRMSA", topology="nsfnet_chen", num_envs=8, seeds=list(range(8)), j=8, episode_length=20)
    refused(deep, b"j must be in [1, 8]", j=0)
    refused(deep, b"j must be in [1, 8]", j=9)
    deep.close()
    # a 65-slot service (800 Gb/s on BPSK: 64 + 1), and a per-env window beyond 64 KiB (31 cores x 512 slots on Germany50's 88 links:
    # 174 KiB; on COST239's 26 links the window is 53 136 B and the configuration is a case of the table, rmcsa_c31_s512)
    with pytest.raises(_lib.OrlError, match=r"n_slots entries must be in \[1, 64\]"):
        orl.make("RMSA", topology="nsfnet_chen", num_envs=8, seeds=list(range(8)), num_spectrum_resources=320,
                 bit_rate_selection="discrete", bit_rates=(100, 800), **kw)
    with pytest.raises(_lib.OrlError, match="per-env LDS window too large"):
        orl.make("RMCSA", topology="germany50", num_envs=8, seeds=list(range(8)), num_spectrum_resources=512, num_spatial_resources=31,
                 worst_xt=-84.7, **kw)
    env = orl.make("RMSA", topology="nsfnet_chen", num_envs=8, seeds=list(range(8)), **kw)
    env.run("SAP_FF", 30)
    env.check()
    env.close()
