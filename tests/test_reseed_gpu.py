"""seed() on live batches (orl_batch_reseed).  A reseed of a live env does more than replace its generator: the first one copies
the env's MT19937 array, wherever it stands, into a second array from which the bit rates keep coming (the reference's
functools.partial binding, rmsa_env.py:85-87 / 97-99, rmcsa_env.py:87-99), parks that array's position in the env's record, and —
every family but RWA — takes the batch off k_agent / k_agent_qos / k_persist for good: it goes on through k_step on the state those
kernels left behind, and its snapshots grow by the second arrays.

1. the fixtures recorded from the reference (tests/golden/v*, w3_*) under the step forms, the kernel switch included;
2. batches of every family against the CPU oracle, reseeded under masks cut against the groups of 8 envs a wavefront owns, after
   stepping in every form, at 64 envs and at the sizes where the library itself picks k_agent / k_agent_qos;
3. snapshots across reseeds (twin device batches: the oracle has none), and the refusal of a snapshot of the wrong size;
4. the Python surfaces (VecEnv, env_method, the gym facade, MultiDeviceBatch);
5. the readers of the env record after a reseed (action masks, both matrix observations).

Every comparison is == on integers and float64."""
import numpy as np
import pytest

from tests.helpers import golden_names, load_golden, replay_v, replay_w
from tests.test_gpu_parity import DEVICE_PAIRS, _exact, _need_devices, _product, _ran_pair_form, force_impl
from tests.test_set_load_gpu import SWEEP, _sweep_batches

pytestmark = pytest.mark.gpu

ORL_FLAG_MT2 = 4  # csrc/orl_device.h
MT_BYTES = 624 * 4
_OVERRIDES = ("ORL_STEP_IMPL", "ORL_PERSIST", "ORL_AGENT_STEP", "ORL_LIB_VARIANT", "ORL_PERSIST_VARIANT", "ORL_PERSIST_INNER",
              "ORL_PERSIST_RW", "ORL_JIT_SPEC")


def _unforced(monkeypatch):
    for k in _OVERRIDES:
        monkeypatch.delenv(k, raising=False)


def _step_kernel(env):
    return int(env.lib.orl_batch_debug_step_kernel(env._h))


def _persist_spec(env):
    return int(env.lib.orl_batch_debug_persist_spec(env._h))


# ---- 1. the reference's own traces --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", ["wave64", "persist", "agent8"])
@pytest.mark.parametrize("name", golden_names("v") + ["w3_rmsa_events", "w3_rwa_events"])
def test_hip_reproduces_seed_fixtures(name, impl, monkeypatch):
    """Under agent8 the env steps through k_agent (QoS: k_agent_qos) until its first seed — v2 and w3: 45 / 90 steps — and
    through k_step from there on: the switch of kernels on a live env, against the reference itself.  RWA binds no stream and
    keeps its kernels."""
    force_impl(monkeypatch, impl)
    g = load_golden(name)
    meta = g["meta"]
    rwa = meta["env"] == "RWA"
    env = _product(meta, **(dict(action_histograms=True) if "actions_output" in g else {}))
    agent = 2 if impl == "agent8" else 0
    assert _step_kernel(env) == agent and not env.flags().any()
    sb0 = env.lib.orl_batch_state_bytes(env._h)
    seen = []

    def on_event(t, kind):
        if kind == "seed":
            seen.append(t)
            assert _step_kernel(env) == (agent if rwa else 0), (name, t)
            assert env.flags()[0] == (0 if rwa else ORL_FLAG_MT2), (name, t)
            assert env.lib.orl_batch_state_bytes(env._h) == sb0 + (0 if rwa else MT_BYTES), (name, t)

    if name.startswith("w"):
        # replay_w has no hook: the same checks once the replay is over
        replay_w(env, g, _exact(name))
        on_event(meta["n_steps"], "seed")
    else:
        replay_v(env, g, _exact(name), on_event=on_event)
        assert seen and seen[0] == meta["first_seed_step"]
    assert env.flags()[0] == (0 if rwa else ORL_FLAG_MT2)
    env.close()


# ---- 2. batches against the oracle -------------------------------------------------------------------------------------------------
_RMSA, _DEEP, _RWA, _RMCSA, _QOS = (SWEEP[f] for f in ("RMSA", "DeepRMSA", "RWA", "RMCSA", "QoSConstrainedRA"))
# name: (family, kwargs, one load per oracle batch (interleaved over the env index), heuristic)
FAMS = {
    "rmsa": ("RMSA", _RMSA[0], _RMSA[1], _RMSA[2]),
    "rmsa_discrete": ("RMSA", dict(mean_service_holding_time=25, episode_length=100, num_spectrum_resources=64, allow_rejection=True,
                                   bit_rate_selection="discrete"), [40, 120, 90, 60], "SAP_FF"),
    "deeprmsa": ("DeepRMSA", dict(j=2, episode_length=50), _DEEP[1], _DEEP[2]),
    "rwa": ("RWA", _RWA[0], _RWA[1], _RWA[2]),
    "rmcsa": ("RMCSA", _RMCSA[0], _RMCSA[1], _RMCSA[2]),
    "qos": ("QoSConstrainedRA", _QOS[0], _QOS[1], _QOS[2]),
}
# The two-wavefront form of the persistent kernel exists in specialisation libraries only, one per configuration (sizes and the
# capacity the load asks for are compile-time constants): its cases run the benchmark's configurations, whose libraries the build
# makes, and the discrete mode the configuration of the reference's own test, whose library the build makes for this.
PAIR = {
    "rmsa": ("RMSA", dict(mean_service_holding_time=25, episode_length=100, num_spectrum_resources=320, allow_rejection=False), [300] * 4, "SAP_FF"),
    "rmsa_discrete": ("RMSA", dict(mean_service_holding_time=25, episode_length=100, num_spectrum_resources=64, allow_rejection=True,
                                   bit_rate_selection="discrete"), [50] * 4, "SAP_FF"),
    "deeprmsa": ("DeepRMSA", dict(j=1, episode_length=50), [90] * 4, "SAP"),
    "rwa": ("RWA", dict(mean_service_holding_time=25, episode_length=200, allow_rejection=True), [450] * 4, "SAP_FF"),
    "rmcsa": ("RMCSA", dict(mean_service_holding_time=25, episode_length=100, num_spectrum_resources=320, num_spatial_resources=7,
                            allow_rejection=True), [1500] * 4, "SAP_BM_FC_FF"),
}
_SPECIAL = [0, -3, 2**32, 2**62 + 11, None]


def _seeds(n, shift):
    """New seeds per env: 0, a negative one, 2**32, 2**62 + 11 and None among them, at other envs in the second reseed."""
    return [_SPECIAL[(i + shift) % 8] if (i + shift) % 8 < 5 else 7000 * (shift + 1) + i for i in range(n)]


def _masks(n):
    """The masks of the two reseeds, cut against the groups of 8 envs a wavefront owns.  First: group 0 fully selected, group 1 not at
    all, group 2 its first env only, group 3 its last env only, from env 32 on every third.  Second: the first half of group 0 (a
    second time, beside envs that keep their first reseed), the last env of group 1 alone, all of group 2 (one env a second time,
    seven a first time), none of group 3, from env 32 on every second — so that from there envs reseeded twice (i % 6 == 0), first
    now, first before and never share the groups."""
    i = np.arange(n)
    first = np.where(i < 8, 1, np.where(i < 16, 0, np.where(i < 24, i == 16, np.where(i < 32, i == 31, i % 3 == 0)))).astype(np.uint8)
    second = np.where(i < 8, i < 4, np.where(i < 16, i == 15, np.where(i < 24, 1, np.where(i < 32, 0, i % 2 == 0)))).astype(np.uint8)
    return first, second


def test_the_masks_hold_the_groups_asked_for():
    first, second = _masks(64)
    groups = [m[g * 8:(g + 1) * 8] for m in (first, second) for g in range(4)]
    one_hot = lambda k: [int(j == k) for j in range(8)]  # noqa: E731
    for want in ([1] * 8, [0] * 8, one_hot(0), one_hot(7)):
        assert any(list(g) == want for g in groups), want
    assert list(first[32:]) == [int(i % 3 == 0) for i in range(32, 64)]
    both, none = first & second, (1 - first) & (1 - second)
    assert both.any() and none.any() and (first & (1 - second)).any() and (second & (1 - first)).any()
    for shift in (0, 3):
        assert all(any(s is v or (s is not None and s == v) for s in _seeds(64, shift)) for v in _SPECIAL)


def _sample(n):
    """The envs whose per-env read-backs are compared where a family has no bulk read-back: all of a small batch, of a large one the
    first 40 (the groups the masks are cut against) and every 61st."""
    return list(range(n)) if n <= 64 else sorted(set(range(40)) | set(range(40, n, 61)))


class _Pair:
    """A device batch and the oracle batches that hold its envs (one per load: tests.test_set_load_gpu._sweep_batches)."""

    def __init__(self, tag, dev, oracles, policy):
        self.tag, self.dev, self.oracles, self.policy = tag, dev, oracles, policy
        self.qos = dev.ENV_TYPE == 4
        self.rwa = dev.ENV_TYPE == 2
        self.reseeded = np.zeros(dev.num_envs, bool)

    def host(self, n):
        for _t in range(n):
            self.dev.policy_step(self.policy, auto_reset=True, fetch=False)
        self.dev.check()
        for _idx, ora in self.oracles:
            ora.run(self.policy, n)

    def run(self, n):
        st = self.dev.run(self.policy, n)
        for _idx, ora in self.oracles:
            ora.run(self.policy, n)
        return st

    def seed(self, seeds, mask):
        self.dev.seed(seeds, mask=mask)
        for idx, ora in self.oracles:
            ora.seed([seeds[i] for i in idx], mask=mask[idx])
        self.reseeded |= mask.astype(bool)

    def reset(self, full, mask):
        self.dev.reset(full=full, mask=mask)
        for idx, ora in self.oracles:
            ora.reset(full=full, mask=mask[idx])

    def compare(self, what):
        """Counters, services, active lists, slot maps, link and network statistics (QoS: spectrum and link statistics), the
        DeepRMSA observation, the flags; then one step of the heuristic with everything it returns — the info of the discrete mode
        holds the blocking per bit rate and the fairness, which are made of the two bit-rate histograms and nothing else."""
        dev, chk = self.dev, _exact("%s, %s" % (self.tag, what))
        d_cnt, d_svc, d_act = dev.counters(), dev.services(), dev.active()
        d_obs = dev.observation().copy() if dev.obs_dim else None
        if not self.qos:
            d_ls, d_ns, d_sl = dev.link_stats_all(), dev.net_stats_all(), dev.slots_packed()
        picked = set(_sample(dev.num_envs))
        for idx, ora in self.oracles:
            chk(idx[0], "counters", d_cnt[idx], ora.counters())
            chk(idx[0], "services", d_svc[idx], ora.services())
            chk(idx[0], "active", d_act[idx], ora.active())
            if self.qos:
                for k, i in enumerate(idx):
                    if i in picked:
                        chk(i, "spectrum", dev.spectrum(i), ora.spectrum(k))
                        chk(i, "link statistics", dev.link_stats(i)[[0, 3]], ora.link_stats(k)[[0, 3]])
            else:
                chk(idx[0], "slot maps", d_sl[idx], ora.slots_packed())
                chk(idx[0], "link statistics", d_ls[idx], ora.link_stats_all())
                chk(idx[0], "network statistics", d_ns[idx], ora.net_stats_all())
            if d_obs is not None:
                chk(idx[0], "observation", d_obs[idx], ora.observation())
        want = np.where(self.reseeded & (not self.rwa), ORL_FLAG_MT2, 0)
        chk(0, "flags", dev.flags(), want)
        a_d = dev.policy(self.policy).copy()
        obs_d, r_d, d_d, i_d = dev.step(a_d, auto_reset=True)
        for idx, ora in self.oracles:
            a_o = ora.policy(self.policy)
            chk(idx[0], "actions", a_d[idx], a_o)
            obs_o, r_o, d_o, i_o = ora.step(a_o, auto_reset=True)
            chk(idx[0], "reward", r_d[idx], r_o)
            chk(idx[0], "done", d_d[idx], d_o)
            chk(idx[0], "info", i_d[idx], i_o)
            if obs_o is not None:
                chk(idx[0], "observation of the step", obs_d[idx], obs_o)


def _pair(name, table=FAMS, n_seeds=16, omp=False, **extra):
    fam, kw, loads, policy = table[name]
    dev, oracles = _sweep_batches(fam, n_seeds=n_seeds, loads=loads, kw=kw, omp=omp or n_seeds > 16, **extra)
    return _Pair(name, dev, oracles, policy)


def _reseed_sequence(p, before, n_host=50, n_run=60, n_more=25, n_end=15):
    """37 steps in the form under test, a masked reseed, host steps and a device-resident run, a second reseed under another mask,
    more steps, a masked full reset and a masked soft reset, steps again; the oracle compared after every phase, and the routing
    the library documents asserted: off k_agent / k_persist for good, except RWA."""
    dev = p.dev
    n = dev.num_envs
    first, second = _masks(n)
    sb0 = dev.lib.orl_batch_state_bytes(dev._h)
    before(p)
    p.compare("before the reseed")  # (37 steps: the envs stand at different positions of their streams and hold pending releases)
    agent0 = _step_kernel(dev)

    p.seed(_seeds(n, 0), first)
    assert dev.lib.orl_batch_state_bytes(dev._h) == sb0 + (0 if p.rwa else n * MT_BYTES)
    assert _step_kernel(dev) == (agent0 if p.rwa else 0)
    p.compare("right after the first reseed")
    p.host(n_host)
    p.compare("host steps after the first reseed")
    st = p.run(n_run)
    if p.rwa:
        assert _persist_spec(dev) >= 0 and st.launches >= 1  # the persistent kernel, on the new generators
    else:
        assert _persist_spec(dev) == -1 and _step_kernel(dev) == 0
    p.compare("a device-resident run after the first reseed")

    p.seed(_seeds(n, 3), second)
    assert dev.lib.orl_batch_state_bytes(dev._h) == sb0 + (0 if p.rwa else n * MT_BYTES)
    p.host(n_more)
    p.compare("host steps after the second reseed")
    i = np.arange(n)
    p.reset(True, (i % 4 == 1).astype(np.uint8))   # k_reset keeps the flag and the parked position of the second stream
    p.reset(False, (i % 4 == 2).astype(np.uint8))
    p.compare("right after the resets")
    p.host(n_end)
    p.run(n_end)
    assert _step_kernel(dev) == (agent0 if p.rwa else 0) and (_persist_spec(dev) >= 0) == p.rwa
    p.compare("after the resets")
    dev.close()


def _by_host(p):
    p.host(37)


def _by_run(p):
    st = p.run(37)
    assert p.qos or (_persist_spec(p.dev) >= 0 and st.launches >= 1)


@pytest.mark.parametrize("form", ["host", "agent", "run"])
@pytest.mark.parametrize("name", sorted(FAMS))
def test_reseed_after_every_way_of_stepping(name, form, monkeypatch):
    """64 envs: host steps through k_step, host steps through k_agent / k_agent_qos (forced), a device-resident run in the form the
    library picks."""
    _unforced(monkeypatch)
    if form == "agent":
        monkeypatch.setenv("ORL_AGENT_STEP", "1")
    p = _pair(name)
    assert _step_kernel(p.dev) == (2 if form == "agent" else 0)
    _reseed_sequence(p, _by_run if form == "run" else _by_host)


@pytest.mark.parametrize("name", sorted(PAIR))
def test_reseed_after_a_run_in_the_two_wavefront_form(name, monkeypatch):
    """(QoSConstrainedRA has no persistent kernel, hence no such form; RMCSA's specialisation is the one-wavefront kernel.)"""
    force_impl(monkeypatch, "persist_pair")
    p = _pair(name, table=PAIR)

    def before(p):
        _by_run(p)
        assert p.dev.specialised and (_ran_pair_form(p.dev) or name == "rmcsa")

    _reseed_sequence(p, before)


@pytest.mark.parametrize("name", sorted(set(FAMS) - {"qos"}))
def test_reseed_where_the_library_itself_steps_through_k_agent(name, monkeypatch):
    """2 048 envs, nothing forced: the smallest batch step_route sends through k_agent by itself, so the reseed takes it off that
    kernel as it does for a user."""
    _unforced(monkeypatch)
    p = _pair(name, n_seeds=512)
    assert _step_kernel(p.dev) == 2
    _reseed_sequence(p, _by_host)


def test_reseed_where_the_library_itself_steps_through_k_agent_qos(monkeypatch):
    """20 480 QoSConstrainedRA envs, nothing forced: the smallest batch step_route sends through k_agent_qos.  The whole sequence at
    its full length: a QoS step is cheap enough for the CPU oracle of 20 480 envs (a quarter of a second for 120 steps, measured);
    most of this test's few seconds go into making three times 20 480 generator states in Python.  Spectrum and link statistics,
    which have no bulk read-back, are compared on the envs of _sample()."""
    _unforced(monkeypatch)
    p = _pair("qos", n_seeds=5120)
    assert _step_kernel(p.dev) == 2
    _reseed_sequence(p, _by_host)


@pytest.mark.parametrize("name", ["rmsa", "rmsa_discrete"])
def test_the_second_stream_regenerates_after_a_reseed(name, monkeypatch):
    """Both bit-rate modes, 660 + 60 services of every reseeded env after its reseed: a service takes at least one of the 624 words
    of the construction-time stream, so that stream passes its end — and is regenerated in place, in the second array — at least
    once, wherever it stood when it was copied."""
    _unforced(monkeypatch)
    p = _pair(name, omp=True)
    _reseed_sequence(p, _by_host, n_host=60, n_run=660)


# ---- 3. snapshots across a reseed ---------------------------------------------------------------------------------------------------
def _readback(env):
    out = dict(counters=env.counters(), services=env.services(), active=env.active(), flags=env.flags())
    if env.ENV_TYPE == 4:
        out["spectrum"] = np.stack([env.spectrum(i) for i in range(env.num_envs)])
        out["link_stats"] = np.stack([env.link_stats(i) for i in range(env.num_envs)])
    else:
        out.update(slots=env.slots_packed(), link_stats=env.link_stats_all(), net_stats=env.net_stats_all())
    if env.obs_dim:
        out["observation"] = env.observation().copy()
    for i in (0, env.num_envs - 1) if env.ENV_TYPE != 4 else ():
        t, rec = env.pending(i)
        order = np.lexsort((rec[:, 2], t))
        out["pending times %d" % i], out["pending records %d" % i] = t[order], rec[order]
    return out


def _same(tag, a, b):
    chk = _exact(tag)
    assert sorted(a) == sorted(b)
    for k in a:
        chk(0, k, a[k], b[k])


def _go_on(env, policy):
    """A device-resident run and host steps; what the batch looks like afterwards."""
    env.run(policy, 60)
    for _t in range(15):
        env.policy_step(policy, auto_reset=True, fetch=False)
    env.check()
    return _readback(env)


@pytest.mark.parametrize("name", sorted(FAMS))
def test_snapshot_across_reseeds(name, monkeypatch):
    """Twin device batches.  A snapshot taken after a masked reseed brings back flags, second streams and parked positions — after a
    run, and after a second reseed under another mask (against the twin that never had the second one).  A snapshot's size follows
    the batch: one taken before the first reseed no longer fits, one of a reseeded batch does not fit a fresh batch; set_state
    refuses both with ValueError before the library is called, and the batch's state stays as it was.  (RWA keeps no second stream:
    its state does not grow and its earlier snapshots stay valid.)"""
    import optical_rl_gym_amd as orl

    _unforced(monkeypatch)
    fam, kw, loads, policy = FAMS[name]
    n = 32
    args = dict(mean_service_holding_time=7.5, mean_service_inter_arrival_time=7.5 / loads[1]) if fam == "DeepRMSA" else dict(load=loads[1])
    a, b, fresh = (orl.make(fam, topology="nsfnet_chen", num_envs=n, seeds=list(range(300, 300 + n)), **kw, **args) for _ in range(3))
    rwa = fam == "RWA"
    first, second = _masks(n)
    for env in (a, b):
        env.run(policy, 37)
    sb0 = a.lib.orl_batch_state_bytes(a._h)
    early = a.get_state()
    assert early.size == sb0
    for env in (a, b):
        env.seed(_seeds(n, 0), mask=first)
    grown = sb0 + (0 if rwa else n * MT_BYTES)
    assert a.lib.orl_batch_state_bytes(a._h) == grown and fresh.lib.orl_batch_state_bytes(fresh._h) == sb0
    snap = a.get_state()
    assert snap.size == grown
    want_flags = np.where(first.astype(bool) & (not rwa), ORL_FLAG_MT2, 0)

    # reseed -> snapshot -> run -> restore -> run again
    once = _go_on(a, policy)
    twin = _go_on(b, policy)
    _same("%s: twins after the reseed" % name, once, twin)
    a.set_state(snap)
    assert np.array_equal(a.flags(), want_flags)
    _same("%s: the run repeated from the snapshot" % name, _go_on(a, policy), once)

    # ... -> second reseed with another mask -> steps -> restore: as if the second reseed had never been
    a.set_state(snap)
    a.seed(_seeds(n, 3), mask=second)
    assert np.array_equal(a.flags(), np.where((first | second).astype(bool) & (not rwa), ORL_FLAG_MT2, 0))
    a.run(policy, 40)
    a.set_state(snap)
    assert np.array_equal(a.flags(), want_flags) and a.lib.orl_batch_state_bytes(a._h) == grown
    _same("%s: restored behind a second reseed" % name, _go_on(a, policy), twin)

    # snapshots of the wrong size
    if not rwa:
        for env, wrong in ((a, early), (fresh, snap)):
            state, look = env.get_state(), _readback(env)
            with pytest.raises(ValueError, match="set_state"):
                env.set_state(wrong)
            assert np.array_equal(env.get_state(), state)
            _same("%s: after the refusal" % name, _readback(env), look)
        _same("%s: the refused batch goes on" % name, _go_on(a, policy), _go_on(b, policy))
    else:
        a.set_state(early)  # still fits: back before the reseed
        assert not a.flags().any()
    for env in (a, b, fresh):
        env.close()


# ---- 4. the Python surfaces -----------------------------------------------------------------------------------------------------------
def _vec_pair(n=8):
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd.vec_env import OpticalVecEnv
    from oracle.oracle import OracleBatch

    kw = dict(mean_service_holding_time=7.5, mean_service_inter_arrival_time=1.0 / 12.0, j=2, episode_length=50)
    seeds = list(range(40, 40 + n))
    venv = OpticalVecEnv(orl.make("DeepRMSA", topology="nsfnet_chen", num_envs=n, seeds=seeds, **kw))
    return venv, OracleBatch("DeepRMSA", "nsfnet_chen", seeds, **kw)


def _vec_steps(venv, ora, obs, n, chk, what):
    """n steps of the SAP heuristic through the VecEnv and through the oracle (both reset finished episodes by themselves)."""
    chk(0, what + ": observation", obs, ora.observation())
    for t in range(n):
        a_o = ora.policy("SAP")
        a_d = venv.batch.policy("SAP")[:, 0].copy()
        chk(t, what + ": actions", a_d, a_o[:, 0])
        obs, rew, done, _infos = venv.step(a_d)
        obs_o, r_o, d_o, _i = ora.step(a_o, auto_reset=True)
        chk(t, what + ": observation", obs, obs_o)
        chk(t, what + ": reward", rew, r_o)
        chk(t, what + ": done", np.asarray(done, np.uint8), d_o)
    chk(n, what + ": services", venv.batch.services(), ora.services())
    chk(n, what + ": counters", venv.batch.counters(), ora.counters())
    return obs


def test_vec_env_seed_and_env_method():
    """OpticalVecEnv.seed(s): env i continues with random.Random(s + i); seed(s, indices) and env_method("seed", s, indices=...)
    reseed the selected envs only, env i with s + i all the same; seed(None) is the reference's 41."""
    venv, ora = _vec_pair()
    n = venv.num_envs
    chk = _exact("vec env")
    obs = venv.reset()
    ora.reset(full=False)
    obs = _vec_steps(venv, ora, obs, 37, chk, "before")

    def mask(indices):
        m = np.zeros(n, np.uint8)
        m[indices] = 1
        return m

    assert venv.seed(2**32 - 3) == [2**32 - 3 + i for i in range(n)]
    ora.seed(2**32 - 3)
    obs = _vec_steps(venv, ora, obs, 40, chk, "seed(s)")
    assert venv.seed(-2, indices=[1, 4, 5]) == [-1, 2, 3]
    ora.seed([-2 + i for i in range(n)], mask=mask([1, 4, 5]))
    obs = _vec_steps(venv, ora, obs, 40, chk, "seed(s, indices)")
    assert venv.env_method("seed", 900, indices=[0, 5]) == [900, 905]
    ora.seed(900, mask=mask([0, 5]))
    obs = _vec_steps(venv, ora, obs, 40, chk, "env_method")
    assert venv.env_method("seed", None, indices=7) == [48]
    ora.seed(41, mask=mask([7]))
    _vec_steps(venv, ora, obs, 40, chk, "env_method, None")
    assert np.array_equal(venv.batch.flags(), np.full(n, ORL_FLAG_MT2))
    venv.close()


def test_facade_seed_replays_the_reference_trace():
    """The gym-shaped class: env.seed(s) at the recorded steps of the discrete-mode trace."""
    from optical_rl_gym_amd import gym_api

    name = "v1_seed_rmsa_discrete"
    g = load_golden(name)
    kw = dict(g["meta"]["kwargs"])
    env = gym_api.RMSAEnv(topology=g["meta"]["topology"], **kw)
    returned = []

    class _ThroughTheFacade:
        def __getattr__(self, attr):
            return getattr(env.batch, attr)

        def seed(self, seeds):
            returned.append((seeds[0], env.seed(seeds[0]), env.rand_seed))

    replay_v(_ThroughTheFacade(), g, _exact(name))
    assert len(returned) == 5
    for arg, ret, rand_seed in returned:
        assert ret == [41 if arg is None else arg] and rand_seed == ret[0]  # optical_network_env.py:205-210
    env.close()


@pytest.mark.parametrize("devs", DEVICE_PAIRS)
def test_multi_device_batch_seed_equals_the_single_batch(devs):
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd.sharding import MultiDeviceBatch

    _need_devices(devs)
    fam, kw, loads, policy = FAMS["rmsa_discrete"]
    n = 40  # two shards of 20: the masks' groups of 8 straddle the cut
    seeds = list(range(50, 50 + n))
    one = orl.make(fam, topology="nsfnet_chen", num_envs=n, seeds=seeds, load=90, **kw)
    many = MultiDeviceBatch(fam, n, seeds=seeds, device_ids=devs, topology="nsfnet_chen", load=90, **kw)
    first, second = _masks(n)
    chk = _exact("multi-device seed")
    for step, (sd, mask) in enumerate(((_seeds(n, 0), first), (_seeds(n, 3), second), (77, None))):
        for env in (one, many):
            env.run(policy, 60)
            env.seed(sd, mask=mask)
            env.run(policy, 60)
        chk(step, "counters", many.counters(), one.counters())
        chk(step, "services", many.services(), one.services())
        chk(step, "flags", np.concatenate([s.flags() for s in many.shards]), one.flags())
        lo = 0
        for s in many.shards:
            chk(step, "slot maps", s.slots_packed(), one.slots_packed()[lo:lo + s.num_envs])
            lo += s.num_envs
    one.close()
    many.close()


# ---- 5. readers of the env record after a reseed -------------------------------------------------------------------------------------
def _reseeded(name, n=24):
    """A batch that stepped, was reseeded under the first mask, stepped on, was reseeded under the second and stepped again."""
    import optical_rl_gym_amd as orl

    fam, kw, loads, policy = FAMS[name]
    args = dict(mean_service_holding_time=7.5, mean_service_inter_arrival_time=7.5 / loads[1]) if fam == "DeepRMSA" else dict(load=loads[1])
    env = orl.make(fam, topology="nsfnet_chen", num_envs=n, seeds=list(range(600, 600 + n)), **kw, **args)
    first, second = _masks(n)
    env.run(policy, 80)
    env.seed(_seeds(n, 0), mask=first)
    env.run(policy, 40)
    for _t in range(7):
        env.policy_step(policy, auto_reset=True, fetch=False)
    env.seed(_seeds(n, 3), mask=second)
    for _t in range(9):
        env.policy_step(policy, auto_reset=True, fetch=False)
    env.check()
    assert env.flags().any() and not env.flags().all()
    return env


@pytest.mark.parametrize("name", ["rmsa", "deeprmsa"])
def test_action_mask_of_a_reseeded_batch(name, monkeypatch):
    """The high half of the record's hint word now holds the parked position of the second stream; the mask kernel reads the
    record."""
    from tests.test_action_mask_gpu import _check

    _unforced(monkeypatch)
    env = _reseeded(name)
    _check(env, "after two reseeds")
    env.step(env.policy(FAMS[name][3]), auto_reset=True)
    _check(env, "a step later")
    env.close()


def test_matrix_paths_observation_of_a_reseeded_batch(monkeypatch):
    from tests.test_qos_matrix_obs_gpu import _check

    _unforced(monkeypatch)
    env = _reseeded("qos")
    _check(env, "after two reseeds")
    env.step(env.policy("SAP_FF"), auto_reset=True)
    _check(env, "a step later")
    env.close()


@pytest.mark.parametrize("name", ["rmsa", "rmcsa"])
def test_matrix_observation_of_a_reseeded_batch(name, monkeypatch):
    """SimpleMatrixObservation (rmsa_env.py:806-837, rmcsa_env.py:914-947): one-hot min(source, destination), one-hot
    max(source, destination), the slot maps."""
    _unforced(monkeypatch)
    env = _reseeded(name)
    N = env.topology.n_nodes
    for what in ("after two reseeds", "a step later"):
        got, svc = env.matrix_observation(), env.services()
        want = np.zeros_like(got)
        for i in range(env.num_envs):
            src, dst = int(svc[i, 2]), int(svc[i, 3])
            want[i, min(src, dst)] = 1
            want[i, N + max(src, dst)] = 1
            want[i, 2 * N:] = env.slots(i).reshape(-1)
        assert got.shape[1] == 2 * N + env.slots(0).size and np.array_equal(got, want), (name, what)
        env.step(env.policy(FAMS[name][3]), auto_reset=True)
    env.close()
