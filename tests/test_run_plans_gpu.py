"""Device-resident runs under every run plan, and what happens to an env at the end of an episode (tests/run_plans.py holds the
table; tests/test_run_plans.py proves on the CPU that the plans are the ones stated and that the oracle's trajectories give both
halves of a batch something to get wrong).

A plan is (steps per launch, one stream or two halves on two streams), forced through ORL_PERSIST_CHUNK / ORL_PERSIST_PARTS: the
library itself takes two halves from 16 384 envs only, where no test switches on the per-env arrays whose second-half pointers
env_view (csrc/orl_api.hip) offsets by hand.  Here batches of 9 to 64 envs run in halves of 16 + 4, 8 + 1 and 32 + 32 envs, with
launches of one step, launches that end on, one before and one after the step that returns done, through every form of the
persistent kernel; every case asserts the plan (orl_debug_run_plan under its environment, the number of launches) and the form
(orl_batch_debug_persist_form) that ran.  The reference is the CPU oracle on the same seeds — every env after every piece, floats as
bit patterns, no tolerance anywhere — and the one-wavefront kernels a second one."""
import numpy as np
import pytest

from tests import run_plans as rp
from tests.helpers import _exact_bits, force_impl, resets_between_runs

pytestmark = pytest.mark.gpu

MATRIX = rp.matrix()
TWO = [("7", 2), ("L", 2), ("1", 2)]  # plans of the checks of single arrays: all in two halves


def _plan_ids(plans):
    return [rp.plan_id(p) for p in plans]


def _begin(monkeypatch, name, form, plan, n=20, ledger=False):
    cfg = rp.CONFIGS[name]
    force_impl(monkeypatch, form)
    rp.set_plan(monkeypatch, cfg, plan)
    return cfg, rp.make_dev(cfg, n), rp.Ora(cfg, n, ledger=ledger)


# ---- 1. plans through the persistent kernel ---------------------------------------------------------------------------------
_WAVE64 = {}


def wave64_final(name, n):
    """the last snapshot of the case's sequence under the one-wavefront kernels (itself compared with the oracle piece by piece):
    once per configuration and batch size"""
    if (name, n) not in _WAVE64:
        cfg = rp.CONFIGS[name]
        with pytest.MonkeyPatch.context() as mp:
            force_impl(mp, "wave64")
            dev = rp.make_dev(cfg, n)
            _WAVE64[name, n] = rp.drive_case(dev, rp.Ora(cfg, n), cfg, None, None, "%s, %d envs, wave64" % (name, n))
            assert int(dev.lib.orl_batch_debug_persist_form(dev._h)) == -1
            dev.close()
    return _WAVE64[name, n]


@pytest.mark.parametrize("case", MATRIX, ids=[rp.case_id(c) for c in MATRIX])
def test_every_plan_through_the_persistent_kernel_matches_the_oracle(case, monkeypatch):
    base = wave64_final(case.config, case.n)
    tag = rp.case_id(case)
    cfg, dev, ora = _begin(monkeypatch, case.config, case.form, case.plan, case.n)
    last = rp.drive_case(dev, ora, cfg, case.form, case.plan, tag)
    chk = _exact_bits(tag + ", against the one-wavefront kernels")
    assert set(last) == set(base)
    for what in base:
        chk(0, what, last[what], base[what])
    dev.close()


# ---- 2. the optional per-env arrays, in both halves --------------------------------------------------------------------------
def _runs(dev, ora, cfg, form, plan, tag):
    L = rp.steps_per_episode(cfg)
    for steps in (L + 4, 2 * L):
        rp.run_checked(dev, ora, cfg, form, plan, steps, tag)


def _host_step(dev, ora, cfg):
    a = ora.policy(cfg.policy)
    _o, _r, _d, info_d = dev.step(a, auto_reset=True)
    _r, _d, info_o = ora.step(a, auto_reset=True)
    return np.array(info_d), info_o


def _histograms_equal(dev, ora, tag):
    for i in range(dev.num_envs):
        for which, got, ref in zip(("actions_output", "actions_taken"), dev.action_histograms_of(i), ora.action_histograms_of(i)):
            assert got.shape == ref.shape, (tag, i, which)
            assert np.array_equal(got, ref), "%s: %s of env %d (%s) differs at cells %r" % (
                tag, which, i, rp.half_of(i, dev.num_envs, ("7", 2)), np.argwhere(got != ref)[:6].tolist())
        assert dev.action_histograms_of(i)[0].sum() > 0


@pytest.mark.parametrize("plan", TWO, ids=_plan_ids(TWO))
def test_bit_rate_and_action_histograms_in_both_halves(plan, monkeypatch):
    """discrete bit rates: the four bit-rate histograms through the info entries made of them (rmsa_env.py:258-282), of every env,
    at the host step after the run; the opt-in 2-D action histograms of every env"""
    tag = "rmsa_disc, %s" % rp.plan_id(plan)
    cfg, dev, ora = _begin(monkeypatch, "rmsa_disc", "persist", plan)
    _runs(dev, ora, cfg, "persist", plan, tag)
    _histograms_equal(dev, ora, tag)
    info_d, info_o = _host_step(dev, ora, cfg)
    keys = dev.info_keys
    chk = _exact_bits(tag + ", the host step after the runs")
    cols = [keys.index("bit_rate_blocking_%d" % r) for r in (10, 40, 100)]
    for i in range(dev.num_envs):
        chk(i, "blocking per bit rate of env %d (%s)" % (i, rp.half_of(i, 20, plan)), info_d[i, cols], info_o[i, cols])
        chk(i, "fairness of env %d (%s)" % (i, rp.half_of(i, 20, plan)), info_d[i, keys.index("fairness")], info_o[i, keys.index("fairness")])
    chk(0, "info", info_d, info_o)
    assert (info_o[16:, cols] > 0).any() and len({tuple(r) for r in info_o[:, cols]}) >= 19  # (the rows tell the envs apart)
    _histograms_equal(dev, ora, tag)
    dev.close()


@pytest.mark.parametrize("plan", TWO, ids=_plan_ids(TWO))
def test_rwa_action_marginals_in_both_halves(plan, monkeypatch):
    """path_action_probability / wavelength_action_probability (rwa_env.py:140-160) of every env at the host step after the run"""
    tag = "rwa, %s" % rp.plan_id(plan)
    cfg, dev, ora = _begin(monkeypatch, "rwa", "persist", plan)
    _runs(dev, ora, cfg, "persist", plan, tag)
    info_d, info_o = _host_step(dev, ora, cfg)
    K1, S1 = dev.k_paths + 1, dev.num_spectrum_resources + 1
    assert info_d.shape[1] == 2 + K1 + S1 and dev.info_keys[2].startswith("path_action_probability")
    chk = _exact_bits(tag + ", the host step after the runs")
    for i in range(dev.num_envs):
        half = rp.half_of(i, 20, plan)
        chk(i, "path_action_probability of env %d (%s)" % (i, half), info_d[i, 2:2 + K1], info_o[i, 2:2 + K1])
        chk(i, "wavelength_action_probability of env %d (%s)" % (i, half), info_d[i, 2 + K1:], info_o[i, 2 + K1:])
    assert len({tuple(r) for r in info_o[:, 2:]}) == 20
    dev.close()


@pytest.mark.parametrize("plan", TWO, ids=_plan_ids(TWO))
def test_rmcsa_action_histograms_in_both_halves(plan, monkeypatch):
    """the opt-in 4-D arrays (rmcsa_env.py:145-180) of a batch of 2 cores and 16 slots"""
    tag = "rmcsa_small, %s" % rp.plan_id(plan)
    cfg, dev, ora = _begin(monkeypatch, "rmcsa_small", "persist", plan)
    _runs(dev, ora, cfg, "persist", plan, tag)
    _histograms_equal(dev, ora, tag)
    dev.close()


def test_rmcsa_launches_of_one_step_after_a_rejected_service(monkeypatch):
    """What test_rmcsa_action_histograms_in_both_halves[chunk1-parts2] found, under the library's own plan: run(policy, 1) again and
    again.  A launch takes the core whose sums it logs from the env record, which after a rejected service holds the reject index (the
    number of cores): the sums of a core that does not exist went into the log word of the launch's step and overflowed into its core
    field, and where that step was also the launch's last and accepted, its network-compactness update was finished from the wrong
    core's sums.  The heuristic gives the reject action only where no path fits at all (a service that merely fails keeps its core): the
    oracle's trajectory must hold it at least once, followed by an accepted service (here: env 1, step 33)."""
    cfg = rp.CONFIGS["rmcsa_small"]
    force_impl(monkeypatch, "persist")
    monkeypatch.delenv("ORL_PERSIST_CHUNK", raising=False)
    monkeypatch.delenv("ORL_PERSIST_PARTS", raising=False)
    dev, ora = rp.make_dev(cfg, 20), rp.Ora(cfg, 20)
    cores = cfg.kw["num_spatial_resources"]
    history, pattern = [], 0
    for t in range(40):
        a = ora.policy(cfg.policy)
        reward, _done, _info = ora.step(a, auto_reset=True)
        history.append((a[:, 2] == cores, reward > 0))
        if t >= 1:
            pattern += int((history[t - 1][0] & history[t][1]).sum())
        dev.run(cfg.policy, 1)
        assert int(dev.lib.orl_batch_debug_persist_form(dev._h)) >= 0
        rp.compare(dev, ora, cfg, ("128", 1), "rmcsa_small, runs of one step", "run %d" % t)
    assert pattern >= 1, pattern
    dev.close()


@pytest.mark.parametrize("form", ["persist", "persist_global", "persist_rd"])
@pytest.mark.parametrize("plan", TWO, ids=_plan_ids(TWO))
def test_path_ff_with_a_path_column_per_env_in_both_halves(plan, form, monkeypatch):
    tag = "rmsa_pathff, %s, %s" % (form, rp.plan_id(plan))
    cfg, dev, ora = _begin(monkeypatch, "rmsa_pathff", form, plan)
    _runs(dev, ora, cfg, form, plan, tag)
    rp.host_steps(dev, ora, cfg, 2, tag)
    _runs(dev, ora, cfg, form, plan, tag)
    dev.close()


@pytest.mark.parametrize("plan", TWO, ids=_plan_ids(TWO))
def test_per_env_rates_in_both_halves(plan, monkeypatch):
    """rates() as the device holds them after runs in two halves, before and after a masked set_load (the trajectories, which
    depend on them, are compared with the oracle all along)"""
    from optical_rl_gym_amd.envs import derive_rates

    tag = "rmsa_loads, %s" % rp.plan_id(plan)
    cfg, dev, ora = _begin(monkeypatch, "rmsa_loads", "persist", plan)
    loads = np.array(cfg.loads(20))
    chk = _exact_bits(tag)

    def rates_are(loads, label):
        _miat, lam_a, lam_h = derive_rates(loads, np.full(20, cfg.kw["mean_service_holding_time"]))
        got_a, got_h = dev.rates()
        chk(0, "lambda_arrival " + label, got_a, lam_a)
        chk(0, "lambda_holding " + label, got_h, lam_h)

    _runs(dev, ora, cfg, "persist", plan, tag)
    rates_are(loads, "after the runs")
    new, mask = rp.set_load_change(20)
    dev.set_load(load=new, mask=mask)
    ora.set_load(new, mask)
    loads = np.where(mask != 0, new, loads)
    rates_are(loads, "after the masked set_load")
    _runs(dev, ora, cfg, "persist", plan, tag)
    rates_are(loads, "after the runs that followed it")
    dev.close()


@pytest.mark.parametrize("form", rp.forms_of("deeprmsa"))
@pytest.mark.parametrize("plan", TWO, ids=_plan_ids(TWO))
def test_deeprmsa_observation_rows_in_both_halves(plan, form, monkeypatch):
    """the observation the run left in the device buffer is the one a fresh evaluation gives, and the oracle's"""
    tag = "deeprmsa, %s, %s" % (form, rp.plan_id(plan))
    cfg, dev, ora = _begin(monkeypatch, "deeprmsa", form, plan)
    obs = dev.device_tensor("obs")
    chk = _exact_bits(tag)
    L = rp.steps_per_episode(cfg)
    for steps in (L, 1, L + 4):
        rp.run_checked(dev, ora, cfg, form, plan, steps, tag)
        in_loop = obs.cpu().numpy().copy()
        chk(steps, "the rows the run left against the oracle", in_loop, ora.observation())
        chk(steps, "the rows the run left against a fresh observation()", in_loop, dev.observation())
    dev.close()


# ---- 3. the episode log ---------------------------------------------------------------------------------------------------
LOG_PLANS = [("1", 2), ("L", 2), ("L-1", 2), ("7", 2), ("128", 2)]
LOG_RUNS = [(name, plan) for name in ("rmsa", "deeprmsa", "rwa", "rmcsa") for plan in LOG_PLANS] + [("qos", "k_step"), ("qos", "k_agent_qos")]


def _begin_log(monkeypatch, name, route):
    """route: a plan (persistent kernel, the library's form), a name of helpers.IMPLS (host steps), or QoSConstrainedRA's step kernel"""
    cfg = rp.CONFIGS[name]
    if cfg.fam == rp.QOS:
        monkeypatch.setenv("ORL_AGENT_STEP", "1" if route in ("k_agent_qos", "agent8") else "0")
        plan = None
    elif isinstance(route, tuple):
        force_impl(monkeypatch, "persist")
        rp.set_plan(monkeypatch, cfg, route)
        plan = route
    else:
        force_impl(monkeypatch, route)
        plan = None
    dev, ora = rp.make_dev(cfg, 20), rp.Ora(cfg, 20, ledger=True)
    if cfg.fam == rp.QOS:
        assert int(dev.lib.orl_batch_debug_step_kernel(dev._h)) == (2 if route in ("k_agent_qos", "agent8") else 0)
    return cfg, dev, ora, plan


def _log_id(case):
    return "%s-%s" % (case[0], rp.plan_id(case[1]) if isinstance(case[1], tuple) else case[1])


@pytest.mark.parametrize("name,route", LOG_RUNS, ids=[_log_id(c) for c in LOG_RUNS])
def test_episode_log_of_device_resident_runs(name, route, monkeypatch):
    """A log armed for fewer episodes than finish: counts goes on counting, a row keeps its first episodes, nothing else is written
    (every row of every env is compared, a guard row behind the read-back).  Disarmed, nothing is logged and the read-back is
    refused; re-armed with another capacity, counts and rows start from zero."""
    from optical_rl_gym_amd._lib import OrlError

    tag = "episode log, " + _log_id((name, route))
    cfg, dev, ora, plan = _begin_log(monkeypatch, name, route)
    form = "persist" if plan else None
    L = rp.steps_per_episode(cfg)
    rp.arm_log(dev, rp.SMALL_CAP)
    counts, acc, _rew = rp.read_log(dev, rp.SMALL_CAP)
    assert not counts.any() and not acc.any()
    rp.drive_case(dev, ora, cfg, form, plan, tag)
    counts = rp.compare_log(dev, ora, rp.SMALL_CAP, tag + ", capacity %d" % rp.SMALL_CAP)
    assert (counts > rp.SMALL_CAP).all()  # the log was too small for every env
    rp.arm_log(dev, 0)
    with pytest.raises(OrlError, match="not armed"):
        rp.read_log(dev, rp.SMALL_CAP)
    rp.run_checked(dev, ora, cfg, form, plan, L + 2, tag + ", disarmed")
    # (re-armed at an episode's start: the reward sums of QoSConstrainedRA start with the arming)
    dev.reset(full=False)
    ora.reset(full=False)
    rp.arm_log(dev, 9)
    ora.start_ledger()
    counts, acc, rew = rp.read_log(dev, 9)
    assert not counts.any() and not acc.any() and (rew is None or not rew.any())
    rp.run_checked(dev, ora, cfg, form, plan, 3 * L + 1, tag + ", re-armed")
    counts = rp.compare_log(dev, ora, 9, tag + ", capacity 9")
    assert (counts == 3).all()
    rp.arm_log(dev, 0)
    dev.close()


LOG_HOST = [(name, route) for name in ("rmsa", "deeprmsa", "rwa", "rmcsa") for route in ("wave64", "agent8", "split2")] + [("qos", "k_step"), ("qos", "k_agent_qos")]


@pytest.mark.parametrize("name,route", LOG_HOST, ids=[_log_id(c) for c in LOG_HOST])
def test_episode_log_of_host_steps(name, route, monkeypatch):
    """Host-driven steps through every step kernel.  With auto reset: as a device-resident run.  Without: the episode is logged
    once, when done is returned, and not again while the env is stepped on."""
    tag = "episode log, host steps, " + _log_id((name, route))
    cfg, dev, ora, _plan = _begin_log(monkeypatch, name, route)
    if cfg.fam != rp.QOS:
        assert int(dev.lib.orl_batch_debug_step_kernel(dev._h)) == (2 if route == "agent8" else 0)
    L = rp.steps_per_episode(cfg)
    rp.arm_log(dev, rp.SMALL_CAP)
    dones = rp.host_steps(dev, ora, cfg, 3 * L + 2, tag)
    assert (dones.sum(0) == 3).all()
    rp.compare(dev, ora, cfg, ("128", 1), tag, "%d host steps with auto reset" % (3 * L + 2))
    counts = rp.compare_log(dev, ora, rp.SMALL_CAP, tag + ", auto reset, capacity %d" % rp.SMALL_CAP)
    assert (counts == 3).all()
    dev.reset(full=False)
    ora.reset(full=False)
    rp.arm_log(dev, 5)
    ora.start_ledger()
    dones = rp.host_steps(dev, ora, cfg, L + 3, tag + ", no auto reset", auto_reset=False)
    assert (dones.sum(0) == 1).all() and dones[L - 1].all()  # done once, at the episode's last step, and never again
    rp.compare(dev, ora, cfg, ("128", 1), tag, "%d host steps without a reset" % (L + 3))
    counts = rp.compare_log(dev, ora, 5, tag + ", no auto reset, capacity 5")
    assert (counts == 1).all()
    rp.arm_log(dev, 0)
    dev.close()


# ---- 4. episode lengths at the edge -----------------------------------------------------------------------------------------
# (the fixtures recorded from the reference at these lengths, tests/golden/g10_* and q2_*, replay through every host-step route in
# tests/test_gpu_parity.py)
EDGE_BASE = {"RMSA": "rmsa", "DeepRMSA": "deeprmsa", "RWA": "rwa", "RMCSA": "rmcsa", rp.QOS: "qos"}
EDGES = [("RMSA", 1), ("RMSA", 2), ("RMSA", 3), ("DeepRMSA", 1), ("DeepRMSA", 2), ("DeepRMSA", 3), ("RWA", 1), ("RWA", 2), ("RMCSA", 2),
         (rp.QOS, 1), (rp.QOS, 2)]
EDGE_PLANS = [("1", 2), ("128", 2)]


def _edge_cfg(fam, length):
    base = rp.CONFIGS[EDGE_BASE[fam]]
    return base._replace(name="%s_len%d" % (base.name, length), kw=dict(base.kw, episode_length=length))


def _dones_per_step(cfg):
    """Steps between two dones, None where done never comes.  RMSA and DeepRMSA count the pending service when it is created and
    again in the soft reset (rmsa_env.py:314, 576), so episode_length=1 never returns done and 2 makes every step terminal; RWA and
    QoSConstrainedRA count at the decision: 1 makes every step terminal.  RMCSA counts at the decision and in the soft reset
    (rmcsa_env.py:293, 414): as RMSA after a soft reset, but the first episode of a fresh env is a step longer."""
    L = rp.steps_per_episode(cfg)
    return None if L == 0 else L


@pytest.mark.parametrize("plan", EDGE_PLANS, ids=_plan_ids(EDGE_PLANS))
@pytest.mark.parametrize("fam,length", EDGES, ids=["%s-len%d" % e for e in EDGES])
def test_episode_lengths_at_the_edge(fam, length, plan, monkeypatch):
    cfg = _edge_cfg(fam, length)
    tag = "%s, %s" % (cfg.name, rp.plan_id(plan))
    qos = fam == rp.QOS
    force_impl(monkeypatch, "persist")
    rp.set_plan(monkeypatch, cfg, plan)
    if qos:  # no persistent kernel serves it: its runs are launches of its step kernel
        plan = None
    dev, ora = rp.make_dev(cfg, 20), rp.Ora(cfg, 20, ledger=True)
    form = None if qos else "persist"
    rp.arm_log(dev, 4)
    every = _dones_per_step(cfg)
    total = 0
    for steps, hosts in ((5, 4), (1, 3), (12, 6)):
        rp.run_checked(dev, ora, cfg, form, plan, steps, tag)
        dones = rp.host_steps(dev, ora, cfg, hosts, tag)  # (reward, done and info of every env at every step)
        for t in range(hosts):
            want = every is not None and (total + steps + t + 1) % every == 0
            assert (dones[t] == want).all(), (tag, total + steps + t, dones[t])
        total += steps + hosts
        rp.compare(dev, ora, cfg, plan or ("128", 1), tag, "%d host steps" % hosts)
    counts = rp.compare_log(dev, ora, 4, tag + ", episode log")
    fresh = 1 if fam == "RMCSA" else 0  # (the step by which the first episode of a fresh RMCSA env is longer)
    assert (counts == (0 if every is None else (total - fresh) // every)).all()
    if fam in ("RMSA", "DeepRMSA", "RMCSA"):
        c = dev.counters()
        assert (c[:, 2] == (total + 1 if every is None else total % every + 1)).all()  # episode_services_processed, the pending one included
    rp.arm_log(dev, 0)
    dev.close()


@pytest.mark.parametrize("route", ["wave64", "split2", "persist", "agent8"])
def test_terminal_observation_when_every_step_is_terminal(route, monkeypatch):
    """DeepRMSA at episode_length=2: every step returns done, and the terminal-observation rows hold the observation of the step
    that ended the episode — which the soft reset behind it leaves as it is — at every step, for every env."""
    cfg = _edge_cfg("DeepRMSA", 2)
    force_impl(monkeypatch, route)
    dev, ora = rp.make_dev(cfg, 20), rp.Ora(cfg, 20)
    obs, tobs, done = dev.device_tensor("obs"), dev.device_tensor("terminal_obs"), dev.device_tensor("done")
    chk = _exact_bits("DeepRMSA, episode_length=2, %s" % route)
    for t in range(12):
        a = ora.policy(cfg.policy)
        dev.step(a, auto_reset=True, fetch=False)
        dev.sync()
        ora.step(a, auto_reset=True)
        assert done.cpu().numpy().astype(bool).all(), t
        chk(t, "terminal observation", tobs.cpu().numpy(), ora.observation())
        chk(t, "observation", obs.cpu().numpy(), ora.observation())
        chk(t, "a fresh observation()", dev.observation(), ora.observation())
    dev.close()


@pytest.mark.parametrize("fam", ["RMSA", "DeepRMSA", "RMCSA"])
def test_evaluate_refuses_an_episode_that_never_ends(fam):
    import optical_rl_gym_amd as orl

    never = _edge_cfg(fam, 1)
    dev = rp.make_dev(never, 9)
    before = rp.snapshot(dev, fam, 9)
    with pytest.raises(ValueError, match="never returns done"):
        dev.evaluate(never.policy, 3)
    with pytest.raises(ValueError, match="never returns done"):
        orl.evaluate_heuristic(dev, never.policy, n_eval_episodes=3)
    after = rp.snapshot(dev, fam, 9)
    chk = _exact_bits("%s, episode_length=1, after the refusal" % fam)
    for what in before:
        chk(0, what, after[what], before[what])
    dev.run(never.policy, 5)  # (and no log was left armed: the batch runs on)
    dev.close()
    one = _edge_cfg(fam, 2)  # one-step episodes: the shortest evaluate() can play
    dev = rp.make_dev(one, 9)
    ora = rp.Ora(one, 9, ledger=True)
    rewards, lengths = dev.evaluate(one.policy, 4)
    ora.reset(full=False)
    ora.run(one.policy, 4)
    accepted = np.array([e[:4] for e in ora.episodes], np.float64)
    assert (lengths == 1).all() and np.array_equal(rewards, 2.0 * accepted - 1 if fam == "DeepRMSA" else accepted)
    dev.close()


# ---- 5. resets between runs, every form, the batch in two halves --------------------------------------------------------------
RESETS = [(name, form) for name in ("rmsa", "deeprmsa", "rwa", "rmcsa") for form in rp.forms_of(name)]


@pytest.mark.parametrize("name,form", RESETS, ids=["%s-%s" % r for r in RESETS])
def test_full_and_masked_resets_between_runs_in_two_halves(name, form, monkeypatch):
    """tests/test_gpu_parity.py::test_full_and_masked_resets_match_oracle in every form of the persistent kernel (k_reset also drops
    parked look-ahead services and row-cache stamps, which the forms use differently), 20 envs as halves of 16 and 4: a full reset
    of envs on both sides of the split, and a soft reset of exactly the second half."""
    from oracle.oracle import OracleBatch

    plan = ("7", 2)
    cfg = rp.CONFIGS[name]
    force_impl(monkeypatch, form)
    rp.set_plan(monkeypatch, cfg, plan)
    dev = rp.make_dev(cfg, 20)
    ora = OracleBatch(cfg.fam, rp.TOPO, rp.seeds_of(cfg, 20), **cfg.kw)
    both, second = rp.reset_masks(20)
    assert both[:16].any() and both[16:].any() and not second[:16].any() and second[16:].all()
    tag = "%s, %s, %s" % (name, form, rp.plan_id(plan))

    def after_run(steps):
        rp.assert_plan(dev, cfg, plan, steps, tag)
        rp.assert_form_ran(dev, cfg, form, tag)

    resets_between_runs(dev, ora, cfg.policy, [both, second], _exact_bits(tag), sample=range(20), after_run=after_run)
    dev.close()
