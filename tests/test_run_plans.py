"""The CPU side of tests/test_run_plans_gpu.py (tests/run_plans.py holds the table both share).  The plan: for every (batch, plan)
pair the GPU module runs, under every form's environment, orl_debug_run_plan gives the parts, the split point and the launch length
the table states, and the pure form choice gives the form the GPU case asserts.  The matrix: the subset of the cross product covers
what it must.  The oracle alone: its trajectories over the steps a GPU case runs show, in BOTH halves of the batch, what the checks
of the second half's per-env arrays need in order not to pass trivially — printed as observed.  And evaluate() refuses a
configuration whose episodes never end."""
import os
import shutil

import numpy as np
import pytest

from tests import run_plans as rp
from tests.helpers import force_impl

needs_lib = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")

MATRIX = rp.matrix()


def _derived(cfg, n):
    """the configuration as the C ABI takes it, without a device (per-env loads: the scalar pair of the largest, as a batch's)"""
    from optical_rl_gym_amd.envs import ENV_CLASSES

    kw = rp.dev_kwargs(cfg, n)
    if cfg.loads:
        kw["load"] = max(cfg.loads(n))
    return ENV_CLASSES[cfg.fam]._derived(topology=rp.TOPO, **kw)


# ---- the matrix ---------------------------------------------------------------------------------------------------------------
def test_matrix_covers_what_it_must():
    assert len(MATRIX) == len(set(MATRIX)) and len(MATRIX) <= 150
    full = {(c.form, c.plan) for c in MATRIX if c.config == "rmsa" and c.n == 20}
    assert full == {(f, p) for f in rp.FORMS for p in rp.PLANS}
    two = [c for c in MATRIX if rp.expected_split(c.n, c.plan)[0] == 2]
    assert {c.config for c in two} == set(rp.MATRIX_CONFIGS)
    assert {c.form for c in two} == set(rp.FORMS)
    assert {c.plan for c in two} == {p for p in rp.PLANS if p[1] == 2}
    assert {c.n for c in two} == {20, 9, 64}
    assert any(c.n == 8 and c.plan[1] == 2 for c in MATRIX)  # two parts asked of one wavefront: the fall-back
    assert {c.config for c in two if c.plan[0] == "L"} == set(rp.MATRIX_CONFIGS)
    assert {c.config for c in MATRIX if c.form == "persist_pair"} == set(rp.PAIR_CONFIGS)
    for name in rp.MATRIX_CONFIGS:  # every plan is a launch length of its own
        L = rp.steps_per_episode(rp.CONFIGS[name])
        assert 12 <= rp.CONFIGS[name].kw["episode_length"] <= 30
        assert len({rp.chunk_of(p, L) for p in rp.PLANS}) == 6 and L - 1 > 7
    print("%d cases, %d of them in two halves" % (len(MATRIX), len(two)))


def test_batch_table_is_the_split_rule():
    """halves of 16 and 4, 8 and 1, 32 and 32; one wavefront stays whole (wavefronts own 8 consecutive envs)"""
    for n, (first, second) in rp.BATCHES.items():
        n_wg = (n + 7) // 8
        assert first + second == n
        assert (first, second) == (((n_wg + 1) // 2 * 8, n - (n_wg + 1) // 2 * 8) if n_wg >= 2 else (n, 0))


@needs_lib
@pytest.mark.parametrize("form", rp.FORMS)
def test_every_pair_of_batch_and_plan_gives_the_plan_of_the_table(form, monkeypatch):
    force_impl(monkeypatch, form)
    seen = 0
    extra = [rp.Case(name, form, plan, 20) for name in rp.CONFIGS if name != "qos" for plan in rp.PLANS if form in rp.forms_of(name)]
    for c in dict.fromkeys([c for c in MATRIX if c.form == form] + extra):
        cfg = rp.CONFIGS[c.config]
        L = rp.steps_per_episode(cfg)
        rp.set_plan(monkeypatch, cfg, c.plan)
        env = _derived(cfg, c.n)
        parts, half = rp.expected_split(c.n, c.plan)
        for steps in rp.run_lengths(L) + [130, 220]:
            for tuned in (False, True):
                for have in (0, 2, 256):  # whatever statistics log an earlier run left
                    p = dict(zip(env.RUN_PLAN_FIELDS, env.run_plan(c.n, steps, tuned=tuned, log_cap_have=have)))
                    what = (rp.case_id(c), steps, tuned, have, p)
                    assert p["persist"] == 1 and p["two_kernel"] == 0, what
                    assert (p["parts"], p["half"]) == (parts, half), what
                    assert p["chunk"] == rp.chunk_of(c.plan, L), what
                    seen += 1
        tuned = form == "persist_pair"
        choice = dict(zip(env.PERSIST_CHOICE_FIELDS, env.persist_choice(c.n, tuned=tuned)))
        want = rp.expected_form(cfg, form)
        assert want is None or choice["form"] == want, (rp.case_id(c), choice)
        if form == "persist_pair":
            assert choice["rw"] == (cfg.fam != "RMCSA"), (rp.case_id(c), choice)
    assert seen
    # without the overrides none of these batches would run in two halves: the GPU cases must fail if they are ignored
    monkeypatch.delenv("ORL_PERSIST_CHUNK")
    monkeypatch.delenv("ORL_PERSIST_PARTS")
    p = dict(zip(env.RUN_PLAN_FIELDS, _derived(rp.CONFIGS["rmsa"], 64).run_plan(64, 300)))
    assert (p["parts"], p["half"], p["chunk"]) == (1, 64, 128)


# ---- the oracle alone ---------------------------------------------------------------------------------------------------------
def _halves(n):
    first, _second = rp.BATCHES[n]
    return range(first), range(first, n)


def _cells(hist):
    out, taken = hist
    return set(map(tuple, np.argwhere(np.asarray(out) != 0))) | {("taken",) + tuple(c) for c in np.argwhere(np.asarray(taken) != 0)}


CONDITION_CASES = [(name, n) for name in rp.CONFIGS for n in ((20, 9, 64) if name in rp.MATRIX_CONFIGS else (20,))]


@pytest.mark.parametrize("name,n", CONDITION_CASES, ids=["%s-%d" % c for c in CONDITION_CASES])
def test_oracle_trajectories_give_both_halves_something_to_get_wrong(name, n):
    cfg = rp.CONFIGS[name]
    ora = rp.Ora(cfg, n, ledger=True)
    rp.drive_oracle(ora, cfg)
    first, second = _halves(n)
    episodes = [len(e) for e in ora.episodes]
    c = ora.counters()
    print("%s, %d envs: episodes finished per env %d..%d, envs with an accepted-and-rejected episode %d + %d, accepted %d of %d services"
          % (name, n, min(episodes), max(episodes), ora.mixed[list(first)].sum(), ora.mixed[list(second)].sum(), c[:, 1].sum(), c[:, 0].sum()))
    for half in (first, second):
        assert max(episodes[i] for i in half) > rp.SMALL_CAP
        assert any(ora.mixed[i] for i in half)
    if cfg.kw.get("bit_rate_selection") == "discrete":
        seen = set().union(*[ora.rates_seen[i] for i in second])
        print("   bit rates requested in the second half: %s" % sorted(seen))
        assert seen == {10, 40, 100}
    if cfg.dev_kw.get("action_histograms"):
        in_first = set().union(*[_cells(ora.action_histograms_of(i)) for i in first])
        own = [len(_cells(ora.action_histograms_of(i)) - in_first) for i in second]
        print("   action-histogram cells of second-half envs that no first-half env has: %s" % own)
        assert max(own) > 0
        if n == 20:  # ... and not even the env 16 rows further down, whose rows a missing offset would show
            assert all(_cells(ora.action_histograms_of(i)) != _cells(ora.action_histograms_of(i - 16)) for i in second)
    if cfg.loads:
        loads = np.array(cfg.loads(n))
        new, mask = rp.set_load_change(n)
        after = np.where(mask != 0, new, loads)
        print("   loads %s -> %s" % (loads.tolist(), after.tolist()))
        for values in (loads, after):
            assert not set(values[list(first)]) & set(values[list(second)])
        assert mask[list(first)].any() and mask[list(second)].any() and not mask.all()
    if cfg.paths:
        paths = cfg.paths(n)
        assert set(paths) == set(range(6)) and all(paths[i] != paths[i - 16] for i in second)


def test_oracle_at_episode_lengths_1_and_2():
    """done and the episode counters as the reference lines give them (rmsa_env.py:280, 314, 576; rwa_env.py:135-136, 160): the
    fixtures g10_* / q2_* pin the same through tests/test_oracle_golden.py"""
    from tests.helpers import load_golden

    for name, dones in (("g10_rmsa_len1_sapff", 0), ("g10_deeprmsa_len1_sap", 0), ("g10_rmsa_len2_sapff", 48), ("g10_deeprmsa_len2_sap", 48),
                        ("g10_rmcsa_len2_sapff", 48), ("g10_rmsa_len3_sapff", 24), ("g10_deeprmsa_len3_sap", 24), ("g10_rwa_len1_sapff", 48),
                        ("g10_rwa_len2_sapff", 24), ("q2_qos_len1_sapff", 48), ("q2_qos_len2_sapff", 24)):
        g = load_golden(name)
        assert g["meta"]["n_steps"] == 48 and int(g["done"].sum()) == dones, name
        assert os.path.getsize(os.path.join(rp.__file__.rsplit(os.sep, 1)[0], "golden", name + ".npz")) < 100 * 1024


# ---- evaluate() where an episode never ends -------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,kw", [("RMSA", {}), ("DeepRMSA", {}), ("RMCSA", dict(num_spatial_resources=7))])
def test_evaluate_refuses_an_episode_that_never_ends(fam, kw):
    import optical_rl_gym_amd as orl
    from tests.oracle_backend import OracleBackend

    ora = OracleBackend(fam, rp.TOPO, [3, 4], episode_length=1, **kw)
    before = ora.counters().copy()
    policy = "SAP" if fam == "DeepRMSA" else "SAP_FF"
    with pytest.raises(ValueError, match="never returns done"):
        ora.evaluate(policy, 2)
    with pytest.raises(ValueError, match="episode_length=1"):
        orl.evaluate_heuristic(ora, policy, n_eval_episodes=2)
    assert np.array_equal(ora.counters(), before)
    ok = OracleBackend(fam, rp.TOPO, [3, 4], episode_length=2, **kw)  # one-step episodes: the shortest that end
    rewards, lengths = ok.evaluate(policy, 3)
    assert rewards.shape == (2, 3) and (lengths == 1).all()


@needs_lib
@pytest.mark.parametrize("fam", ["RMSA", "DeepRMSA", "RMCSA"])
def test_batch_evaluate_refuses_before_it_touches_the_batch(fam):
    """BatchedOpticalEnv.evaluate on a configuration object without a batch behind it: the refusal comes before the first call
    into the library (anything else would fail on the missing handle)"""
    from optical_rl_gym_amd.envs import ENV_CLASSES

    env = ENV_CLASSES[fam]._derived(topology=rp.TOPO, episode_length=1)
    assert env._h is None and env.steps_per_episode() == 0
    with pytest.raises(ValueError, match="never returns done"):
        env.evaluate("SAP" if fam == "DeepRMSA" else "SAP_FF", 2)
    for fam2 in ("RWA", "QoSConstrainedRA"):  # these count at the decision: every step is terminal, nothing to refuse
        assert ENV_CLASSES[fam2]._derived(topology=rp.TOPO, episode_length=1).steps_per_episode() == 1
