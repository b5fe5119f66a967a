"""Spectrum-assignment rules for RMSA and RWA actions on the device (include/orl.h, orl_batch_assign_spectrum; k_assign_spectrum in
csrc/orl_assign.h) against the numpy restatement (tests/assign_restate.py, pinned to the oracle's step in
tests/test_assign_spectrum.py) on every env, from every source of the path, against the step itself, under graph capture, over a
sharded batch and through the VecEnv's path-only action space."""
import functools

import numpy as np
import pytest

from tests import assign_cases as ac
from tests import assign_restate as ar
from tests.oracle_backend import OracleBackend

pytestmark = pytest.mark.gpu

K = ac.K
NAMES = [s.name for s in ac.SHAPES]
ROW_WORDS = {64: 1, 65: 2, 128: 2, 129: 5, 321: 8, 512: 8}


def _make(shape, n=None, seeds=None, **extra):
    import optical_rl_gym_amd as orl

    seeds = ac.seeds_of(shape) if seeds is None else seeds
    return orl.make(shape.fam, topology=shape.topology, num_envs=len(seeds) if n is None else n, seeds=seeds, **dict(shape.kw, **extra))


def _rows(got, want, what, given=None):
    assert got.shape == want.shape and got.dtype == np.int32, what
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, "%s: %d envs differ, first %d: given %r, got %r, want %r" % (
        what, len(bad), bad[0], None if given is None else given[bad[0]], got[bad[0]], want[bad[0]])


def _check(env, shape, what, rng, seen, sources=False):
    """Every env, all six rules, both n_given against the restatement, with no state byte or flag changed; sources: the path also
    from column 0 of the actions tensor as torch wrote it, and the answer read from that tensor after fetch=False."""
    import torch

    avail, services = ac.state_of(env, shape)
    snap, flags = env.get_state(), env.flags().copy()
    acts, s = env.device_tensor("actions"), env.torch_stream()
    for rule, g, given, want in ac.expected(shape, avail, services, rng, seen)[0]:
        _rows(env.assign_spectrum(rule, paths=given, n_given=g), want, "%s, %s, n_given = %d, host paths" % (what, rule, g), given)
        if sources:
            with torch.cuda.stream(s):
                acts.fill_(-7)
                if g:
                    acts[:, 0].copy_(torch.as_tensor(given, dtype=torch.int32, device=acts.device))
                assert env.assign_spectrum(rule, n_given=g, fetch=False) is None
            env.sync()
            _rows(acts.cpu().numpy(), want, "%s, %s, n_given = %d, device paths" % (what, rule, g), given)
            if g:
                with torch.cuda.stream(s):
                    acts.fill_(-7)
                    assert env.assign_spectrum(rule, paths=given, fetch=False) is None
                env.sync()
                _rows(acts.cpu().numpy(), want, "%s, %s, host paths, fetch=False" % (what, rule), given)
    assert np.array_equal(env.get_state(), snap) and np.array_equal(env.flags(), flags), what


@functools.lru_cache(maxsize=None)
def _walk(name):
    shape = ac.SHAPE_BY_NAME[name]
    env = _make(shape)
    assert env.lib.orl_batch_row_words(env._h) == ROW_WORDS[shape.S]
    rng, seen = np.random.default_rng(shape.S), {}
    _check(env, shape, "after construction", rng, seen)
    ac.agent_steps(env, shape, ac.AGENT_STEPS, np.random.RandomState(shape.S))
    _check(env, shape, "after %d agent steps" % ac.AGENT_STEPS, rng, seen)
    # crowded maps under the same pending services, through a snapshot (no step follows: the snapshot is put back)
    snap = env.get_state()
    avail, services = ac.state_of(env, shape)
    crowded = ac.crowd(shape, avail, services)
    ac.set_maps(env, snap, crowded)
    assert np.array_equal(ac.state_of(env, shape)[0], crowded)
    _check(env, shape, "on crowded maps", rng, seen, sources=True)
    env.set_state(snap)
    env.reset(full=True)
    _check(env, shape, "after a full reset", rng, seen)
    assert not (env.flags() & 2).any()
    env.check()
    env.close()
    return seen


@pytest.mark.parametrize("name", NAMES)
def test_rules_equal_restatement_on_every_env(name):
    """After construction, after the agent's steps, on crowded maps (there from every source of the path) and after a full reset.
    What the states hold is printed; tests/test_assign_spectrum.py establishes the kinds per family on the oracle."""
    seen = _walk(name)
    print(name, seen)
    assert seen.get("no_completion", 0) > 0 and seen.get("last_start", 0) > 0 and seen.get("later_path", 0) > 0, seen


def _compare(env, ora, what):
    assert np.array_equal(env.counters(), ora.counters()), what
    assert np.array_equal(env.services(), ora.services()), what
    assert np.array_equal(env.slots_packed(), ora.slots_packed()), what


@pytest.mark.parametrize("name", [s.name for s in ac.SHAPES if s.envs <= 24])
def test_assignment_then_step_equals_the_oracle_stepped_with_the_restatement(name):
    """assign_spectrum(rule, fetch=False); step(None) for 60 steps, the rule changing with the step, against an oracle env stepped
    with the restatement's action: reward, done, counters, slot maps and services of every env at every step."""
    shape = ac.SHAPE_BY_NAME[name]
    env, ora = _make(shape), OracleBackend(shape.fam, shape.topology, ac.seeds_of(shape), **shape.kw)
    topo = ac.topology(shape.topology)
    provisioned = 0
    for t in range(60):
        rule = ar.RULES[t % 6]
        avail, services = ac.state_of(ora, shape)
        want = ar.assign(ar.Prepared(ac.ENV_TYPE[shape.fam], avail, services, topo, K, shape.S), rule, 0)
        assert env.assign_spectrum(rule, fetch=False) is None
        _, r_d, d_d, _ = env.step(None, auto_reset=True)
        _, r_o, d_o, _ = ora.step(want, auto_reset=True)
        assert np.array_equal(r_d, r_o) and np.array_equal(d_d, d_o), (t, rule)
        _compare(env, ora, (t, rule))
        provisioned += int((want[:, 0] < K).sum())
    assert provisioned > 0 and not (env.flags() & 2).any()
    env.check()
    env.close()


@pytest.mark.parametrize("name", NAMES)
def test_captured_assignment_and_step(name):
    """One single-stream graph of {assign_spectrum(n_given=1, paths=None); step(None)}, the path column rewritten by torch between
    the replays: 20 replays against the oracle stepped with the restatement's action."""
    import torch

    shape = ac.SHAPE_BY_NAME[name]
    rule = ar.RULES[(NAMES.index(name) + 2) % 6]
    env, ora = _make(shape), OracleBackend(shape.fam, shape.topology, ac.seeds_of(shape), **shape.kw)
    topo = ac.topology(shape.topology)
    acts, s = env.device_tensor("actions"), env.torch_stream()
    rew, done = env.device_tensor("reward"), env.device_tensor("done")
    rng = np.random.default_rng(shape.S + 1)

    def load():
        avail, services = ac.state_of(ora, shape)
        paths = ac.draw_paths(services, topo, rng)
        with torch.cuda.stream(s):
            acts[:, 0].copy_(torch.as_tensor(paths, dtype=torch.int32, device=acts.device))
        env.sync()
        return ar.assign(ar.Prepared(ac.ENV_TYPE[shape.fam], avail, services, topo, K, shape.S), rule, 1, paths)

    def oracle_step(want, what):
        _, r, d, _ = ora.step(want, auto_reset=True)
        assert np.array_equal(rew.cpu().numpy(), r) and np.array_equal(done.cpu().numpy().astype(bool), np.asarray(d).astype(bool)), what
        assert np.array_equal(acts.cpu().numpy(), want), what
        _compare(env, ora, what)

    want = load()  # (the first call comes before the capture: nothing is allocated inside)
    with torch.cuda.stream(s):
        env.assign_spectrum(rule, n_given=1, fetch=False)
        env.step(None, auto_reset=True, fetch=False)
    torch.cuda.synchronize()
    oracle_step(want, "eager")
    g = torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=s):
        env.assign_spectrum(rule, n_given=1, fetch=False)
        env.step(None, auto_reset=True, fetch=False)
    torch.cuda.synchronize()
    for it in range(20):
        want = load()
        g.replay()
        torch.cuda.synchronize()
        oracle_step(want, "replay %d" % it)
    assert not (env.flags() & 2).any()
    env.check()
    env.close()


@pytest.mark.parametrize("fam,kw", [("DeepRMSA", dict(mean_service_holding_time=7.5, mean_service_inter_arrival_time=1.0 / 12.0, j=2, episode_length=50)),
                                    ("RMCSA", dict(load=100, num_spectrum_resources=64, num_spatial_resources=7)),
                                    ("QoSConstrainedRA", dict(load=10))])
def test_other_families_refuse_the_rules(fam, kw):
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd._lib import OrlError

    env = orl.make(fam, topology="nsfnet_chen", num_envs=16, seeds=list(range(16)), **kw)
    snap = env.get_state()
    acts = env.device_tensor("actions").cpu().numpy().copy()
    for fetch in (True, False):
        for rule in ar.RULES:
            with pytest.raises(OrlError, match="RMSA and RWA only"):
                env.assign_spectrum(rule, fetch=fetch)
        with pytest.raises(OrlError, match="RMSA and RWA only"):
            env.assign_spectrum("best", paths=np.zeros(16, np.int32), fetch=fetch)
    env.sync()
    assert np.array_equal(env.get_state(), snap) and np.array_equal(env.device_tensor("actions").cpu().numpy(), acts)  # nothing was queued
    env.reset(full=True)  # (still usable)
    env.check()
    env.close()


def test_arguments_are_checked():
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd._lib import OrlError

    shape = ac.SHAPE_BY_NAME["rmsa_nsf_s64"]
    env = _make(shape, seeds=list(range(16)))
    env.assign_spectrum()
    acts = env.device_tensor("actions").cpu().numpy().copy()
    ok = np.zeros(16, np.int32)
    for fetch in (True, False):
        for rule in (-1, 6, 99):
            with pytest.raises(OrlError, match="unknown spectrum-assignment rule"):
                env.assign_spectrum(rule, fetch=fetch)
        for g in (-1, 2):
            with pytest.raises(OrlError, match="outside 0 .. 1"):
                env.assign_spectrum("best", n_given=g, fetch=fetch)
            with pytest.raises(OrlError, match="outside 0 .. 1"):
                env.assign_spectrum("best", paths=ok, n_given=g, fetch=fetch)
        with pytest.raises(OrlError, match="n_given == 0"):
            env.assign_spectrum("best", paths=ok, n_given=0, fetch=fetch)
    with pytest.raises(ValueError):
        env.assign_spectrum("worst")
    for bad in (np.zeros((16, 1), np.int32), np.zeros(15, np.int32), np.zeros(16, np.float64)):
        with pytest.raises(ValueError):
            env.assign_spectrum("best", paths=bad)
    env.sync()
    assert np.array_equal(env.device_tensor("actions").cpu().numpy(), acts)  # nothing was queued
    assert env.assign_spectrum("last", paths=np.zeros(16, np.int64)).shape == (16, 4)
    env.step(None, auto_reset=True)  # (still usable)
    env.check()
    env.close()
    for cls, kw in ((orl.RMSAEnv, dict(load=100, num_spectrum_resources=64)), (orl.RWAEnv, dict(load=100, num_spectrum_resources=64))):
        one = cls(topology="nsfnet_chen", seed=3, **kw)
        one.reset()
        full = one.assign_spectrum("last")
        assert isinstance(full, tuple) and len(full) == 2 and all(isinstance(v, int) for v in full)
        assert full == tuple(int(v) for v in one.batch.assign_spectrum("last")[0][:2])
        assert full != (K, 64) and one.assign_spectrum("last", path=full[0]) == full
        assert one.assign_spectrum("first", path=K) == (K, 64) and one.assign_spectrum("first", path=-1) == (K, 64)
        one.close()


def test_multi_device_batch_cuts_paths_by_shard():
    from optical_rl_gym_amd.sharding import MultiDeviceBatch

    shape = ac.SHAPE_BY_NAME["rmsa_nsf_s65"]
    n, cut = 200, 72
    seeds = list(range(40, 40 + n))
    whole = _make(shape, seeds=seeds)
    multi = MultiDeviceBatch.from_shards([_make(shape, seeds=seeds[:cut]), _make(shape, seeds=seeds[cut:])])
    for t in range(20):
        a = whole.policy("SAP_FF").copy()
        whole.step(a, auto_reset=True)
        multi.step(a, auto_reset=True)
    avail, services = ac.state_of(whole, shape._replace(envs=n))
    topo = ac.topology(shape.topology)
    prep = ar.Prepared(0, avail, services, topo, K, shape.S)
    for rule in ("best", "most_used"):
        given = ac.draw_paths(services, topo, np.random.default_rng(3))
        want = whole.assign_spectrum(rule, paths=given)
        _rows(want, ar.assign(prep, rule, 1, given), rule, given)
        assert np.array_equal(multi.assign_spectrum(rule, paths=given), want), rule
        assert np.array_equal(np.concatenate([sh.assign_spectrum(rule, paths=given[lo:hi]) for sh, lo, hi in
                                              zip(multi.shards, (0, cut), (cut, n))]), want), rule
        assert multi.assign_spectrum(rule, paths=given, fetch=False) is None
        for sh in multi.shards:
            sh.sync()
        assert np.array_equal(np.concatenate([sh.device_tensor("actions").cpu().numpy() for sh in multi.shards]), want), rule
        assert np.array_equal(multi.assign_spectrum(rule), whole.assign_spectrum(rule)), rule
        with pytest.raises(ValueError):
            multi.assign_spectrum(rule, paths=given[:cut])
    multi.close()
    whole.close()


@pytest.mark.parametrize("allow_rejection", [False, True])
def test_vec_env_path_only_action_space(allow_rejection):
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd.vec_env import OpticalVecEnv

    n, S = 32, 24
    shape = ac.Shape("rmsa_small", "RMSA", "nsfnet_chen", S, n, dict(load=400, num_spectrum_resources=S, allow_rejection=allow_rejection,
                                                                    mean_service_holding_time=10.0, episode_length=50))
    env = _make(shape, seeds=list(range(900, 900 + n)))
    topo = ac.topology(shape.topology)
    rmcsa = orl.make("RMCSA", topology="nsfnet_chen", num_envs=8, seeds=list(range(8)), load=100, num_spectrum_resources=64, num_spatial_resources=7)
    with pytest.raises(ValueError, match="RMSA and RWA"):
        OpticalVecEnv(rmcsa, spectrum_assignment="best")
    rmcsa.close()
    with pytest.raises(ValueError):
        OpticalVecEnv(env, spectrum_assignment="worst")
    plain = OpticalVecEnv(env)
    assert hasattr(plain.action_space, "nvec") and plain.spectrum_assignment is None  # (the default: nothing changes)
    venv = OpticalVecEnv(env, spectrum_assignment="best")
    assert int(venv.action_space.n) == K + 1 and not hasattr(venv.action_space, "nvec")
    venv.reset()
    rng = np.random.default_rng(5)
    kinds = [0, 0]
    for t in range(30):
        avail, services = ac.state_of(env, shape)
        prep = ar.Prepared(0, avail, services, topo, K, S)
        fit = ar.path_fits(prep)
        fb = ~fit.any(axis=1)
        want = np.concatenate([fit, np.full((n, 1), allow_rejection)], axis=1)
        if not allow_rejection:
            want[fb, :-1] = True  # the fallback row
        masks = venv.action_masks()
        assert masks.shape == (n, K + 1) and masks.dtype == np.bool_ and np.array_equal(masks, want), t
        # a set path column, uniformly; the reject column (set, as allow_rejection is on, but never preferred) where there is none
        actions = np.array([rng.choice(np.flatnonzero(row[:K])) if row[:K].any() else K for row in masks])
        if t % 10 == 9:
            actions[0] = K  # the reject action of the path-only space
            fb[0] = True
        chosen = ar.assign(prep, "best", 1, np.minimum(actions, K).astype(np.int32))
        before = env.counters()[:, 1].copy()
        venv.step_async(actions)
        venv.step_wait()
        assert np.array_equal(env.device_tensor("actions").cpu().numpy(), chosen), t
        assert np.array_equal(env.counters()[:, 1] - before, (~fb).astype(np.int64)), t
        kinds[0] += int(fb.sum())
        kinds[1] += int((~fb).sum())
    print("rows without / with a fit:", kinds)
    assert min(kinds) > 0 and not (env.flags() & 2).any()
    env.check()
    venv.close()
