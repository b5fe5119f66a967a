"""Per-env traffic load and set_load, host side (no GPU): the rates the constructors and set_load hand to the C ABI are the
reference's own expressions evaluated per env (optical_network_env.py:92-94, rmsa_env.py:548-553), bad arguments are refused
before any ABI call, the s1_* fixtures (tools/gen_golden_set_load.py) carry their schedule and come from the same reference as
the g* / q* ones, and a multi-device batch cuts per-env arguments per shard."""
import json

import numpy as np
import pytest

from tests.helpers import load_golden, replay, replay_q

S1 = ["s1_rmsa_set_load", "s1_deeprmsa_set_load", "s1_rwa_set_load", "s1_rmcsa_set_load", "s1_qos_set_load"]


def _derive(cls, num_envs, **kw):
    """A batch object that stopped before the ABI (what spec_flags() builds): its configuration and its rate arrays."""
    self = cls.__new__(cls)
    self._derive_only = True
    self.__init__(topology="nsfnet_chen", num_envs=num_envs, **kw)
    return self


def _reference_rates(load, mht):
    miat = 1 / float(load / float(mht))
    return miat, 1 / miat, 1 / mht


def test_array_load_gives_the_reference_expressions_per_env():
    from optical_rl_gym_amd import envs

    loads = [100, 150.5, 300, 399.999, 60, 1e-3, 7, 250]
    mhts = [25, 10.0, 7.5, 33, 10800.0, 1, 25, 12.5]
    for cls in (envs.BatchedRMSAEnv, envs.BatchedRWAEnv, envs.BatchedRMCSAEnv, envs.BatchedQoSConstrainedRA):
        for load, mht in ((loads, 25), (np.array(loads), mhts), (300, mhts)):
            b = _derive(cls, 8, load=load, mean_service_holding_time=mht)
            la, lh = b._rate_arrays
            assert la.dtype == np.float64 and lh.dtype == np.float64 and la.shape == (8,) and lh.shape == (8,)
            for i in range(8):
                ld = load[i] if not np.isscalar(load) else load
                h = mht[i] if not np.isscalar(mht) else mht
                miat, ra, rh = _reference_rates(float(ld), float(h))
                assert la[i] == ra and lh[i] == rh and b.mean_service_inter_arrival_time[i] == miat
                assert b.load[i] == float(ld) and b.mean_service_holding_time[i] == float(h)
            for name in ("load", "mean_service_holding_time", "mean_service_inter_arrival_time"):
                v = getattr(b, name)
                assert isinstance(v, np.ndarray) and v.dtype == np.float64 and v.shape == (8,)
            # the configuration's scalar pair is that of the env with the largest load: it sizes the pending-release arrays
            top = int(np.argmax(la / lh))
            assert b._cfg.lambda_arrival == la[top] and b._cfg.lambda_holding == lh[top]


def test_deeprmsa_array_inter_arrival_time():
    from optical_rl_gym_amd import envs

    miats = [1.0 / 12.0, 0.1, 0.05, 0.2]
    mhts = [7.5, 25.0, 10.0, 7.5]
    for mht, miat in ((7.5, miats), (mhts, miats), (mhts, 0.1)):
        b = _derive(envs.BatchedDeepRMSAEnv, 4, mean_service_holding_time=mht, mean_service_inter_arrival_time=miat)
        la, lh = b._rate_arrays
        for i in range(4):
            h = float(mht[i] if not np.isscalar(mht) else mht)
            a = float(miat[i] if not np.isscalar(miat) else miat)
            load = h / a  # deeprmsa_env.py:25
            m, ra, rh = _reference_rates(load, h)
            assert b.load[i] == load and b.mean_service_inter_arrival_time[i] == m and la[i] == ra and lh[i] == rh


def test_scalar_arguments_take_the_scalar_path():
    from optical_rl_gym_amd import envs

    b = _derive(envs.BatchedRMSAEnv, 8, load=300, mean_service_holding_time=25)
    assert b._rate_arrays == (None, None)
    miat, ra, rh = _reference_rates(300, 25)
    assert b.load == 300 and b.mean_service_holding_time == 25 and b.mean_service_inter_arrival_time == miat
    assert np.isscalar(b.load) and np.isscalar(b.mean_service_inter_arrival_time)
    assert b._cfg.lambda_arrival == ra and b._cfg.lambda_holding == rh
    d = _derive(envs.BatchedDeepRMSAEnv, 4, mean_service_holding_time=7.5, mean_service_inter_arrival_time=1.0 / 12.0)
    assert d._rate_arrays == (None, None) and d.load == 7.5 / (1.0 / 12.0)


def test_rates_are_not_part_of_the_specialisation_flags():
    """A sweep builds one specialisation: the flags of a per-env batch are those of a uniform batch at its largest load (the
    pending-release capacity is the only thing the load decides), and two sweeps with the same largest load share them."""
    from optical_rl_gym_amd import envs

    kw = dict(topology="nsfnet_chen", mean_service_holding_time=25, num_spectrum_resources=320)
    cls = envs.BatchedRMSAEnv

    def flags(load, n):
        self = _derive(cls, n, load=load, **{k: v for k, v in kw.items() if k != "topology"})
        import ctypes as C
        buf = C.create_string_buffer(1024)
        n_ = self.lib.orl_spec_flags_for_batch(C.byref(self._cfg), C.byref(self._desc), 1 << 20, buf, len(buf))
        return buf.value.decode() if n_ > 0 else None

    uniform = flags(400, 1)
    assert uniform and flags([100, 400, 250, 175], 4) == uniform and flags([400, 399, 10, 20], 4) == uniform
    assert "lambda" not in uniform.lower() and flags(400, 1) == cls.spec_flags(load=400, **kw)


@pytest.mark.parametrize("bad", [[100, 200, 300], [[100, 200], [300, 400]], [100, 0, 300, 400], [100, -5, 300, 400],
                                 [100, float("nan"), 300, 400], [100, float("inf"), 300, 400]])
def test_bad_per_env_arguments_raise_before_the_abi(bad):
    from optical_rl_gym_amd import envs

    with pytest.raises(ValueError):
        _derive(envs.BatchedRMSAEnv, 4, load=bad, mean_service_holding_time=25)
    with pytest.raises(ValueError):
        _derive(envs.BatchedRMSAEnv, 4, load=300, mean_service_holding_time=bad)
    with pytest.raises(ValueError):
        _derive(envs.BatchedDeepRMSAEnv, 4, mean_service_inter_arrival_time=bad)
    b = _derive(envs.BatchedRMSAEnv, 4, load=300, mean_service_holding_time=25)
    with pytest.raises(ValueError):
        b._derive_set_load(load=bad)
    with pytest.raises(ValueError):
        b._derive_set_load(mean_service_holding_time=bad)
    assert b.load == 300 and b._h is None  # nothing changed, no handle was ever made


def test_set_load_derivation_follows_the_reference_rule_per_env():
    """A given load replaces the env's load, a given holding time its holding time, the inter-arrival mean follows from the
    env's (new or kept) pair; unselected envs keep everything (optical_network_env.py:86-94 per env)."""
    from optical_rl_gym_amd import envs

    b = _derive(envs.BatchedRMSAEnv, 4, load=[100, 200, 300, 400], mean_service_holding_time=25)
    mask = np.array([1, 0, 1, 0], np.uint8)
    load, mht, miat, la, lh, m = b._derive_set_load(load=[150, 999, 60, 999], mask=mask)
    assert list(load) == [150, 200, 60, 400] and list(mht) == [25, 25, 25, 25] and m is not None
    for i in range(4):
        mi, ra, rh = _reference_rates(float(load[i]), 25.0)
        assert miat[i] == mi and la[i] == ra and lh[i] == rh
    b.load, b.mean_service_holding_time = load, mht
    load2, mht2, miat2, la2, lh2, _ = b._derive_set_load(mean_service_holding_time=10.0, mask=mask)
    assert list(load2) == [150, 200, 60, 400] and list(mht2) == [10.0, 25, 10.0, 25]
    assert miat2[0] == _reference_rates(150.0, 10.0)[0] and miat2[1] == _reference_rates(200.0, 25.0)[0]
    with pytest.raises(ValueError):
        b._derive_set_load(load=100, mask=[1, 0, 1])
    # a uniform batch and a uniform change keep scalars
    u = _derive(envs.BatchedRMSAEnv, 4, load=300, mean_service_holding_time=25)
    load, mht, miat, la, lh, m = u._derive_set_load(load=400)
    assert load == 400 and mht == 25 and np.isscalar(miat) and m is None
    assert (la == _reference_rates(400, 25)[1]).all() and (lh == 1 / 25).all()
    with pytest.raises(ValueError):
        u._derive_set_load(load=0)
    with pytest.raises(ValueError):
        u._derive_set_load(mean_service_holding_time=float("nan"))


@pytest.mark.parametrize("name", S1)
def test_fixture_carries_its_schedule_and_starts_like_the_reference(name):
    """Every s1_* file loads with its schedule, and the oracle built with the initial kwargs reproduces the trace exactly up to
    the first scheduled step: the fixtures come from the same reference as the g* / q* ones."""
    from oracle.oracle import OracleBatch

    g = load_golden(name)
    sched = {int(k): v for k, v in json.loads(str(g["schedule"])).items()}
    assert len(sched) == 3 and all(set(v) <= {"load", "mean_service_holding_time"} for v in sched.values())
    after = g["after_change"]
    assert [int(r[0]) for r in after] == sorted(sched)
    for t, load, mht, miat in after:  # what the reference env held after each change: set_load's rule
        assert miat == 1 / float(load / float(mht))
        if "load" in sched[int(t)]:
            assert load == sched[int(t)]["load"]
        if "mean_service_holding_time" in sched[int(t)]:
            assert mht == sched[int(t)]["mean_service_holding_time"]
    first = min(sched)
    meta = g["meta"]
    kw = dict(meta["kwargs"])
    seed = kw.pop("seed")
    ora = OracleBatch(meta["env"], meta["topology"], [seed], **kw)

    def check(t, what, got, exp):
        got, exp = np.asarray(got), np.asarray(exp)
        assert np.array_equal(got, exp, equal_nan=got.dtype.kind == "f" and exp.dtype.kind == "f"), (name, t, what)

    if meta["env"] == "QoSConstrainedRA":
        g2 = dict(g, meta=dict(meta, n_steps=first, snapshot_steps=[]))
        g2["svc"] = g["svc"][: first + 1]
        replay_q(ora, g2, check)
    else:
        replay(ora, g, check, n_steps=first)
    # ... and the service drawn by step `first`, the first one under the new rates, is not the one the constant-load oracle draws
    check(first, "svc", ora.services()[0], g["svc"][first])
    ora.step(ora.policy(meta["policy"]))
    assert ora.services()[0][0] != g["svc"][first + 1][0]


def test_multi_device_batch_cuts_per_env_arguments():
    from optical_rl_gym_amd.sharding import cut_per_env_kwargs, shard_range

    names = ("load", "mean_service_holding_time", "mean_service_inter_arrival_time")
    kw = dict(load=np.arange(10, 20), mean_service_holding_time=25, episode_length=100)
    parts = []
    for r in range(3):
        lo, hi = shard_range(10, r, 3)
        cut = cut_per_env_kwargs(kw, names, 10, lo, hi)
        assert cut["mean_service_holding_time"] == 25 and cut["episode_length"] == 100 and len(cut["load"]) == hi - lo
        parts.append(cut["load"])
    assert np.array_equal(np.concatenate(parts), np.arange(10, 20))
    with pytest.raises(ValueError):
        cut_per_env_kwargs(dict(load=[1, 2, 3]), names, 10, 0, 4)
    with pytest.raises(ValueError):
        cut_per_env_kwargs(dict(load=np.ones((10, 2))), names, 10, 0, 4)


def test_multi_device_wrapper_over_oracle_shards_has_the_batch_surface():
    """MultiDeviceBatch.from_shards over oracle stand-ins: the methods exist and the per-env attributes concatenate (the oracle
    has one load per batch and no set_load of its own, so set_load itself is a GPU test)."""
    from optical_rl_gym_amd.sharding import MultiDeviceBatch
    from tests.oracle_backend import OracleBackend

    kw = dict(mean_service_holding_time=25, episode_length=50, num_spectrum_resources=64)
    a = OracleBackend("RMSA", "nsfnet_chen", [1, 2, 3], load=100, **kw)
    b = OracleBackend("RMSA", "nsfnet_chen", [4, 5], load=200, **kw)
    a.load, b.load = 100, 200
    m = MultiDeviceBatch.from_shards([a, b])
    assert list(m.load) == [100, 100, 100, 200, 200] and callable(m.set_load) and callable(m.rates)
    b.load = 100
    assert m.load == 100
    m.close()
