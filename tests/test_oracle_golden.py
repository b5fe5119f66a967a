"""Pins the CPU oracle (oracle/orl_oracle.c) to the reference: every golden trace captured by
importing the reference (oracle/gen_golden.py) must be reproduced bit-for-bit — integers with ==,
float64 values with == as well (the oracle uses the same libm and the same operation order)."""
import numpy as np
import pytest

from oracle.oracle import OracleBatch
from tests.helpers import golden_names, load_golden, replay, replay_h, replay_q, replay_v, replay_w


def _make(meta):
    kw = dict(meta["kwargs"])
    seed = kw.pop("seed")
    return OracleBatch(meta["env"], meta["topology"], [seed], **kw)


def _exact(name):
    def check(t, what, got, exp):
        if got is None:
            return
        got, exp = np.asarray(got), np.asarray(exp)
        if got.dtype.kind == "f" or exp.dtype.kind == "f":
            ok = np.array_equal(got.astype(np.float64), exp.astype(np.float64), equal_nan=True)
        else:
            ok = np.array_equal(got, exp)
        assert ok, "%s: step %d: %s differs\n got %r\n exp %r" % (name, t, what, got, exp)
    return check


@pytest.mark.parametrize("name", golden_names())
def test_oracle_reproduces_reference_trace(name):
    g = load_golden(name)
    env = _make(g["meta"])
    replay(env, g, _exact(name))


@pytest.mark.parametrize("name", golden_names("w"))
def test_oracle_reproduces_wrapper_and_event_fixtures(name):
    """PathOnlyFirstFitAction, SimpleMatrixObservation, the 2-D action histograms, seed() and reset(full) mid-run, as
    captured from the reference by oracle/gen_golden_wrappers.py."""
    g = load_golden(name)
    env = _make(g["meta"])
    replay_w(env, g, _exact(name))


def test_oracle_reproduces_rmcsa_4d_action_histograms():
    """RMCSAEnv.actions_output / actions_taken (rmcsa_env.py:145-180, 219, 273, 284-289; cleared by a full reset, :437-454)."""
    g = load_golden("h1_rmcsa_hist4d")
    replay_h(_make(g["meta"]), g, _exact("h1_rmcsa_hist4d"))


@pytest.mark.parametrize("name", golden_names("q"))
def test_oracle_reproduces_qos_fixtures(name):
    """QoSConstrainedRA (qos_constrained_ra.py) as captured from the reference with its constructor repaired at import
    time (oracle/gen_golden_qos.py): three heuristics and a stored action stream, three service classes."""
    g = load_golden(name)
    env = _make(g["meta"])
    replay_q(env, g, _exact(name))


@pytest.mark.parametrize("name", golden_names("v"))
def test_oracle_reproduces_seed_fixtures(name):
    """seed() on a live env of the families and the bit-rate mode the w3 fixtures leave out (oracle/gen_golden_seed.py):
    DeepRMSA with its observation, RMSA with discrete bit rates, RMCSA — whose bit rates stay on the constructor's stream
    (rmsa_env.py:85-87 / 97-99, rmcsa_env.py:87-99) — and QoSConstrainedRA, which binds nothing."""
    g = load_golden(name)
    replay_v(_make(g["meta"]), g, _exact(name))


SEED_FIXTURES = {"v1_seed_deeprmsa": 640, "v1_seed_rmsa_discrete": 640, "v1_seed_rmcsa": 0, "v1_seed_qos": 0}
SEED_FIXTURES_LATE = ["v2_seed_deeprmsa_late", "v2_seed_rmsa_discrete_late", "v2_seed_rmcsa_late", "v2_seed_qos_late"]


def _events(meta):
    return {int(k): [tuple(e) for e in v] for k, v in meta["events"].items()}


def test_seed_fixtures_hold_every_event():
    """What the v1 fixtures were recorded for is in them: a seed before the first step, one in mid-episode, later ones, None, a
    seed in the step of a full reset, a negative seed, one >= 2**32; and, where the bit-rate stream must be seen regenerating
    (624 words of state, at least one word per service), at least 640 services after the first seed.  The v2 fixtures have
    their first seed in mid-episode, so that steps on the constructor's generator come before it."""
    assert golden_names("v") == sorted(list(SEED_FIXTURES) + SEED_FIXTURES_LATE)
    for name, least in SEED_FIXTURES.items():
        g = load_golden(name)
        meta = g["meta"]
        events = _events(meta)
        seeds = [(t, arg) for t, ev in sorted(events.items()) for kind, arg in ev if kind == "seed"]
        alone = [t for t, _arg in seeds if all(kind == "seed" for kind, _a in events[t])]
        episode_starts = set(int(t) + 1 for t in np.flatnonzero(g["done"])) | {0}
        assert seeds[0][0] == 0 == meta["first_seed_step"], name
        assert any(t > 0 and t not in episode_starts for t in alone), name  # in mid-episode
        assert len(seeds) >= 3, name
        assert any(arg is None for _t, arg in seeds), name
        assert any(arg is not None and arg < 0 for _t, arg in seeds), name
        assert any(arg is not None and arg >= 2**32 for _t, arg in seeds), name
        assert any({"seed", "full_reset"} <= {kind for kind, _a in ev} for ev in events.values()), name
        assert max(events) < meta["n_steps"], name
        assert meta["services_after_first_seed"] >= least, name
        assert meta["n_steps"] - seeds[0][0] >= least, name  # (every step draws one service)
    for name in SEED_FIXTURES_LATE:
        g = load_golden(name)
        first = g["meta"]["first_seed_step"]
        assert first >= 37 and not g["done"][first - 1] and len(_events(g["meta"])) >= 3, name
