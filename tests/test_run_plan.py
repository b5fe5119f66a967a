"""The host-side decisions of the library, pinned case by case without a GPU (orl_debug_run_plan): the step route a batch takes at
creation (persistent kernel, two-kernel form, k_agent, item-mask limit) and the plan of a device-resident run (steps per launch,
one stream or two, the split point, the capacities of the logs, whether the step counters are cleared).  Every row of
tests/golden/run_plan.npz — configurations x library build x batch sizes x run lengths x batch states x overrides, recorded from
the statements as they stood in batch_create_impl, ensure_logs and orl_batch_run before they became pure functions
(tools/gen_golden_run_plan.py) — is recomputed with the library under test and compared with ==.  A slip here fails no other
test without a GPU: it costs a fault (a log that is not there), a silent 5-20 % (wrong chunk or parts), or a wrong kernel behind
a VecEnv."""
import json
import os
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


def _golden():
    d = np.load(os.path.join(ROOT, "tests", "golden", "run_plan.npz"))
    return np.ascontiguousarray(d["cols"].T), json.loads(str(d["meta"]))


def _rows_deferred(rows, meta, col):
    """Rows whose chosen form is rows-deferred: ORL_PERSIST_VARIANT=7 is set, and the form is possible (a single-core family the
    persistent kernel serves, at most 64 links — persist_rd_possible, csrc/orl_persist_form.h; every configuration of the grid has
    at most 512 slots; cfg4 and cfg4n are RMCSA, cfg5 has 88 links)."""
    forced = np.array([ov.get("ORL_PERSIST_VARIANT") == "7" for ov in meta["overrides"]])[rows[:, col["override"]]]
    fits = np.array([name not in ("cfg4", "cfg4n", "cfg5", "cfg2_e130")  for name in meta["configs"]])[rows[:, col["config"]]]
    return forced & fits & (rows[:, col["persist"]] == 1)


def test_fixture_reaches_every_decision():
    """What the grid must reach, whatever the library under test does."""
    import gen_golden_run_plan as gen

    rows, meta = _golden()
    col = {n: i for i, n in enumerate(meta["columns"])}
    ov = meta["overrides"]
    assert meta["configs"] == [c[0] for c in gen.configs()] and meta["libs"] == list(gen.LIBS) and ov == gen.OVERRIDES
    assert meta["n_cu"] == gen.N_CU and meta["run_base"] == list(gen.RUN_BASE)
    assert len(rows) == len(set(gen.grid())) and (rows[:, col["valid"]] == 1).all()
    import gen_golden_persist_choice as pc

    assert set(meta["configs"]) > {c[0] for c in pc.configs()} and {"qos_k9", "cfg2_e130"} <= set(meta["configs"])
    assert set(rows[:, col["batch"]]) == {64, 2047, 2048, 4096, 12288, 16376, 16384, 20479, 20480, 65536}
    assert set(rows[:, col["steps"]]) == {0, 1, 2, 20, 128, 129, 256, 257, 300, 3000}
    assert set(rows[:, col["log_cap_have"]]) == {0, 2, 12, 256} and set(rows[:, col["run_base"]]) == {0, 1} and set(rows[:, col["wg_dirty"]]) == {0, 1}
    assert meta["run_base"] == [0, (1 << 30) - 100] and set(rows[:, col["lib"]]) == {0, 1} and set(rows[:, col["tuned"]]) == {0, 1}
    # every variable unset, at both ends of its accepted range and just outside each end
    for var, values in (("ORL_ITEM_MASKS", "0 1 8 9"), ("ORL_PERSIST_CHUNK", "0 1 2147483647"), ("ORL_PERSIST_PARTS", "0 1 2 3"),
                        ("ORL_LOG_CAP", "1 2 256 257"), ("ORL_ELOG_CAP", "33 34 4096 4097"), ("ORL_RUN_BASE_LIMIT", "0 1 9223372036854775807"),
                        ("ORL_STEP_IMPL", "2 63 64"), ("ORL_PERSIST", "0 1"), ("ORL_AGENT_STEP", "0 1")):
        assert {o[var] for o in ov if var in o} >= set(values.split()), var
        assert set(rows[:, col["override"]]) >= {i for i, o in enumerate(ov) if var in o}, var
    run = rows[rows[:, col["persist"]] == 1]
    assert set(run[:, col["parts"]]) == {1, 2}
    plain = run[np.array(["ORL_PERSIST_CHUNK" not in o for o in ov])[run[:, col["override"]]]]
    assert (plain[:, col["chunk"]] < 128).any() and (plain[:, col["chunk"]] == 128).any()  # a chunk clamped by the log
    have = run[run[:, col["log_cap_have"]] > 0]
    assert (have[:, col["log_cap"]] > have[:, col["log_cap_have"]]).any() and (have[:, col["log_cap"]] == have[:, col["log_cap_have"]]).any()
    assert set(run[:, col["clear_counters"]]) == {0, 1}
    for name in ("persist", "two_kernel", "agent_step"):
        assert set(rows[:, col[name]]) == {0, 1}, name
    default = rows[rows[:, col["lib"]] == 0]
    assert set(default[:, col["two_kernel"]]) == {0}
    masks = {v: rows[np.array([o.get("ORL_ITEM_MASKS") == v for o in ov])[rows[:, col["override"]]]] for v in ("1", "9")}
    assert (masks["1"][:, col["item_masks"]] == 1).all() and (masks["1"][:, col["rel_limit"]] == 1).all()  # the override taken
    assert (masks["9"][:, col["item_masks"]] == 8).all() and (masks["9"][:, col["rel_limit"]] == 31).all()  # ... and ignored
    rd = _rows_deferred(rows, meta, col)
    assert rd.any() and (~rd & (rows[:, col["persist"]] == 1)).any()
    assert (rows[rd][:, col["elog_cap"]] > 0).all()
    assert {34, 4096} <= set(rows[rd][:, col["elog_cap"]])


def test_every_decision_is_the_recorded_one():
    """== on every column of every row, but for the one deliberate difference: a batch whose chosen form is not rows-deferred plans
    no event log (elog_cap 0), where the recording has the capacity every single-core batch of at most 64 links used to get."""
    import gen_golden_run_plan as gen

    rows, meta = _golden()
    col = {n: i for i, n in enumerate(meta["columns"])}
    got = gen.rows()
    assert got.shape == rows.shape and got.dtype == rows.dtype
    rd = _rows_deferred(rows, meta, col)
    assert (got[~rd][:, col["elog_cap"]] == 0).all()
    want = rows.copy()
    want[~rd, col["elog_cap"]] = 0
    bad = np.nonzero((got != want).any(axis=1))[0]
    lines = []
    n_key = len(gen.KEY_COLS)
    for i in bad[:20]:
        k = dict(zip(meta["columns"][:n_key], rows[i, :n_key].tolist()))
        lines.append("%s, %s library, %d envs, %d steps, tuned %d, log %d, run_base %d, dirty %d, %s: recorded %s, now %s" % (
            meta["configs"][k["config"]], meta["libs"][k["lib"]], k["batch"], k["steps"], k["tuned"], k["log_cap_have"],
            meta["run_base"][k["run_base"]], k["wg_dirty"], meta["overrides"][k["override"]] or "no override",
            dict(zip(meta["columns"][n_key:], want[i, n_key:].tolist())), dict(zip(meta["columns"][n_key:], got[i, n_key:].tolist()))))
    assert not len(bad), "%d of %d decisions differ:\n%s" % (len(bad), len(rows), "\n".join(lines))
