#!/usr/bin/env python3
"""tests/golden/run_plan.npz: the host-side decisions of the library — the step route of a batch (persistent kernel, two-kernel
form, k_agent, item-mask limit) and the plan of a device-resident run (steps per launch, one stream or two, the split point, the
capacities of the statistics and the event log, whether the step counters are cleared) — over a grid of configurations, library
builds, batch sizes, run lengths, batch states and overrides.  No device is needed (orl_debug_run_plan).

The fixture is a record of those decisions as they were BEFORE they became pure functions (csrc/orl_run_plan.h): it was written
by this script running on commit 6755957 with record_parent_run_plan.patch applied (the patch that accompanied the change:
nothing but the query, over statements lifted verbatim out of that commit's batch_create_impl, ensure_logs and orl_batch_run,
and its Python binding).  tests/test_run_plan.py recomputes every row with the library under test and compares with ==, but
for one column: where the chosen form is not rows-deferred the library now plans no event log (elog_cap 0), and the recording
has the capacity every single-core batch of at most 64 links used to get.  The file is regenerated only when a decision is
changed on purpose, never to make that test pass; the zip members carry a fixed date, so the same library gives the same bytes.

Usage:  python3 tools/gen_golden_run_plan.py [out.npz]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden", "run_plan.npz")

LIBS = ("default", "alt")
N_CU = 256
ENVS = (64, 2047, 2048, 4096, 12288, 16376, 16384, 20479, 20480, 65536)
STEPS = (0, 1, 2, 20, 128, 129, 256, 257, 300, 3000)
LOG_HAVE = (0, 2, 12, 256)
RUN_BASE = (0, (1 << 30) - 100)
RD = {"ORL_PERSIST_VARIANT": "7"}  # a rows-deferred form wherever it is possible
STEP_VARS = ("ORL_STEP_IMPL", "ORL_PERSIST", "ORL_AGENT_STEP", "ORL_ITEM_MASKS")
RUN_VARS = ("ORL_PERSIST_CHUNK", "ORL_PERSIST_PARTS", "ORL_LOG_CAP", "ORL_ELOG_CAP", "ORL_RUN_BASE_LIMIT")
# every variable at both ends of its accepted range and just outside each end (a switch: each value it distinguishes, and another)
STEP_OVERRIDES = ([{"ORL_STEP_IMPL": v} for v in ("64", "63", "2")] + [{"ORL_PERSIST": v} for v in ("0", "1")]
                  + [{"ORL_PERSIST": "0", "ORL_STEP_IMPL": v} for v in ("2", "64")]
                  + [{"ORL_AGENT_STEP": v} for v in ("0", "1")] + [{"ORL_AGENT_STEP": "1", "ORL_STEP_IMPL": "64"}]
                  + [{"ORL_ITEM_MASKS": v} for v in ("0", "1", "8", "9")])
RUN_OVERRIDES = ([{"ORL_PERSIST_CHUNK": v} for v in ("0", "1", "64", "2147483647")]
                 + [{"ORL_PERSIST_PARTS": v} for v in ("0", "1", "2", "3")]
                 + [{"ORL_LOG_CAP": v} for v in ("1", "2", "256", "257")]
                 + [dict(RD, ORL_LOG_CAP=v) for v in ("2", "256")]
                 + [dict(RD, ORL_ELOG_CAP=v) for v in ("33", "34", "4096", "4097")] + [{"ORL_ELOG_CAP": "34"}]
                 + [{"ORL_RUN_BASE_LIMIT": v} for v in ("0", "1", "1073741823", "9223372036854775807")])
OVERRIDES = [{}, RD] + STEP_OVERRIDES + RUN_OVERRIDES
# every other variable the choice of the form reads: unset while the grid is walked
OTHER_VARS = ("ORL_PERSIST_VARIANT", "ORL_PERSIST_RW", "ORL_PERSIST_INNER", "ORL_PERSIST_EVL", "ORL_PERSIST_WGS_PER_CU", "ORL_PERSIST_SPEC",
              "ORL_PERSIST_FAIR", "ORL_ROW_CACHE_KEEP")
KEY_COLS = ("config", "lib", "batch", "steps", "tuned", "log_cap_have", "run_base", "wg_dirty", "override", "valid")


def configs():
    """Those of the form choice's fixture (the bench workloads, two more of RMSA, QoSConstrainedRA), QoSConstrainedRA with more than
    8 paths (no k_agent_qos) and RMSA on more than 128 links (no k_agent): the last two are topology descriptions no topology file
    backs — the query reads the description's sizes only."""
    import gen_golden_persist_choice as pc

    out = [c + ({},) for c in pc.configs()]
    name, fam, topo, kw = pc.configs()[-1]
    assert fam == "QoSConstrainedRA"
    out.append(("qos_k9", fam, topo, kw, dict(k_paths=9)))
    name, fam, topo, kw = [c for c in pc.configs() if c[0] == "cfg2"][0]
    out.append(("cfg2_e130", fam, topo, kw, dict(n_links=130)))
    return out


def grid():
    """(config, lib, batch, steps, tuned, log_cap_have, run_base index, wg_dirty, override index): the product pruned to three slices."""
    names = [c[0] for c in configs()]
    n_cfg, none, rd = len(names), 0, 1
    for ci in range(n_cfg):  # every configuration, batch size and run length, a fresh batch, with and without a rows-deferred form
        for oi in (none, rd):
            for batch in ENVS:
                for steps in STEPS:
                    for tuned in (0, 1):
                        yield (ci, 0, batch, steps, tuned, 0, 0, 0, oi)
    for ci in (names.index("cfg2"), names.index("cfg4"), names.index("cfg5")):  # the batch's state in front of the run
        for oi in (none, rd):
            for batch in (64, 4096, 65536):
                for steps in (1, 20, 129, 300, 3000):
                    for have in LOG_HAVE:
                        for bi in range(len(RUN_BASE)):
                            for dirty in (0, 1):
                                yield (ci, 0, batch, steps, 1, have, bi, dirty, oi)
    for ci in range(n_cfg):  # the overrides: the step route in both builds at the batch sizes it turns on, the run plan in one
        for oi in range(2, 2 + len(STEP_OVERRIDES)):
            for li in range(len(LIBS)):
                for batch in (64, 2047, 2048, 20479, 20480, 65536):
                    yield (ci, li, batch, 20, 1, 0, 0, 0, oi)
        for oi in range(2 + len(STEP_OVERRIDES), len(OVERRIDES)):
            for batch in (64, 4096, 65536):
                for steps in (20, 300):
                    yield (ci, 0, batch, steps, 1, 12, 1, 0, oi)


def rows():
    """[n][len(KEY_COLS) + 11] int32: the key columns, then the fields of envs.RUN_PLAN_FIELDS (zeros where the query refuses)."""
    from optical_rl_gym_amd import envs

    saved = {k: os.environ.pop(k, None) for k in STEP_VARS + RUN_VARS + OTHER_VARS}
    cfgs = []
    for _name, fam, topo, kw, desc in configs():
        cfg = envs.ENV_CLASSES[fam]._derived(topology=topo, **kw)
        for k, v in desc.items():
            setattr(cfg._desc, k, v)
        cfgs.append(cfg)
    out = []
    try:
        last = None
        for key in sorted(set(grid()), key=lambda k: k[8]):  # (the slices overlap in a few rows)
            ci, li, batch, steps, tuned, have, bi, dirty, oi = key
            if oi != last:
                for k in STEP_VARS + RUN_VARS + OTHER_VARS:
                    os.environ.pop(k, None)
                os.environ.update(OVERRIDES[oi])
                last = oi
            p = cfgs[ci].run_plan(batch, steps, tuned, N_CU, have, RUN_BASE[bi], dirty, LIBS[li])
            out.append(key + (int(p is not None),) + (p or (0,) * len(envs.BatchedOpticalEnv.RUN_PLAN_FIELDS)))
    finally:
        for k in STEP_VARS + RUN_VARS + OTHER_VARS:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})
    return np.array(sorted(out), np.int32)


if __name__ == "__main__":
    from gen_golden_persist_choice import write
    from optical_rl_gym_amd import envs

    r = rows()
    meta = dict(columns=list(KEY_COLS + envs.BatchedOpticalEnv.RUN_PLAN_FIELDS), configs=[c[0] for c in configs()], libs=list(LIBS),
                overrides=OVERRIDES, n_cu=N_CU, run_base=list(RUN_BASE))
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    # (stored column by column: a column repeats itself far more than a row does, and the file is a third of the size)
    write(path, dict(cols=np.ascontiguousarray(r.T), meta=np.array(json.dumps(meta, sort_keys=True))))
    print("%s: %d rows, %d bytes" % (path, len(r), os.path.getsize(path)))
