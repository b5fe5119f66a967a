#!/usr/bin/env python3
"""tests/golden/persist_choice.npz: what the launcher of the persistent kernel chooses (form, LDS template argument, waves per
SIMD, pair form, row-cache level, release times in LDS, window bytes, launch LDS bytes, workgroups per CU) over a grid of
configurations, batch sizes, library builds and ORL_PERSIST_* overrides.  No device is needed (orl_debug_persist_choice).

The fixture is a record of the choice as it was BEFORE the choice became a table and a pure function: it was written by this
script running on commit 5393dbbe6c8ec077a72bf0aab137904189aca453 with record_parent_choice.patch applied (the patch that
accompanied the change: nothing but the query, on top of that commit's unchanged persist_choose, and its Python binding).
tests/test_persist_choice.py recomputes every row with the library under test and compares with ==.  The file is regenerated
only when a choice is changed on purpose, never to make that test pass; the zip members carry a fixed date, so the same
library gives the same bytes.

Usage:  python3 tools/gen_golden_persist_choice.py [out.npz]
"""
import io
import json
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "persist_choice.npz")

BATCHES = (64, 1024, 4096, 8192, 12288, 12296, 16384, 24576, 24584, 32768, 65536, 1 << 20)
LIBS = ("default", "alt")
OVERRIDE_VARS = ("ORL_PERSIST_VARIANT", "ORL_PERSIST_RW", "ORL_PERSIST_INNER", "ORL_PERSIST_EVL", "ORL_PERSIST_WGS_PER_CU")
OVERRIDES = ([{}] + [{"ORL_PERSIST_VARIANT": str(v)} for v in range(-1, 10)]
             + [{"ORL_PERSIST_RW": "0"}, {"ORL_PERSIST_RW": "1"}, {"ORL_PERSIST_VARIANT": "4", "ORL_PERSIST_RW": "1"}]
             + [{"ORL_PERSIST_INNER": str(v)} for v in (0, 1, 2)]
             + [{"ORL_PERSIST_RW": "1", "ORL_PERSIST_EVL": str(v)} for v in (0, 1)]
             + [{"ORL_PERSIST_WGS_PER_CU": str(v)} for v in (8, 11)])
# every other variable the launcher reads: unset while the grid is walked
OTHER_VARS = ("ORL_PERSIST_SPEC", "ORL_PERSIST_FAIR", "ORL_ROW_CACHE_KEEP")
KEY_COLS = ("config", "batch", "tuned", "lib", "override", "served")


def configs():
    """The six bench workloads, the two extra configurations of the specialisation test (tests/test_gpu_parity.py), and one the
    persistent kernel does not serve (QoSConstrainedRA: the query returns 0)."""
    from bench import WORKLOADS

    out = [(name, fam, topo, kw) for name, (fam, topo, kw, _policy) in WORKLOADS.items()]
    fam, topo, kw, _policy = WORKLOADS["cfg2"]
    out.append(("rmsa100", fam, topo, dict(kw, num_spectrum_resources=100, load=120)))
    out.append(("odd300", fam, topo, dict(kw, num_spectrum_resources=300, load=250, bit_rate_lower_bound=40, bit_rate_higher_bound=90)))
    out.append(("qos", "QoSConstrainedRA", "nsfnet_chen", dict(num_spectrum_resources=32, num_service_classes=2,
                                                              classes_arrival_probabilities=[0.5, 0.5], classes_reward=[2.0, 1.0])))
    return out


def rows():
    """[n][len(KEY_COLS) + 9] int32: the key columns, then the fields of envs.PERSIST_CHOICE_FIELDS (zeros where not served)."""
    from optical_rl_gym_amd import envs

    saved = {k: os.environ.pop(k, None) for k in OVERRIDE_VARS + OTHER_VARS}
    out = []
    try:
        for ci, (_name, fam, topo, kw) in enumerate(configs()):
            cfg = envs.ENV_CLASSES[fam]._derived(topology=topo, **kw)
            for oi, ov in enumerate(OVERRIDES):
                os.environ.update(ov)
                try:
                    for li, variant in enumerate(LIBS):
                        for batch in BATCHES:
                            for tuned in (0, 1):
                                c = cfg.persist_choice(batch, tuned, variant)
                                out.append((ci, batch, tuned, li, oi, int(c is not None)) + (c or (0,) * len(cfg.PERSIST_CHOICE_FIELDS)))
                finally:
                    for k in ov:
                        del os.environ[k]
    finally:
        os.environ.update({k: v for k, v in saved.items() if v is not None})
    return np.array(out, np.int32)


def write(path, arrays):
    """np.savez_compressed with a fixed date on every member: the same arrays give the same file."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


if __name__ == "__main__":
    from optical_rl_gym_amd import envs

    r = rows()
    meta = dict(columns=list(KEY_COLS + envs.BatchedOpticalEnv.PERSIST_CHOICE_FIELDS),
                configs=[c[0] for c in configs()], libs=list(LIBS), overrides=OVERRIDES)
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    write(path, dict(rows=r, meta=np.array(json.dumps(meta, sort_keys=True))))
    print("%s: %d rows, %d bytes" % (path, len(r), os.path.getsize(path)))
