"""The form the launcher of the persistent kernel chooses, pinned case by case without a GPU (orl_debug_persist_choice): every
row of tests/golden/persist_choice.npz — configurations x batch sizes x tuned / untuned x library build x ORL_PERSIST_*
overrides, recorded from the choice as it was before it became a table and a pure function (tools/gen_golden_persist_choice.py)
— is recomputed with the library under test and compared with ==.  A slip in the choice fails no other test without a GPU: it
costs 5-20 % on some configuration, or routes a family into a form that is not built."""
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
    d = np.load(os.path.join(ROOT, "tests", "golden", "persist_choice.npz"))
    return d["rows"], json.loads(str(d["meta"]))


def test_fixture_covers_every_form_and_every_field():
    """What the grid must reach, whatever the library under test does: every form 0-8 (2 and 3 through the alt library), the pair
    form, release times in LDS, every row-cache level, a tuned row that differs from its untuned one, a configuration that is
    not served, and rows whose launch asks for more LDS than the window (ORL_PERSIST_WGS_PER_CU)."""
    import gen_golden_persist_choice as gen

    rows, meta = _golden()
    col = {n: i for i, n in enumerate(meta["columns"])}
    assert meta["configs"] == [c[0] for c in gen.configs()] and meta["libs"] == list(gen.LIBS) and meta["overrides"] == gen.OVERRIDES
    assert len(rows) == len(gen.configs()) * len(gen.OVERRIDES) * len(gen.LIBS) * len(gen.BATCHES) * 2
    assert len(gen.configs()) >= 9 and set(gen.BATCHES) >= {64, 1024, 4096, 8192, 12288, 12296, 16384, 24576, 24584, 32768, 65536, 1 << 20}
    served = rows[rows[:, col["served"]] == 1]
    assert set(served[:, col["form"]]) == set(range(9))
    default = served[served[:, col["lib"]] == 0]
    assert set(default[:, col["form"]]) == set(range(9)) - {2, 3}
    assert set(served[:, col["rw"]]) == {0, 1} and set(served[:, col["evl"]]) == {0, 1} and set(served[:, col["inner"]]) == {0, 1, 2}
    assert set(served[:, col["lds_arg"]]) == set(range(6)) and set(served[:, col["waves"]]) == {2, 3, 4}
    assert (served[:, col["launch_lds_bytes"]] > served[:, col["window_bytes"]]).any()
    assert (rows[:, col["served"]] == 0).any()
    tuned, untuned = rows[rows[:, col["tuned"]] == 1], rows[rows[:, col["tuned"]] == 0]
    key = [col[n] for n in gen.KEY_COLS if n != "tuned"]
    assert (tuned[:, key] == untuned[:, key]).all()
    assert (tuned[:, len(gen.KEY_COLS):] != untuned[:, len(gen.KEY_COLS):]).any()


def test_every_choice_is_the_recorded_one():
    import gen_golden_persist_choice as gen

    rows, meta = _golden()
    got = gen.rows()
    assert got.shape == rows.shape and got.dtype == rows.dtype
    bad = np.nonzero((got != rows).any(axis=1))[0]
    lines = []
    for i in bad[:20]:
        ci, batch, tuned, li, oi = (int(v) for v in rows[i, :5])
        lines.append("%s, %d envs, tuned %d, %s library, %s: recorded %s, now %s" % (
            meta["configs"][ci], batch, tuned, meta["libs"][li], meta["overrides"][oi] or "no override",
            dict(zip(meta["columns"][5:], rows[i, 5:].tolist())), dict(zip(meta["columns"][5:], got[i, 5:].tolist()))))
    assert not len(bad), "%d of %d choices differ:\n%s" % (len(bad), len(rows), "\n".join(lines))
