"""The host-side decisions of the per-step device views, pinned case by case without a GPU (orl_debug_view_plan over
csrc/orl_view_plan.h): the shape of a view's rows (row length, blocks, pitch) and the geometry of its launch (wavefronts per
workgroup, grid, dynamic LDS, staged / chunked / counted, or refused).  Every row of tests/golden/view_plan.npz — views x env
families x row widths x sizes x layouts / rules / j x batch sizes, recorded from the statements as they stood in the seven launchers
and the shape functions before they became pure functions (tools/gen_golden_view_plan.py) — is recomputed with the library under
test and compared with ==.  A slip here fails no other test without a GPU: it costs a launch failure or a silent change of form at
k = 64, many cores or 512 slots, shapes the small GPU cases do not reach."""
import json
import os
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")

LDS_DEFAULT, LDS_MAX = 48 * 1024, 64 * 1024


def _golden():
    d = np.load(os.path.join(ROOT, "tests", "golden", "view_plan.npz"))
    return np.ascontiguousarray(d["cols"].T), json.loads(str(d["meta"]))


def _sel(rows, col, **eq):
    keep = np.ones(len(rows), bool)
    for name, v in eq.items():
        keep &= rows[:, col[name]] == v
    return rows[keep]


def test_fixture_reaches_every_decision():
    """What the grid must reach, whatever the library under test does."""
    import gen_golden_view_plan as gen

    rows, meta = _golden()
    col = {n: i for i, n in enumerate(meta["columns"])}
    assert meta["columns"] == list(gen.KEY_COLS + ("valid",) + gen.FIELDS) and meta["views"] == list(gen.VIEWS)
    assert len(rows) == len(set(gen.grid())) and 2000 <= len(rows) <= 5000 and (rows[:, col["valid"]] == 1).all()
    assert set(rows[:, col["view"]]) == set(range(7)) and set(rows[:, col["env"]]) == set(range(5))
    slot_maps = rows[rows[:, col["env"]] != gen.QOS]  # (QoSConstrainedRA keeps a counter per link: row width 1 whatever S)
    assert {(w, s) for w, s in slot_maps[:, [col["W"], col["S"]]].tolist()} == {(1, 64), (2, 65), (2, 128), (5, 129), (5, 320), (8, 321), (8, 512)}
    assert set(rows[:, col["K"]]) >= {1, 5, 8, 9, 23, 24, 38, 39, 64} and set(rows[:, col["M"]]) == {1, 6, 32, 33}
    assert set(rows[:, col["C"]]) >= {1, 2, 7, 13, 31} and set(rows[:, col["J"]]) == {1, 8} and set(rows[:, col["B"]]) == {1, 31, 32, 33, 65536}
    for view in range(7):
        assert set(_sel(rows, col, view=view)[:, col["B"]]) == {1, 31, 32, 33, 65536}, view
    mask = _sel(rows, col, view=gen.ACTION_MASK)
    assert set(mask[:, col["arg"]]) == {0, 1, 2, 3} and set(mask[:, col["env"]]) == {gen.RMSA, gen.DEEPRMSA, gen.RWA}
    assert set(mask[:, col["ok"]]) == {0, 1}
    # joint RMSA at 8 words: 4 wavefronts x 8 envs x (16 k + 2) words of 4 bytes fit 48 KiB up to k = 23
    joint8 = _sel(mask, col, env=gen.RMSA, arg=gen.JOINT, W=8, S=512)
    assert _sel(joint8, col, K=23)[:, col["ok"]].tolist() == [1] and _sel(joint8, col, K=24)[:, col["ok"]].tolist() == [0]
    assert (mask[mask[:, col["ok"]] == 1][:, col["waves"]] == 4).all()
    assert (mask[:, col["dim"]] == 0).any() and (mask[:, col["dim"]] > 0).any()  # a layout the family does not have
    rm = _sel(rows, col, view=gen.RMCSA_MASK)
    assert set(rm[:, col["arg"]]) == {0, 1, 2, 3}
    pm64 = rm[(rm[:, col["arg"]] == gen.PATH_MOD) & (rm[:, col["K"]] == 64) & (rm[:, col["M"]] <= 32)]
    assert set(pm64[:, col["waves"]]) == {4, 2, 1, 0} and (pm64[:, col["C"]] <= 31).all()  # C rising, every one an accepted C
    assert (pm64[pm64[:, col["waves"]] == 0][:, col["ok"]] == 0).all()
    m33 = _sel(rm, col, M=33)
    assert len(m33) and (m33[:, col["ok"]] == 0).all()
    for r in m33[m33[:, col["dim"]] > 0]:  # ... which M alone refuses: the same sizes at M = 32 are taken
        twin = _sel(rm, col, M=32, K=r[col["K"]], C=r[col["C"]], W=r[col["W"]], S=r[col["S"]], arg=r[col["arg"]], B=r[col["B"]])
        assert len(twin) == 1
    assert (_sel(rm, col, M=32, K=5, C=7)[:, col["ok"]] == 1).all()
    assert len(_sel(rows, col, view=gen.COMPLETE, waves=4, lds_bytes=0)) == len(_sel(rows, col, view=gen.COMPLETE))
    asg = _sel(rows, col, view=gen.ASSIGN)
    assert set(asg[:, col["arg"]]) == set(range(6))
    for W in (1, 2, 5, 8):
        assert set(_sel(asg, col, W=W)[:, col["counted"]]) == {0, 1}, W
    assert ((asg[:, col["counted"]] == 1) == (asg[:, col["arg"]] >= 4)).all()
    assert ((asg[:, col["lds_bytes"]] > 0) == (asg[:, col["counted"]] == 1)).all()
    pf = _sel(rows, col, view=gen.PATH_FEATURES)
    assert set(pf[:, col["arg"]]) == {1, 8} and set(pf[:, col["staged"]]) == {0, 1} and set(pf[:, col["env"]]) == {0, 1, 2, 3}
    assert set(pf[pf[:, col["staged"]] == 1][:, col["waves"]]) == {4, 2, 1}
    assert ((pf[:, col["staged"]] == 0) == (pf[:, col["lds_bytes"]] == 0)).all()
    lf = _sel(rows, col, view=gen.LINK_FEATURES)
    assert set(lf[lf[:, col["chunk"]] == 0][:, col["waves"]]) == {4, 2, 1}   # whole
    assert set(lf[lf[:, col["chunk"]] > 0][:, col["waves"]]) == {4, 2, 1}    # chunked (by the formula 1 from k = 58, 2 from k = 26)
    assert (_sel(lf, col, K=64)[:, col["chunk"]] > 0).any()
    qo = _sel(rows, col, view=gen.MATRIX_PATHS_OBS)
    assert set(qo[:, col["ok"]]) == {0, 1} and (qo[:, col["env"]] == gen.QOS).all()
    # 4 wavefronts x E (k + 1) u16: 64 KiB at E (k + 1) = 8192
    assert (_sel(qo, col, E=128, K=63)[:, col["ok"]] == 1).all() and (_sel(qo, col, E=128, K=64)[:, col["ok"]] == 0).all()


def _check_properties(rows, col, what):
    view, ok, waves = rows[:, col["view"]], rows[:, col["ok"]] == 1, rows[:, col["waves"]].astype(np.int64)
    qos = view == 6
    assert (rows[~ok][:, col["waves"]:] == 0).all(), what  # a refused launch: every plan field 0
    assert np.isin(waves[ok], (1, 2, 4)).all() and (rows[ok, col["block"]] == 64 * waves[ok]).all(), what
    assert (rows[ok, col["lds_bytes"]] <= np.where(qos, LDS_MAX, LDS_DEFAULT)[ok]).all() and (rows[:, col["lds_bytes"]] >= 0).all(), what
    per_wg = np.where(qos, waves, 8 * waves)[ok]  # envs of a workgroup
    grid, B = rows[ok, col["grid"]].astype(np.int64), rows[ok, col["B"]].astype(np.int64)
    assert ((grid - 1) * per_wg < B).all() and (B <= grid * per_wg).all(), what
    chunk = rows[:, col["chunk"]]
    assert (chunk >= 0).all() and (chunk % 8 == 0).all() and (chunk[view != 5] == 0).all(), what
    assert ((rows[:, col["pitch"]].astype(np.int64) * rows[:, col["elem_bytes"]]) % 16 == 0).all(), what
    assert (rows[:, col["pitch"]] >= rows[:, col["dim"]]).all() and (rows[:, col["pitch"]] - rows[:, col["dim"]] < 16 // rows[:, col["elem_bytes"]]).all(), what
    blocks = rows[np.isin(view, (4, 5))]  # the feature rows: a header of 1 + 2 N, then rows x width
    assert (blocks[:, col["dim"]] == 1 + 2 * blocks[:, col["N"]] + blocks[:, col["rows"]] * blocks[:, col["width"]]).all(), what
    # a chunked round of link features fits, and 8 more slot rows per env would not
    lf = rows[(view == 5) & (chunk > 0)]
    sets = 8 * 2 * lf[:, col["K"]].astype(np.int64) * 8
    per8 = 8 * 8 * lf[:, col["width"]].astype(np.int64) * 4
    w = lf[:, col["waves"]].astype(np.int64)
    assert (w * (sets + lf[:, col["chunk"]] // 8 * per8) == lf[:, col["lds_bytes"]]).all(), what
    assert (w * (sets + (lf[:, col["chunk"]] // 8 + 1) * per8) > LDS_DEFAULT).all(), what


def test_properties_no_recording_can_get_wrong():
    """Of the recording and of the library under test: the LDS of a workgroup within the view's limit, a grid that covers the batch
    and not a workgroup more, a chunk that is a positive multiple of 8 where rows are chunked, a row pitch of whole 16-byte stores."""
    import gen_golden_view_plan as gen

    rows, meta = _golden()
    col = {n: i for i, n in enumerate(meta["columns"])}
    _check_properties(rows, col, "recorded")
    _check_properties(gen.rows(), col, "library under test")


def test_every_decision_is_the_recorded_one():
    import gen_golden_view_plan as gen

    rows, meta = _golden()
    got = gen.rows()
    assert got.shape == rows.shape and got.dtype == rows.dtype
    bad = np.nonzero((got != rows).any(axis=1))[0]
    n_key = len(gen.KEY_COLS) + 1
    lines = ["%s: recorded %s, now %s" % (dict(zip(meta["columns"][:n_key], rows[i, :n_key].tolist())), dict(zip(gen.FIELDS, rows[i, n_key:].tolist())),
                                          dict(zip(gen.FIELDS, got[i, n_key:].tolist()))) for i in bad[:20]]
    assert not len(bad), "%d of %d decisions differ:\n%s" % (len(bad), len(rows), "\n".join(lines))
