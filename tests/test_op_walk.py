"""The walks and the model of tests/op_walk.py on the oracle alone, before any device is involved: a rebuild by replay is exact on the
oracle itself; over a family's walks every ordered pair of state-changing kinds occurs and every query kind follows every kind;
and the walks reach what they exist for (episode ends, blocking, copies into and out of busy envs, restores across an episode end,
set_load on envs whose pending service was drawn at the old rates).  tests/test_op_walk_gpu.py drives the same walks on the device."""
import functools

import numpy as np
import pytest

from tests import op_walk as ow
from tests.helpers import _exact_bits

FAMILY_NAMES = sorted(ow.FAMILIES)
# RMCSA: reach limits refuse about 45 % of the services whatever chooses the action (tests/slot_agent.py: acceptance 0.58 under its
# agent, the same under SAP_BM_FC_FF here), so 64 pending releases need more than 200 steps in a row without a full reset even at the
# largest load the configuration's event capacity admits: outside a walk's budget of steps
# rwa_s8: 8 wavelengths on 22 links hold 70 to 80 services when nothing more fits (76 after 111 steps of SAP_FF from construction,
# the maximum over 16 envs), and no walk leaves an env that many steps without a full reset or a restore
NO_64_PENDING = ("rmcsa", "rwa_s8")


@functools.lru_cache(maxsize=None)
def driven(name):
    """every walk of the family on the model, finished episodes counted"""
    return [ow.drive_oracle(name, w, ledger=True) for w in ow.walks_of(name)]


def test_the_circuit_takes_every_ordered_pair_once():
    for k in (1, 2, 5, 10, 11):
        c = ow.euler_circuit(k)
        assert len(c) == k * k + 1 and c[0] == c[-1]
        assert len(ow.pairs_of(c)) == k * k
    pieces = ow.cut(list(range(101)), 35)
    assert [len(p) for p in pieces] == [35, 35, 33] and all(a[-1] == b[0] for a, b in zip(pieces, pieces[1:]))


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_walks_stay_inside_their_budget_and_the_api(name):
    f = ow.FAMILIES[name]
    lo, hi = ow.load_range(f)
    cap = ow.capacity_needed(ow.base_rates(f)[0])
    assert ow.capacity_needed(hi) <= cap < ow.capacity_needed(hi + 1.0) and lo < hi
    walks = ow.walks_of(name)
    assert [w.name for w in walks] == list(ow.WALK_NAMES)
    assert any(w.fresh for w in walks) and any(not w.fresh for w in walks)
    lengths = set()
    for w in walks:
        kinds = w.kinds()
        assert len(kinds) <= ow.MAX_OPS and w.steps() <= ow.MAX_STEPS, (w.name, len(kinds), w.steps())
        ops = [it for what, it in w.items if what == "op"]
        if w.fresh:
            assert "seed" not in kinds
        else:  # the second streams exist before the first snapshot is taken
            assert w.items[0][0] == "op" and kinds[0] == "seed" and not ops[0]["mask"].any()
        assert w.items[0 if w.fresh else 1] == ("q", dict(q="get_state"))
        snapshots = 0
        for what, it in w.items:
            if what == "q":
                snapshots += it["q"] == "get_state"
                continue
            if it["kind"] == "run":
                lengths.add(it["n"])
            if it["kind"] == "set_state":
                assert 0 <= it["snapshot"] < snapshots
            if it["kind"] == "set_load":
                for v in (it["load"], it["mht"]):
                    assert v is None or (np.all(np.asarray(v) > 0) and np.asarray(v).shape in ((), (f.batch,)))
                assert it["load"] is None or np.all(ow.capacity_needed(np.max(it["load"])) <= cap)
            if it["kind"] == "copy_envs":
                src, dst = it["src"], it["dst"]
                assert len(src) == len(dst) and len(set(dst)) == len(dst) and not set(src) & set(dst)
                assert min(src) >= 0 and min(dst) >= 0 and max(src) < f.batch and max(dst) < f.batch
    assert lengths == set(ow.RUN_LENGTHS)
    copies = [it["variant"] for w in walks for what, it in w.items if what == "op" and it["kind"] == "copy_envs"]
    assert {"fan_out", "pairs", "chain", "named"} <= set(copies)
    masks = [it["mask"] for w in walks for what, it in w.items if what == "op" and "mask" in it]
    sums = {None if m is None else int(m.sum()) for m in masks}
    assert {None, 0, 1, 4, 8, f.batch - 1} <= sums


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_every_pair_of_kinds_and_every_query_after_every_kind(name):
    walks = ow.walks_of(name)
    pairs = set().union(*(ow.pairs_of(w.kinds()) for w in walks))
    missing = [(a, b) for a in ow.KINDS for b in ow.KINDS if (a, b) not in pairs]
    assert not missing, missing
    fresh = set().union(*(ow.pairs_of(w.kinds()) for w in walks if w.fresh))
    assert not [(a, b) for a in ow.FRESH_KINDS for b in ow.FRESH_KINDS if (a, b) not in fresh]  # (what the loop forms run unreduced)
    after = set()
    for w in walks:
        last = None
        for what, it in w.items:
            if what == "op":
                last = it["kind"]
            elif last is not None:
                after.add((last, it["q"]))
    missing = [(k, q) for k in ow.KINDS for q in ow.queries_of(ow.FAMILIES[name]) if (k, q) not in after]
    assert not missing, missing


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_rebuild_by_replay_is_exact_on_the_oracle(name):
    """the env that was driven op by op (runs stepped on the host, rebuilt at every copy and restore) against one replayed from
    its list in one go (runs as oracle runs)"""
    moved = 0
    for w, m in zip(ow.walks_of(name), driven(name)):
        chk = _exact_bits("%s, walk %s" % (name, w.name))
        twins = [m.rebuild(i) for i in range(m.n)]
        got, want = m.readback(twins), m.readback()
        assert set(got) == set(want) and {"counters", "services", "active"} < set(want)
        for what in want:
            for i in range(m.n):
                chk(i, what, got[what][i], want[what][i])
        assert all(lst[0][0] == "make" for lst in m.lists)
        moved += sum(lst[0][1] != s for lst, s in zip(m.lists, ow.seeds_of(m.f)))
    assert moved  # (a copy took its source's construction with it)


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_what_the_walks_reach(name):
    models = driven(name)
    episodes = np.concatenate([m.episodes for m in models])
    blocked = np.concatenate([m.blocked for m in models])
    reach = {k: sum(m.reach[k] for m in models) for k in models[0].reach}
    print(name, "two episodes: %.2f, blocked: %.2f" % ((episodes >= 2).mean(), blocked.mean()), reach)
    assert (episodes >= 2).mean() >= 0.5
    # blocked: a heuristic's own action was not provisioned (run, step with the heuristic's actions, policy_step); an agent's refused
    # actions do not count.  An exception is asserted as one, so that it goes when it is no longer true
    if name in ow.NO_NETWORK_BLOCKING:
        assert not blocked.any()
    else:
        assert blocked.mean() >= 0.25
    assert reach["copy_into_pending"] >= 1
    if name in NO_64_PENDING:
        assert reach["copy_from_64"] == 0
    else:
        assert reach["copy_from_64"] >= 1
    assert reach["restore_across_episode"] >= 1
    assert reach["set_load_on_pending"] >= 1
    named = models[-1]  # the reseeded source and the copy made after the reseed carry the mark, the copy made before does not
    assert named.reach["copy_into_pending"] >= 1 and named.reseeded().sum() == 2


def test_a_restore_puts_back_the_list_a_copy_replaced():
    """snapshot, copy 0 -> 9, restore: env 9 is its own past again, not a prefix of env 0's"""
    m = ow.Model("rwa")
    m.apply(dict(kind="run", policy="SAP_FF", n=7))
    m.snapshot()
    before = m.readback()
    m.apply(dict(kind="run", policy="SAP_FF", n=3))
    m.apply(dict(kind="copy_envs", src=np.array([0]), dst=np.array([9])))
    assert m.lists[9][0] == m.lists[0][0]
    m.apply(dict(kind="set_state", snapshot=0))
    after = m.readback()
    for what in before:
        _exact_bits("restore")(0, what, after[what], before[what])
