"""The index rules of copy_envs (csrc/orl_copy_plan.h, copy_pairs_check) without a device, through orl_debug_copy_pairs_check: the
number of pairs that remain once the no-ops are dropped, or a refusal with its reason in orl_last_error()."""
import numpy as np
import pytest

INVALID = -1  # ORL_E_INVALID


def _check(B_src, B_dst, same, src, dst):
    from optical_rl_gym_amd import _lib

    lib = _lib.lib()
    s = np.ascontiguousarray(src, np.int64)
    d = np.ascontiguousarray(dst, np.int64)
    assert s.shape == d.shape
    rc = int(lib.orl_debug_copy_pairs_check(B_src, B_dst, int(same), len(s), s.ctypes.data if len(s) else None,
                                            d.ctypes.data if len(d) else None))
    return rc, lib.orl_last_error().decode()


def _rules(B_src, B_dst, same, src, dst):
    """The rules restated: every index inside its batch, no destination twice, and inside one batch no destination that is also the
    source of another pair once the src == dst no-ops are gone."""
    if any(s < 0 or s >= B_src for s in src) or any(d < 0 or d >= B_dst for d in dst):
        return INVALID
    if len(set(dst)) != len(dst):
        return INVALID
    pairs = [(s, d) for s, d in zip(src, dst) if not (same and s == d)]
    if same and {d for _s, d in pairs} & {s for s, _d in pairs}:
        return INVALID
    return len(pairs)


B = 67


def test_accepted_lists():
    assert _check(B, B, True, [], [])[0] == 0
    assert _check(B, B, True, [3], [4])[0] == 1
    assert _check(B, B, True, [5] * (B - 1), [i for i in range(B) if i != 5])[0] == B - 1  # fan-out of one source
    assert _check(B, B, True, [0, B - 1], [1, 2])[0] == 2
    assert _check(B, B, True, [0], [B - 1])[0] == 1
    assert _check(B, B, False, [0, B - 1], [B - 1, 0])[0] == 2
    assert _check(B, B, True, [3, 7, 3, 9], [3, 8, 4, 9])[0] == 2  # identity pairs are dropped as no-ops
    assert _check(B, B, True, [3, 3], [3, 5])[0] == 1  # ... also where their env is the source of a real pair
    assert _check(B, B, False, [33], [33])[0] == 1  # between two batches src == dst is a real copy
    assert _check(9, 200, False, [8, 0, 8], [199, 0, 9])[0] == 3  # batches of different sizes
    assert _check(200, 9, False, [199, 100], [8, 0])[0] == 2


@pytest.mark.parametrize("same", [True, False])
def test_refused_lists(same):
    for src, dst, word in (([-1], [0], "source index -1"), ([B], [0], "source index %d" % B), ([0], [-1], "destination index -1"),
                           ([0], [B], "destination index %d" % B), ([1, 2], [5, 5], "occurs twice"), ([5, 0], [5, 5], "occurs twice")):
        rc, why = _check(B, B, same, src, dst)
        assert rc == INVALID and word in why, (src, dst, why)


def test_in_place_overlap_is_refused_and_accepted_between_batches():
    for src, dst in (([0, 1], [1, 2]), ([0, 1], [1, 0])):
        rc, why = _check(B, B, True, src, dst)
        assert rc == INVALID and "scratch batch" in why, why
        assert _check(B, B, False, src, dst)[0] == 2


def test_negative_n_and_null_arrays():
    from optical_rl_gym_amd import _lib

    lib = _lib.lib()
    idx = np.zeros(4, np.int64)
    assert lib.orl_debug_copy_pairs_check(B, B, 1, -1, idx.ctypes.data, idx.ctypes.data) == INVALID
    assert "negative" in lib.orl_last_error().decode()
    assert lib.orl_debug_copy_pairs_check(B, B, 1, 1, None, idx.ctypes.data) == INVALID
    assert "null" in lib.orl_last_error().decode()
    assert lib.orl_debug_copy_pairs_check(B, B, 1, 1, idx.ctypes.data, None) == INVALID
    assert lib.orl_debug_copy_pairs_check(B, B, 1, 0, None, None) == 0


def test_random_lists_against_the_restated_rules():
    rng = np.random.default_rng(20)
    seen = {INVALID: 0, "ok": 0}
    for case in range(10000):
        same = bool(rng.integers(2))
        B_src = int(rng.integers(1, 24))
        B_dst = B_src if same else int(rng.integers(1, 24))
        n = int(rng.integers(0, 7))
        lo = -1 if case % 9 == 0 else 0  # (now and then an index just outside)
        src = [int(v) for v in rng.integers(lo, B_src + (case % 11 == 0), n)]
        dst = [int(v) for v in rng.integers(lo, B_dst + (case % 13 == 0), n)]
        want = _rules(B_src, B_dst, same, src, dst)
        got, why = _check(B_src, B_dst, same, src, dst)
        assert got == want, (B_src, B_dst, same, src, dst, got, want, why)
        seen[INVALID if want == INVALID else "ok"] += 1
    assert seen[INVALID] > 1000 and seen["ok"] > 1000
