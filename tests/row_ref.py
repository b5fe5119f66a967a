"""Run-length reference of the slot-row summary, in plain numpy: what RMSAEnv reads of one link's spectrum through rle()
(rmsa_env.py:651-665) in _update_link_stats (:464-543), get_available_blocks (:667-697) and _get_network_compactness (:699-744).
A row is a 0/1 array of S slots, 1 = free (the reference's available_slots).  Written from those lines, not from the device
code: no bit tricks, no shortcut such as "free blocks inside = used blocks - 1".  Test infrastructure only.

Two forms: *_one works on one row through a run-length encoding, as the reference does; the batched functions take [R, S] arrays and are checked
against the one-row form in tests/test_row_prims.py."""
import numpy as np

from tests.mask_restate import _rle as rle  # run-length encoding, the suite's one restatement of it: (starts, values, lengths)


def summary_one(row):
    """dict of the reference's numbers for one row: free (slots), nu / nf (used / free blocks), lo (first used slot, -1: none), hi
    (last used slot + 1, 0: none), occ = hi - lo and fb = free blocks strictly inside [lo, hi) when nu >= 2 else 0 / 0, longest (free
    run), edge (slot 0 free + slot S - 1 free)."""
    row = np.asarray(row, np.int64)
    starts, values, lengths = rle(row)
    used_blocks, unused_blocks = np.flatnonzero(values == 0), np.flatnonzero(values == 1)
    out = dict(free=int(np.sum(row)), nu=len(used_blocks), nf=len(unused_blocks), lo=-1, hi=0, occ=0, fb=0,
               longest=int(lengths[unused_blocks].max()) if len(unused_blocks) else 0, edge=int(row[0]) + int(row[-1]))
    if len(used_blocks):
        out["lo"] = int(starts[used_blocks[0]])
        out["hi"] = int(starts[used_blocks[-1]] + lengths[used_blocks[-1]])
    if len(used_blocks) > 1:
        _, internal_values, _ = rle(row[out["lo"]:out["hi"]])
        out["occ"] = out["hi"] - out["lo"]
        out["fb"] = int(np.sum(internal_values))
    return out


def blocks_one(row, n):
    """get_available_blocks without the cut to j: [(start, end)] of the free blocks of at least n slots, low to high."""
    starts, values, lengths = rle(np.asarray(row, np.int64))
    idx = np.intersect1d(np.where(values == 1), np.where(lengths >= n))
    return [(int(starts[i]), int(starts[i] + lengths[i])) for i in idx]


def first_slot_mask_one(row, n):
    """bit s: slots s .. s + n - 1 exist and are all free (is_path_free, rmsa_env.py:623-636, on one row)"""
    row = np.asarray(row, np.int64)
    S = len(row)
    return np.array([s + n <= S and not np.any(row[s:s + n] == 0) for s in range(S)], np.uint8)


def inner_run_one(word):
    """The longest run of ones of a 64-slot word without the runs that touch its two ends (a word of ones only: 0)."""
    word = np.asarray(word, np.int64)
    _, values, lengths = rle(word)
    inner = [int(l) for k, (v, l) in enumerate(zip(values, lengths)) if v == 1 and 0 < k < len(values) - 1]
    return max(inner) if inner else 0


# ---- batched ------------------------------------------------------------------------------------------------------------
def _run_end(x):
    """[R, S] 0/1 -> length of the run of ones that ends at each position (0 where x is 0)"""
    x = np.asarray(x, np.int64)
    c = np.cumsum(x, axis=1)
    return c - np.maximum.accumulate(np.where(x == 0, c, 0), axis=1)


def _run_start(x):
    return _run_end(np.asarray(x)[:, ::-1])[:, ::-1]


def summary(rows):
    """summary_one for every row of [R, S]: dict of int64 arrays [R]."""
    rows = np.asarray(rows, np.int64)
    R, S = rows.shape
    idx = np.arange(S)[None, :]
    prev = np.concatenate([np.full((R, 1), -1, np.int64), rows[:, :-1]], axis=1)  # (-1: a block starts at slot 0 whatever it holds)
    used_start = (rows == 0) & (prev != 0)
    free_start = (rows == 1) & (prev != 1)
    nu, nf = used_start.sum(axis=1), free_start.sum(axis=1)
    any_used = (rows == 0).any(axis=1)
    lo = np.where(any_used, np.argmax(rows == 0, axis=1), -1)
    hi = np.where(any_used, S - np.argmax(rows[:, ::-1] == 0, axis=1), 0)
    two = nu > 1
    inside = free_start & (idx >= lo[:, None]) & (idx < hi[:, None])
    return dict(free=rows.sum(axis=1), nu=nu, nf=nf, lo=lo, hi=hi, occ=np.where(two, hi - lo, 0),
                fb=np.where(two, inside.sum(axis=1), 0), longest=_run_end(rows).max(axis=1), edge=rows[:, 0] + rows[:, -1])


def first_slot_mask(rows, n):
    """[R, S] uint8: slots s .. s + n - 1 all free and inside the row"""
    return (_run_start(rows) >= n).astype(np.uint8)


def run_below_from(rows):
    """(below, from_), both [R, S + 1]: free slots directly below slot p / from slot p upwards, slots outside the row taken"""
    rows = np.asarray(rows, np.int64)
    R = rows.shape[0]
    z = np.zeros((R, 1), np.int64)
    return np.concatenate([z, _run_end(rows)], axis=1), np.concatenate([_run_start(rows), z], axis=1)


def inner_runs(words):
    """inner_run_one for [N, 64]"""
    w = np.asarray(words, np.int64)
    lead = np.where(w.all(axis=1), 64, np.argmin(w, axis=1))
    trail = np.where(w.all(axis=1), 64, np.argmin(w[:, ::-1], axis=1))
    idx = np.arange(64)[None, :]
    keep = (idx >= lead[:, None]) & (idx < 64 - trail[:, None])
    return _run_end(np.where(keep, w, 0)).max(axis=1)


def pack(rows, W):
    """[R, S] 0/1 -> [R, W] uint64, bit s % 64 of word s // 64 = slot s, bits >= S zero"""
    rows = np.asarray(rows, np.uint8)
    R, S = rows.shape
    full = np.zeros((R, 64 * W), np.uint8)
    full[:, :S] = rows
    return np.ascontiguousarray(np.packbits(full, axis=1, bitorder="little")).view("<u8").reshape(R, W).astype(np.uint64)


def unpack(words, S=None):
    """[R, W] uint64 -> [R, 64 W] (or [R, S]) 0/1"""
    words = np.ascontiguousarray(np.asarray(words, np.uint64).astype("<u8"))
    bits = np.unpackbits(words.view(np.uint8).reshape(words.shape[0], -1), axis=1, bitorder="little")
    return bits if S is None else bits[:, :S]
