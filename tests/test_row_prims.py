"""The slot-row primitives of csrc/orl_device.h and csrc/orl_device_split.h, called directly (tests/csrc/row_prims.hip wraps them in
thin kernels) and compared, == on integers, with the run-length reference of tests/row_ref.py: the five implementations of the row
summary (link_summary + row_longest_run; the 8-lane row_stat + row_longest_run8; row_stat_lane plain and with the inner-run cache;
the incremental row_inc_apply) and the search helpers beside them, at the slot counts where a 64-slot word ends — a one-bit tail
word, a full last word, a compiled row wider than the spectrum — on structured rows whose block edges sit on every word boundary
and on random rows.  The non-gpu part checks the reference itself against hand-written rows and cross-compiles the harness."""
import ctypes as C
import functools
import hashlib
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import row_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "row_prims.hip")
NONE_LO = 1 << 20  # the device's "no used slot" for lambda_min (row_ref: -1)

SLOTS = {1: (2, 63, 64), 2: (65, 127, 128), 5: (129, 191, 192, 193, 256, 257, 319, 320), 8: (321, 384, 385, 448, 449, 511, 512)}
CASES = [(W, S) for W in sorted(SLOTS) for S in SLOTS[W]]
CASE_IDS = ["w%d_s%d" % c for c in CASES]
CACHED = [c for c in CASES if c[0] <= 5]
CACHED_IDS = ["w%d_s%d" % c for c in CACHED]


# ---- the harness ------------------------------------------------------------------------------------------------------------
def harness_path():
    """tests/csrc/row_prims.hip compiled for gfx950 into the package's build directory, keyed by everything the compilation reads:
    the unit, the compiler's arguments, and _build.source_hash() — every file of csrc/, the library's flags, the compiler's
    version.  Libraries of other keys can never be loaded again and are dropped."""
    from optical_rl_gym_amd import _build

    args = _build.HIPCC_FLAGS + ["-I", _build.CSRC, "-shared"]
    with open(SRC, "rb") as f:
        key = hashlib.sha256(f.read() + " ".join(args).encode() + _build.source_hash().encode()).hexdigest()[:16]
    directory = os.path.join(_build.HERE, "build")
    out = os.path.join(directory, "row_prims_%s.so" % key)
    if not os.path.exists(out):
        os.makedirs(directory, exist_ok=True)
        tmp = out + ".tmp.%d" % os.getpid()
        subprocess.check_call([_build.hipcc_path()] + args + [SRC, "-o", tmp])
        os.replace(tmp, out)
    for name in os.listdir(directory):
        if name.startswith("row_prims_") and name.endswith(".so") and name != os.path.basename(out):
            os.unlink(os.path.join(directory, name))
    return out


@functools.lru_cache(maxsize=None)
def harness():
    from optical_rl_gym_amd import _lib

    _lib.lib()  # first: it brings in the one HIP runtime the process shares with PyTorch (a second copy would find no device)
    lib = C.CDLL(harness_path())
    p, i = C.c_void_p, C.c_int
    sigs = dict(basic=[p, i, i, p, p, p], runs_ge=[p, i, p], nth=[p, i, i, p, i, p], shr=[p, i, p, p], mask_lo=[p],
                masks=[p, p, i, i, p, p, p, p], runs=[p, i, i, p, p], row8=[p, i, i, p], cached=[p, i, i, p, p, p],
                inc=[p, i, i, p, p, i, p, p])
    for name, args in sigs.items():
        for W in SLOTS:
            f = getattr(lib, "rp_%s_w%d" % (name, W))
            f.argtypes, f.restype = args, C.c_int
    return lib


def call(name, W, *args):
    keep = [np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a for a in args]
    for a, k in zip(args, keep):
        assert not isinstance(a, np.ndarray) or a is k, "pass contiguous arrays: outputs are written in place"
    rc = getattr(harness(), "rp_%s_w%d" % (name, W))(*[a.ctypes.data if isinstance(a, np.ndarray) else a for a in keep])
    assert rc == 0, "rp_%s_w%d: HIP error %d" % (name, W, rc)


# ---- rows ---------------------------------------------------------------------------------------------------------------------
def boundary_positions(S):
    """B: the slots next to every 64-slot word boundary and to both ends of the row"""
    B = {0, 1, 31, 32, 33, 62, 63, S - 2, S - 1}
    for j in range(1, S // 64 + 1):
        B |= {64 * j - 1, 64 * j, 64 * j + 1}
    return sorted(b for b in B if 0 <= b < S)


def structured_rows(S):
    B = boundary_positions(S)
    BS = B + [S]
    rows = [np.ones(S, np.uint8), np.zeros(S, np.uint8)]

    def blocks(*ab):
        r = np.ones(S, np.uint8)
        for a, b in ab:
            r[a:b] = 0
        return r

    for b in B:
        rows.append(blocks((b, b + 1)))
        rows.append(1 - rows[-1])
    for a, b in itertools.combinations(BS, 2):
        rows.append(blocks((a, b)))
        rows.append(1 - rows[-1])
    quads = list(itertools.combinations(BS, 4))
    if len(quads) > 2000:  # (S >= 127: 10^4 - 10^5 quadruples; a fixed sample of them, every edge of B still many times over)
        pick = np.random.RandomState(S).choice(len(quads), 2000, replace=False)
        quads = [quads[k] for k in sorted(pick)]
    for a, b, c, d in quads:
        rows.append(blocks((a, b), (c, d)))
    idx = np.arange(S)
    for period in (2, 3, 4):
        for phase in range(period):
            rows.append((idx % period == phase).astype(np.uint8))
            rows.append(1 - rows[-1])
    nw = (S + 63) // 64
    for pattern in range(1 << nw):  # full words next to empty words
        rows.append(np.repeat([(pattern >> w) & 1 for w in range(nw)], 64)[:S].astype(np.uint8))
    return np.array(rows, np.uint8)


def random_rows(S, per=200):
    rng = np.random.RandomState(1000 + S)
    rows = [(rng.random_sample((per, S)) < d).astype(np.uint8) for d in (0.02, 0.2, 0.5, 0.8, 0.98)]
    for mean in (1, 5, 40, 100):  # alternating runs of geometric length
        lengths = rng.geometric(1.0 / mean, size=(per, S))
        first = rng.randint(0, 2, per)
        out = np.zeros((per, S), np.uint8)
        for r in range(per):
            ends = np.cumsum(lengths[r])
            k = int(np.searchsorted(ends, S)) + 1
            out[r] = np.repeat((np.arange(k) + first[r]) % 2, lengths[r, :k])[:S]
        rows.append(out)
    return np.concatenate(rows)


class Data:
    def __init__(self, W, S):
        self.W, self.S = W, S
        structured = structured_rows(S)
        self.rows = np.concatenate([structured, random_rows(S)])
        self.packed = row_ref.pack(self.rows, W)
        self.ref = row_ref.summary(self.rows)
        rng = np.random.RandomState(7 * S + W)
        # the rows of the kernels that take a parameter per thread: some of every kind
        pick = np.unique(np.concatenate([np.arange(min(40, len(self.rows))), rng.choice(len(self.rows), min(360, len(self.rows)), replace=False)]))
        self.sub = self.rows[pick]
        self.sub_packed = np.ascontiguousarray(self.packed[pick])


@functools.lru_cache(maxsize=None)
def data(W, S):
    return Data(W, S)


def dev_lo(lo):
    return np.where(np.asarray(lo) < 0, NONE_LO, lo)


def words_equal(got, rows01, W, what):
    """got: uint64 [..., W]; rows01: the expected rows as 0/1 [..., <= 64 W]"""
    exp = row_ref.pack(rows01.reshape(-1, rows01.shape[-1]), W).reshape(got.shape)
    bad = np.flatnonzero((got != exp).any(axis=-1).reshape(-1))
    assert len(bad) == 0, "%s: %d differ, first at flat index %d: got %r, expected %r" % (
        what, len(bad), bad[0], got.reshape(-1, W)[bad[0]], exp.reshape(-1, W)[bad[0]])


def ints_equal(got, exp, what, rows=None):
    got, exp = np.asarray(got, np.int64), np.asarray(exp, np.int64)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.flatnonzero((got != exp).reshape(len(got), -1).any(axis=1))
    if len(bad):
        row = "" if rows is None else "; row (used slots): %r" % np.flatnonzero(rows[bad[0]] == 0).tolist()
        raise AssertionError("%s: %d rows differ, first %d: got %r, expected %r%s" % (what, len(bad), bad[0], got[bad[0]], exp[bad[0]], row))


# ---- not gpu: the reference against hand-written rows, and the harness build ------------------------------------------------
def _row(S, *used):
    r = np.ones(S, np.uint8)
    for a, b in used:
        r[a:b] = 0
    return r


HAND = [  # (row, free, nu, nf, lo, hi, occ, fb, longest, edge)
    (_row(8), 8, 0, 1, -1, 0, 0, 0, 8, 2),
    (np.zeros(8, np.uint8), 0, 1, 0, 0, 8, 0, 0, 0, 0),
    (_row(8, (0, 1)), 7, 1, 1, 0, 1, 0, 0, 7, 1),
    (_row(8, (7, 8)), 7, 1, 1, 7, 8, 0, 0, 7, 1),
    (_row(8, (2, 4)), 6, 1, 2, 2, 4, 0, 0, 4, 2),
    (_row(10, (1, 3), (6, 7)), 7, 2, 3, 1, 7, 6, 1, 3, 2),
    (_row(10, (0, 2), (8, 10)), 6, 2, 1, 0, 10, 10, 1, 6, 0),
    (_row(12, (0, 1), (2, 3), (4, 5), (11, 12)), 8, 4, 3, 0, 12, 12, 3, 6, 0),
    (_row(65, (63, 65)), 63, 1, 1, 63, 65, 0, 0, 63, 1),
    (_row(65, (0, 1), (64, 65)), 63, 2, 1, 0, 65, 65, 1, 63, 0),
    (_row(129, (10, 20), (60, 70), (127, 128)), 108, 3, 4, 10, 128, 118, 2, 57, 2),
    (_row(130, (64, 128)), 66, 1, 2, 64, 128, 0, 0, 64, 2),
    (np.array([1, 0] * 5, np.uint8), 5, 5, 5, 1, 10, 9, 4, 1, 1),
]


def test_row_ref_on_hand_written_rows():
    keys = ("free", "nu", "nf", "lo", "hi", "occ", "fb", "longest", "edge")
    for row, *want in HAND:
        one = row_ref.summary_one(row)
        assert [one[k] for k in keys] == want, (row.tolist(), one, want)
        batch = row_ref.summary(row[None, :])
        assert [int(batch[k][0]) for k in keys] == want, (row.tolist(), batch, want)
    r = _row(12, (3, 4), (9, 10))  # free blocks [0, 3) [4, 9) [10, 12)
    assert row_ref.blocks_one(r, 1) == [(0, 3), (4, 9), (10, 12)]
    assert row_ref.blocks_one(r, 3) == [(0, 3), (4, 9)]
    assert row_ref.blocks_one(r, 4) == [(4, 9)]
    assert row_ref.blocks_one(r, 6) == []
    assert row_ref.first_slot_mask_one(r, 3).tolist() == [1, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0]
    assert row_ref.first_slot_mask(r[None, :], 3)[0].tolist() == [1, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0]
    assert row_ref.first_slot_mask_one(r, 2).tolist() == [1, 1, 0, 0, 1, 1, 1, 1, 0, 0, 1, 0]
    below, from_ = row_ref.run_below_from(r[None, :])
    assert below[0].tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 4, 5, 0, 1, 2]
    assert from_[0].tolist() == [3, 2, 1, 0, 5, 4, 3, 2, 1, 0, 2, 1, 0]
    word = np.ones(64, np.uint8)
    assert row_ref.inner_run_one(word) == 0
    word[[5, 20, 27, 60]] = 0  # runs 5 | 14 | 6 | 32 | 3: the two at the ends do not count
    assert row_ref.inner_run_one(word) == 32 and int(row_ref.inner_runs(word[None, :])[0]) == 32
    word[:] = 0
    assert row_ref.inner_run_one(word) == 0 and int(row_ref.inner_runs(word[None, :])[0]) == 0
    word[1:63] = 1
    assert row_ref.inner_run_one(word) == 62 and int(row_ref.inner_runs(word[None, :])[0]) == 62
    p = row_ref.pack(_row(65, (1, 63))[None, :], 2)
    assert p.tolist() == [[(1 << 63) | 1, 1]] and row_ref.unpack(p, 65)[0].tolist() == _row(65, (1, 63)).tolist()


def test_row_ref_batched_equals_one_row_form():
    """The vectorised reference the GPU tests use against the rle() form, on rows of every kind at three slot counts."""
    for W, S in ((1, 63), (2, 65), (5, 129)):
        d = data(W, S)
        pick = np.random.RandomState(S).choice(len(d.rows), 150, replace=False)
        rows = d.rows[pick]
        for k, row in enumerate(rows):
            one = row_ref.summary_one(row)
            assert {key: int(d.ref[key][pick[k]]) for key in one} == one, (S, np.flatnonzero(row == 0).tolist())
        for n in (1, 2, 5, 64):
            got = row_ref.first_slot_mask(rows[:40], n)
            for k in range(40):
                assert got[k].tolist() == row_ref.first_slot_mask_one(rows[k], n).tolist()
        words = row_ref.unpack(row_ref.pack(rows, W)).reshape(-1, 64)
        got = row_ref.inner_runs(words)
        assert got.tolist() == [row_ref.inner_run_one(w) for w in words]


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_harness_cross_compiles_for_gfx950():
    path = harness_path()
    assert os.path.exists(path) and os.path.getsize(path) > 0
    rel = os.path.relpath(path, ROOT)
    assert rel.startswith(os.path.join("optical_rl_gym_amd", "build")), rel  # git-ignored, and not under csrc/ (hashed by the build)
    with open(path, "rb") as f:
        blob = f.read()
    for name in ("basic", "row8", "cached", "inc"):
        for W in SLOTS:
            assert ("rp_%s_w%d" % (name, W)).encode() in blob


def test_row_generation_covers_the_edge_classes():
    """The structured rows really hold what the GPU tests rely on (per slot count): the last slot used and free, block edges on
    every word boundary, blocks across one, rows of at least 8 used blocks."""
    for W, S in CASES:
        d = data(W, S)
        assert len(d.rows) < 12000 and d.packed.shape == (len(d.rows), W)
        assert (row_ref.unpack(d.packed)[:, S:] == 0).all()
        assert (d.rows[:, -1] == 0).any() and (d.rows[:, -1] == 1).any()
        assert (S < 16 or (d.ref["nu"] >= 8).any()) and (d.ref["nu"] == 0).any() and (d.ref["free"] == 0).any()
        for j in range(1, (S - 1) // 64 + 1):
            b = 64 * j
            assert ((d.rows[:, b - 1] == 0) & (d.rows[:, b] == 1)).any() and ((d.rows[:, b - 1] == 1) & (d.rows[:, b] == 0)).any()
            assert ((d.rows[:, b - 1] == 0) & (d.rows[:, b] == 0)).any() and ((d.rows[:, b - 1] == 1) & (d.rows[:, b] == 1)).any()


# ---- gpu ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("W,S", CASES, ids=CASE_IDS)
def test_row_summaries_one_thread_per_row(W, S):
    """link_summary, row_longest_run, row_stat_lane<W, false> (every field, max_empty, edge), row_occ_fb, row_longest_free,
    row_inner_cache, row_popc / row_ctz / row_bitlen / row_starts, word_longest_run and word_longest_run_flat."""
    d = data(W, S)
    R = len(d.rows)
    n_ints = int(harness().rp_basic_ints())
    out = np.zeros((R, n_ints), np.int32)
    starts = np.zeros((R, W), np.uint64)
    wl = np.zeros((R, W, 2), np.int32)
    call("basic", W, d.packed, R, S, out, starts, wl)
    ref = d.ref
    any_free = d.rows.any(axis=1)
    first_free = np.where(any_free, np.argmax(d.rows, axis=1), 64 * W)
    last_free = np.where(any_free, S - np.argmax(d.rows[:, ::-1], axis=1), 0)
    ints_equal(out[:, 0], ref["free"], "row_popc", d.rows)
    ints_equal(out[:, 1], first_free, "row_ctz", d.rows)
    ints_equal(out[:, 2], last_free, "row_bitlen", d.rows)
    ints_equal(out[:, 3], ref["longest"], "row_longest_run", d.rows)
    ints_equal(out[:, 4:6], np.stack([ref["occ"], ref["fb"]], 1), "link_summary", d.rows)
    lane = np.stack([ref["free"], ref["nf"], ref["nu"], dev_lo(ref["lo"]), ref["hi"], ref["occ"], ref["fb"], ref["longest"], ref["edge"]], 1)
    ints_equal(out[:, 6:15], lane, "row_stat_lane<W, false> {free, nf, nu, lo, hi, occ, fb, max_empty, edge}", d.rows)
    ints_equal(out[:, 15:17], np.stack([ref["occ"], ref["fb"]], 1), "row_occ_fb", d.rows)
    ints_equal(out[:, 17], ref["longest"], "row_longest_free", d.rows)
    prev = np.concatenate([np.zeros((R, 1), np.uint8), d.rows[:, :-1]], axis=1)
    words_equal(starts, d.rows & (1 - prev), W, "row_starts")
    words = row_ref.unpack(d.packed).reshape(R * W, 64)
    longest = row_ref.summary(words)["longest"].reshape(R, W)
    ints_equal(wl[:, :, 0], longest, "word_longest_run", d.rows)
    full = words.all(axis=1).reshape(R, W)
    ints_equal(wl[:, :, 1], np.where(full, -1, longest), "word_longest_run_flat (words with a zero bit)", d.rows)
    if W <= 5:
        inner = row_ref.inner_runs(words).reshape(R, W)
        ints_equal(out[:, 18], (inner << (6 * np.arange(W))[None, :]).sum(axis=1), "row_inner_cache", d.rows)


@pytest.mark.gpu
def test_word_longest_run_on_any_word():
    """word_longest_run on any 64-bit word and word_longest_run_flat on every one with a zero bit — not only the words that occur in
    slot rows: 10^4 uniformly random words, 10^4 sparse and 10^4 dense ones (a bit set with probability 0.05 / 0.95), every single
    run of ones and every single run of zeros at every offset, 0 and ~0; against a bit-by-bit run count."""
    rng = np.random.RandomState(64)
    bits = [(rng.random_sample((10000, 64)) < d).astype(np.uint8) for d in (0.5, 0.05, 0.95)]
    runs = np.array([(np.arange(64) >= a) & (np.arange(64) < b) for a in range(64) for b in range(a + 1, 65)], np.uint8)
    bits = np.concatenate(bits + [runs, 1 - runs, np.zeros((1, 64), np.uint8)])
    R = len(bits)
    n_ints = int(harness().rp_basic_ints())
    out, starts, wl = np.zeros((R, n_ints), np.int32), np.zeros((R, 1), np.uint64), np.zeros((R, 1, 2), np.int32)
    call("basic", 1, row_ref.pack(bits, 1), R, 64, out, starts, wl)
    longest = row_ref.summary(bits)["longest"]
    assert longest.max() == 64 and longest.min() == 0 and set(range(65)) <= set(longest.tolist())
    ints_equal(wl[:, 0, 0], longest, "word_longest_run", bits)
    ints_equal(wl[:, 0, 1], np.where(bits.all(axis=1), -1, longest), "word_longest_run_flat (words with a zero bit)", bits)
    ints_equal(out[:, 3], longest, "row_longest_run<1>", bits)
    ints_equal(out[:, 17], longest, "row_longest_free<1>", bits)


@pytest.mark.gpu
@pytest.mark.parametrize("W,S", CASES, ids=CASE_IDS)
def test_eight_lane_row_stat_all_lanes_agree(W, S):
    """row_stat<W, true> + row_longest_run8<W>: lane w of a group holds word w (0 for w >= W), the eight groups of a wavefront hold
    eight different rows (shuffled, so that a carry leaking over row_shr:1 from the group below meets a row it does not belong
    to); every one of the 8 lanes is read back."""
    d = data(W, S)
    order = np.random.RandomState(S).permutation(len(d.rows))
    order = np.concatenate([order, order[:(-len(order)) % 8]])
    rows, packed = d.rows[order], np.ascontiguousarray(d.packed[order])
    out = np.zeros((len(rows), 8, 8), np.int32)
    call("row8", W, packed, len(rows), S, out)
    ref = {k: v[order] for k, v in d.ref.items()}
    exp = np.stack([ref["free"], ref["nf"], ref["nu"], dev_lo(ref["lo"]), ref["hi"], ref["occ"], ref["fb"], ref["longest"]], 1)
    for lane in range(8):
        ints_equal(out[:, lane, :], exp, "row_stat<W, true> / row_longest_run8, lane %d {free, nf, nu, lo, hi, occ, fb, longest}" % lane, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("W,S", CASES, ids=CASE_IDS)
def test_run_search_helpers(W, S):
    """row_runs_ge for n = 1 .. 64, nth_block for want = 1 .. 8, row_shr_small (1 .. 63), row_shr_lt32 (1 .. 31),
    row_run_below / row_run_from for every p in 0 .. S."""
    d = data(W, S)
    rows, packed = d.sub, d.sub_packed
    R = len(rows)
    out = np.zeros((R, 64, W), np.uint64)
    call("runs_ge", W, packed, R, out)
    exp = np.stack([row_ref.first_slot_mask(rows, n) for n in range(1, 65)], axis=1)
    words_equal(out, exp, W, "row_runs_ge (n = 1 .. 64)")

    ns = np.array([1, 2, 3, 5, 8, 13, 31, 32, 33, 63, 64], np.int32)
    got = np.zeros((R, len(ns), 8, 2), np.int32)
    call("nth", W, packed, R, S, ns, len(ns), got)
    want = np.zeros_like(got)
    for r in range(R):
        for k, n in enumerate(ns):
            blocks = row_ref.blocks_one(rows[r], int(n))
            for w in range(1, 9):
                found = min(w, len(blocks))
                want[r, k, w - 1] = (found, blocks[found - 1][0] if found else -1)
    ints_equal(got.reshape(R, -1), want.reshape(R, -1), "nth_block {found, start} for n in %r, want = 1 .. 8" % ns.tolist(), rows)

    small = np.zeros((R, 63, W), np.uint64)
    lt32 = np.zeros((R, 31, W), np.uint64)
    call("shr", W, packed, R, small, lt32)
    full = row_ref.unpack(packed)
    exp = np.zeros((R, 63, 64 * W), np.uint8)
    for st in range(1, 64):
        exp[:, st - 1, :64 * W - st] = full[:, st:]
    words_equal(small, exp, W, "row_shr_small (st = 1 .. 63)")
    words_equal(lt32, exp[:, :31], W, "row_shr_lt32 (st = 1 .. 31)")

    below = np.zeros((R, S + 1), np.int32)
    from_ = np.zeros((R, S + 1), np.int32)
    call("runs", W, packed, R, S, below, from_)
    exp_below, exp_from = row_ref.run_below_from(rows)
    ints_equal(below, exp_below, "row_run_below (p = 0 .. S)", rows)
    ints_equal(from_, exp_from, "row_run_from (p = 0 .. S)", rows)


@pytest.mark.gpu
@pytest.mark.parametrize("W,S", CASES, ids=CASE_IDS)
def test_masks(W, S):
    """row_mask_lo(0 .. 64 W); row_range(s, n) with n = 0, 64 aligned and not, and n > 64; mask2 / mask2_word / mask_words and
    row_apply_mask for n = 1 .. 63 and every s0 with s0 + n <= S."""
    d = data(W, S)
    out = np.zeros((64 * W + 1, W), np.uint64)
    call("mask_lo", W, out)
    words_equal(out, (np.arange(64 * W)[None, :] < np.arange(64 * W + 1)[:, None]).astype(np.uint8), W, "row_mask_lo")

    grid = [(s0, n) for n in range(1, 64) for s0 in range(0, S - n + 1)]
    origins = sorted(set(range(0, S + 1, 1 if S <= 130 else 7)) | set(boundary_positions(S)) | set(range(0, S + 1, 64)))
    grid += [(s, n) for s in origins for n in (0, 64, 65, 100, 128, 129, S) if s + n <= 64 * W]
    s0s = np.array([g[0] for g in grid], np.int32)
    ns = np.array([g[1] for g in grid], np.int32)
    M = len(grid)
    split = (ns >= 1) & (ns <= 63) & (s0s + ns <= S)
    rng = np.random.RandomState(S)
    base = d.packed[rng.randint(0, len(d.packed), M)]
    buf = np.ascontiguousarray(base.copy())
    rng_out, m2 = np.zeros((M, W), np.uint64), np.zeros((M, W), np.uint64)
    words = np.zeros(M, np.uint32)
    call("masks", W, s0s, ns, M, S, rng_out, m2, words, buf)
    idx = np.arange(64 * W)[None, :]
    exp = ((idx >= s0s[:, None]) & (idx < (s0s + ns)[:, None])).astype(np.uint8)
    words_equal(rng_out, exp, W, "row_range")
    words_equal(m2[split], exp[split], W, "mask2 / mask2_word")
    touched = exp.reshape(M, W, 64).any(axis=2)
    ints_equal(words[split], (touched[split] << np.arange(W)[None, :]).sum(axis=1), "mask_words")
    rows01 = row_ref.unpack(base)
    prov = (np.arange(M) & 1) == 1
    applied = np.where(prov[:, None], rows01 & (1 - exp), rows01 | exp)
    words_equal(buf[split], applied[split], W, "row_apply_mask")
    assert (buf[~split] == base[~split]).all()


def _one_mask(rng, row):
    """(s0, n, provision) for a row: a provision inside a free run or a release of (part of) a used block, at most 63 slots, pulled
    towards the ends of the run it sits in"""
    starts, values, lengths = row_ref.rle(row)
    kinds = [v for v in (0, 1) if (values == v).any()]
    v = kinds[rng.randint(len(kinds))]
    k = rng.choice(np.flatnonzero(values == v))
    n = int(rng.randint(1, min(63, lengths[k]) + 1)) if rng.randint(3) else int(min(63, lengths[k]))
    room = int(lengths[k]) - n
    off = (0, room, int(rng.randint(room + 1)))[rng.randint(3)]
    return int(starts[k]) + off, n, v == 1


@pytest.mark.gpu
@pytest.mark.parametrize("W,S", CACHED, ids=CACHED_IDS)
def test_cached_row_stat_lane(W, S):
    """row_stat_lane<W, true> after one mask, with the cache word of the row before the mask and with an all-unknown one: the summary
    is the reference's of the new row; the cache word equals the reference's in every touched word and in every word whose
    entry was known."""
    d = data(W, S)
    rng = np.random.RandomState(3 * S)
    pick = np.concatenate([np.arange(min(60, len(d.rows))), rng.choice(len(d.rows), 700, replace=False)])
    rows0 = d.rows[pick]
    masks = np.array([_one_mask(rng, r) for r in rows0], np.int32)
    s0s, ns = np.ascontiguousarray(masks[:, 0]), np.ascontiguousarray(masks[:, 1])
    rows1 = rows0.copy()
    for r in range(len(rows1)):
        assert (rows1[r, s0s[r]:s0s[r] + ns[r]] == masks[r, 2]).all()
        rows1[r, s0s[r]:s0s[r] + ns[r]] = 1 - masks[r, 2]
    n_ints = int(harness().rp_cached_ints())
    out = np.full((len(rows0), 2, n_ints), -1, np.int32)
    call("cached", W, np.ascontiguousarray(d.packed[pick]), len(rows0), S, s0s, ns, out)
    ref = row_ref.summary(rows1)
    exp = np.stack([ref["free"], ref["nf"], ref["nu"], dev_lo(ref["lo"]), ref["hi"], ref["occ"], ref["fb"], ref["longest"], ref["edge"]], 1)
    inner = row_ref.inner_runs(row_ref.unpack(row_ref.pack(rows1, W)).reshape(-1, 64)).reshape(len(rows1), W)
    idx = np.arange(64 * W)[None, :]
    touched = ((idx >= s0s[:, None]) & (idx < (s0s + ns)[:, None])).reshape(len(rows1), W, 64).any(axis=2)
    for v, what in ((0, "cache of the row before"), (1, "all-unknown cache")):
        ints_equal(out[:, v, :9], exp, "row_stat_lane<W, true>, %s {free, nf, nu, lo, hi, occ, fb, max_empty, edge}" % what, rows1)
        cw = (out[:, v, 9].astype(np.int64)[:, None] >> (6 * np.arange(W))[None, :]) & 63
        must = np.ones_like(touched) if v == 0 else touched
        ints_equal(np.where(must, cw, 0), np.where(must, inner, 0), "cache word after the update, %s" % what, rows1)
        assert ((cw == inner) | (cw == 63)).all()  # a word not searched stays unknown, never wrong
        assert ((out[:, v, 9].astype(np.int64) >> (6 * W)) == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("W,S", CASES, ids=CASE_IDS)
def test_incremental_row_summary_over_a_chain_of_masks(W, S):
    """row_inc_apply: RowInc starts from the reference on row0; 32 masks, each a provision that fits a free run or the release of
    exactly an earlier provision; after each one the row bits and {free, used blocks, first used, last used + 1, longest free run}
    equal the reference computed from scratch."""
    d = data(W, S)
    rng = np.random.RandomState(5 * S)
    has_free = np.flatnonzero(d.ref["free"] > 0)
    pick = np.concatenate([has_free[:30], rng.choice(has_free, 90, replace=False)])
    rows0 = d.rows[pick]
    R, chain = len(rows0), 32
    masks = np.zeros((R, chain, 3), np.int32)
    states = np.zeros((R, chain, S), np.uint8)
    for r in range(R):
        row, held = rows0[r].copy(), []
        for c in range(chain):
            starts, values, lengths = row_ref.rle(row)
            free_runs = np.flatnonzero(values == 1)
            if held and (len(free_runs) == 0 or rng.randint(2)):
                s0, n = held.pop(rng.randint(len(held)))
                row[s0:s0 + n] = 1
                masks[r, c] = (s0, n, 0)
            else:
                k = rng.choice(free_runs)
                n = int(rng.randint(1, min(63, lengths[k]) + 1)) if rng.randint(4) else int(min(63, lengths[k]))
                room = int(lengths[k]) - n
                s0 = int(starts[k]) + (0, room, int(rng.randint(room + 1)))[rng.randint(3)]
                row[s0:s0 + n] = 0
                held.append((s0, n))
                masks[r, c] = (s0, n, 1)
            states[r, c] = row
    ref0 = {k: v[pick] for k, v in d.ref.items()}
    init = np.ascontiguousarray(np.stack([ref0["free"], ref0["nu"], dev_lo(ref0["lo"]), ref0["hi"], ref0["longest"]], 1).astype(np.int32))
    out_rows = np.zeros((R, chain, W), np.uint64)
    out_fields = np.full((R, chain, 5), -1, np.int32)
    call("inc", W, np.ascontiguousarray(d.packed[pick]), R, S, init, masks, chain, out_rows, out_fields)
    words_equal(out_rows, states, W, "row bits after each mask")
    ref = row_ref.summary(states.reshape(R * chain, S))
    exp = np.stack([ref["free"], ref["nu"], dev_lo(ref["lo"]), ref["hi"], ref["longest"]], 1).reshape(R, chain, 5)
    for c in range(chain):
        ints_equal(out_fields[:, c], exp[:, c], "RowInc {free, nu, lo, hi, longest} after mask %d of the chain (masks {s0, n, provision}: see the test)" % c,
                   states[:, c])
