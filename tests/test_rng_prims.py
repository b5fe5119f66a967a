"""The device's random draws, called directly (tests/csrc/rng_prims.hip wraps them in thin kernels) and compared bit for bit with
CPython's random module on the same generator states (tests/mt_craft.py): orl_log against math.log; the word streams of the
32-word (Rng) and 16-word (RngG) windows from every position; random / expovariate / choices / randint in both forms, with ties
on cumulative weights, table sizes around every loop bound and rejection runs across window refills; and svc_generate, the
persistent kernel's look-ahead, with the window's wrap at every offset, services whose accepting word is the last word of the
96-word window or the first one behind it, and the flagged state in which not even the first service fits.  The log and
svc_generate cases run on two builds of the harness: the library's flags, and those plus the specialisations' (_build.SPEC_TUNING).

No tolerance anywhere: integers with ==, floats as their uint64 bit patterns."""
import ctypes as C
import functools
import hashlib
import math
import os
import random
import subprocess

import numpy as np
import pytest

from tests import mt_craft as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "rng_prims.hip")
OP_RANDOM, OP_EXPO, OP_CHOICE, OP_CHOICE_PRE, OP_RANDBELOW = range(5)
NEG_ZERO = 1 << 63


# ---- the harness ------------------------------------------------------------------------------------------------------------
def harness_path(tuned=False):
    """tests/csrc/rng_prims.hip compiled for gfx950 into the package's build directory, keyed by the unit, the compiler's arguments
    and _build.source_hash(); tuned: with the extra flags of the JIT specialisations.  Libraries of other keys are dropped."""
    from optical_rl_gym_amd import _build

    args = _build.HIPCC_FLAGS + (_build.SPEC_TUNING if tuned else []) + ["-I", _build.CSRC, "-shared"]
    with open(SRC, "rb") as f:
        key = hashlib.sha256(f.read() + " ".join(args).encode() + _build.source_hash().encode()).hexdigest()[:16]
    directory = os.path.join(_build.HERE, "build")
    prefix = "rng_prims_tuned_" if tuned else "rng_prims_plain_"
    out = os.path.join(directory, "%s%s.so" % (prefix, key))
    if not os.path.exists(out):
        os.makedirs(directory, exist_ok=True)
        tmp = out + ".tmp.%d" % os.getpid()
        subprocess.check_call([_build.hipcc_path()] + args + [SRC, "-o", tmp])
        os.replace(tmp, out)
    for name in os.listdir(directory):
        if name.startswith(prefix) and name.endswith(".so") and name != os.path.basename(out):
            os.unlink(os.path.join(directory, name))
    return out


@functools.lru_cache(maxsize=None)
def harness(tuned=False):
    from optical_rl_gym_amd import _lib

    _lib.lib()  # first: it brings in the one HIP runtime the process shares with PyTorch
    lib = C.CDLL(harness_path(tuned))
    p, i, d = C.c_void_p, C.c_int, C.c_double
    lib.rg_log.argtypes, lib.rg_log.restype = [p, p, C.c_longlong], i
    lib.rg_words.argtypes, lib.rg_words.restype = [i, p, p, i, i, i, p], i
    lib.rg_draw.argtypes, lib.rg_draw.restype = [i, p, p, i, i, i, d, p, i, i, i, p], i
    lib.rg_svc.argtypes, lib.rg_svc.restype = [i, i, p, p, i, i, i, p, d, d, p, i, p, p, p, p, p, p, p, p], i
    lib.rg_consts.argtypes, lib.rg_consts.restype = [p], None
    return lib


@functools.lru_cache(maxsize=None)
def consts():
    out = (C.c_longlong * 8)()
    harness().rg_consts(out)
    return dict(scal_words=out[0], mtpos=out[1], flags=out[2], ev_overflow=out[3], window=out[4], sent_pk=out[5], sent_cnt=out[6],
                sent_f64=out[7])


def _p(a):
    return None if a is None else a.ctypes.data


# ---- states -------------------------------------------------------------------------------------------------------------------
def device_form(states):
    """[nc][625] CPython states -> (mt [nc][624] uint32, pos [nc] int32) as the device keeps them"""
    conv = [mc.to_update_behind(s) for s in states]
    return np.ascontiguousarray(np.array([c[0] for c in conv], np.uint32)), np.array([c[1] for c in conv], np.int32)


def check_final(tag, rngs, mt, pos):
    """the arrays and positions the kernel left against CPython's generators after the same draws: whole-array =="""
    exp_mt, exp_pos = device_form([mc.state_of(g) for g in rngs])
    bad = np.flatnonzero(pos != exp_pos)
    assert len(bad) == 0, "%s: position of case %d: got %d, expected %d (%d cases differ)" % (tag, bad[0], pos[bad[0]], exp_pos[bad[0]], len(bad))
    bad = np.argwhere(mt != exp_mt)
    assert len(bad) == 0, "%s: state array of case %d differs first at word %d (%d words differ)" % (tag, bad[0][0], bad[0][1], len(bad))


@functools.lru_cache(maxsize=None)
def states_at_every_position():
    return np.array([mc.craft(p, [], 9000 + p) for p in range(624)], np.uint32)


def pad8(states):
    states = list(states)
    while len(states) % 8:
        states.append(states[0])
    return np.array(states, np.uint32)


# ---- not gpu ------------------------------------------------------------------------------------------------------------------
def log_inputs():
    """The inputs of the log test: both ends of the near-1 branch +- 4 ulp, the first and last double of each of the 128 table
    intervals and their neighbours at exponents 0, -1, -26 and -52, 1.0, nextafter(1, 0), 2^-53, and 2^20 values 1 - k / 2^53
    with k from CPython's generator (what expovariate passes)."""
    ix = []
    for edge in (0x3FEE000000000000, 0x3FEE000000000000 + 0x0003090000000000):
        ix += [edge + d for d in range(-4, 5)]
    off = 0x3FE6000000000000
    for k in (0, -1, -26, -52):
        for i in range(128):
            base = off + (k << 52) + (i << 45)
            ix += [base - 1, base, base + 1, base + (1 << 45) - 2, base + (1 << 45) - 1, base + (1 << 45)]
    x = np.array(ix, np.uint64).view(np.float64)
    special = np.array([1.0, np.nextafter(1.0, 0.0), 2.0**-53])
    r = random.Random(2024)
    bulk = 1.0 - np.array([r.getrandbits(53) for _ in range(1 << 20)], np.float64) / 2.0**53
    return np.ascontiguousarray(np.concatenate([x, special, bulk]))


def test_log_inputs_cover_the_edges():
    x = log_inputs()
    assert len(x) >= 10**6 and (x > 0).all() and np.isfinite(x).all() and (x >= 2.0**-1022).all()
    ix = x.view(np.uint64)
    near = (ix - np.uint64(0x3FEE000000000000)) < np.uint64(0x0003090000000000)
    assert near.any() and (~near).any() and (x == 1.0).any() and (x == 2.0**-53).any()
    tab = ((ix - np.uint64(0x3FE6000000000000)) >> np.uint64(45)) & np.uint64(127)
    assert set(tab[~near].tolist()) == set(range(128))


def dyadic_weights(n, rs):
    """weights that are multiples of 1 / 64 and sum to exactly 1.0 (so do their partial sums: every cum entry is exact)"""
    units = np.zeros(n, np.int64)
    if n <= 64:
        units += 1
        units += rs.multinomial(64 - n, np.full(n, 1.0 / n))
    else:
        units[rs.choice(n, 64, replace=False)] = 1
    return units / 64.0


def weight_sets(n):
    rs = np.random.RandomState(n)
    sets = {"uniform": np.full(n, 1.0 / n), "skewed": rs.dirichlet(np.full(n, 0.3)) + 1e-12, "dyadic": dyadic_weights(n, rs)}
    z = rs.random_sample(n) + 0.05
    if n >= 2:
        z[0] = 0.0
    if n >= 3:
        z[-1] = 0.0
    if n >= 5:
        z[[n // 2, n // 2 + 1]] = 0.0
    sets["zeros"] = z
    return sets


CHOICE_SIZES = (1, 2, 8, 9, 10, 32, 33, 34, 64, 65, 66, 72, 73, 74, 129, 130)


def choice_states(n, name, w, nc=64, reps=8):
    """nc states for a table: natural streams at spread positions; dyadic tables get random() == k / 64 for every k, so that
    x == cum[i] exactly"""
    states = []
    for c in range(nc):
        p = (c * 41 + n) % 625
        if name == "dyadic":
            outs = []
            for j in range(reps):
                outs += mc.u_exact(((c * reps + j) % 64) << 47)
            states.append(mc.craft(p, outs, 100 * n + c))
        else:
            states.append(mc.craft(p, [], 100 * n + c))
    return np.array(states, np.uint32)


def test_dyadic_tables_produce_ties():
    for n in CHOICE_SIZES:
        w = weight_sets(n)["dyadic"]
        cum = mc.cum_weights(w)
        assert cum[-1] == 1.0 and (np.round(cum * 64) == cum * 64).all()
        zeros = weight_sets(n)["zeros"]
        assert n < 2 or (np.diff(mc.cum_weights(zeros)) == 0).any() or mc.cum_weights(zeros)[0] == 0.0
        if n < 2:
            continue
        ties = 0
        for s in choice_states(n, "dyadic", w):
            g = mc.py_rng(s)
            for _ in range(8):
                x = g.random() * (cum[-1] + 0.0)
                ties += int((cum[:n - 1] == x).any())
        assert ties >= 1, n


# ---- gpu: orl_log -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tuned", [False, True], ids=["lib_flags", "spec_flags"])
def test_device_log_equals_libm(tuned):
    x = log_inputs()
    out = np.zeros_like(x)
    assert harness(tuned).rg_log(_p(x), _p(out), len(x)) == 0
    exp = np.array([math.log(v) for v in x.tolist()])
    bad = np.flatnonzero(mc.bits(out) != mc.bits(exp))
    print("orl_log on the device: %d inputs, %d mismatches" % (len(x), len(bad)))
    assert len(x) >= 10**6
    assert len(bad) == 0, "first mismatch: log(%r) = %r on the device, %r from libm" % (x[bad[0]], out[bad[0]], exp[bad[0]])


# ---- gpu: word streams ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 32, 33, 64, 700])
@pytest.mark.parametrize("form", ["wave64", "group8", "group8_split"])
def test_word_stream_from_every_position(form, n):
    states = states_at_every_position()
    mt, pos = device_form(states)
    assert pos.tolist() == list(range(624))
    words = np.zeros((624, n), np.uint32)
    rc = harness().rg_words(64 if form == "wave64" else 8, _p(mt), _p(pos), 624, n, int(form == "group8_split"), _p(words))
    assert rc == 0, "HIP error %d" % rc
    rngs = [mc.py_rng(s) for s in states]
    exp = np.array([[g.getrandbits(32) for _ in range(n)] for g in rngs], np.uint32)
    bad = np.argwhere(words != exp)
    assert len(bad) == 0, "position %d: word %d is %#x, CPython's %#x (%d differ)" % (
        bad[0][0], bad[0][1], words[tuple(bad[0])], exp[tuple(bad[0])], len(bad))
    check_final("%s, n = %d" % (form, n), rngs, mt, pos)


# ---- gpu: random / expovariate / choices / randint ------------------------------------------------------------------------------
def draw(lanes, states, op, reps, lam=0.0, cum=None, n=0, rand_n=0, rand_bits=0):
    mt, pos = device_form(states)
    out = np.zeros((len(states), reps), np.uint64)
    cum = None if cum is None else np.ascontiguousarray(cum, np.float64)
    rc = harness().rg_draw(lanes, _p(mt), _p(pos), len(states), op, reps, lam, _p(cum), n, rand_n, rand_bits, _p(out))
    assert rc == 0, "HIP error %d" % rc
    return out, mt, pos


def values_equal(tag, got, exp):
    bad = np.argwhere(got != exp)
    assert len(bad) == 0, "%s: case %d, draw %d: got %#x, expected %#x (%d differ)" % (
        tag, bad[0][0], bad[0][1], int(got[tuple(bad[0])]), int(exp[tuple(bad[0])]), len(bad))


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [64, 8])
def test_random_and_expovariate(lanes):
    """Natural streams from spread positions, and random() == 0 / 1 - 2^-53 as the first, the last and an inner pair of words of a
    window and of the windows behind it."""
    W = 32 if lanes == 64 else 16
    reps = 24
    states = [mc.craft((c * 29) % 625, [], 300 + c) for c in range(40)]
    for c, (at, u) in enumerate([(0, mc.U_ZERO), (0, mc.U_MAX), (2, mc.U_ZERO), (W - 2, mc.U_MAX), (W, mc.U_ZERO), (2 * W - 2, mc.U_ZERO),
                                 (2 * W, mc.U_MAX), (6, mc.U_ZERO + mc.U_MAX + mc.U_ZERO)]):
        states.append(mc.craft((c * 83 + 570) % 625, u, 400 + c, at=at))
    states = np.array(states, np.uint32)
    assert len(states) % 8 == 0
    lam = 1 / (1 / float(10 / float(10800.0)))
    for op, fn in ((OP_RANDOM, lambda g: g.random()), (OP_EXPO, lambda g: g.expovariate(lam))):
        rngs = [mc.py_rng(s) for s in states]
        exp = mc.bits(np.array([[fn(g) for _ in range(reps)] for g in rngs]))
        if op == OP_EXPO:
            assert (exp == NEG_ZERO).sum() >= 5  # -log(1.0) / lambd = -0.0
        else:
            assert (exp == 0).sum() >= 5 and (exp == mc.bits([1 - 2.0**-53])[0]).sum() >= 3
        got, mt, pos = draw(lanes, states, op, reps, lam=lam)
        values_equal("op %d, %d lanes" % (op, lanes), got, exp)
        check_final("op %d, %d lanes" % (op, lanes), rngs, mt, pos)


@pytest.mark.gpu
@pytest.mark.parametrize("n", CHOICE_SIZES)
@pytest.mark.parametrize("lanes", [64, 8])
def test_choices(lanes, n):
    """random.choices over a table of n weights: uniform, skewed, with zero weights inside and at both ends (duplicate cumulative
    entries), and dyadic weights with random() == k / 64 (x equal to a cumulative entry: bisect_right goes past it).  The 64-lane
    form also through rng_choice_pre where the table fits the lanes."""
    reps = 8
    for name, w in weight_sets(n).items():
        cum = mc.cum_weights(w)
        states = choice_states(n, name, w, reps=reps)
        ops = [OP_CHOICE] + ([OP_CHOICE_PRE] if lanes == 64 and n <= 64 else [])
        for op in ops:
            rngs = [mc.py_rng(s) for s in states]
            exp = np.array([[g.choices(range(n), weights=w)[0] for _ in range(reps)] for g in rngs], np.uint64)
            got, mt, pos = draw(lanes, states, op, reps, cum=cum, n=n)
            tag = "%s weights, n = %d, %d lanes, op %d" % (name, n, lanes, op)
            values_equal(tag, got, exp)
            check_final(tag, rngs, mt, pos)
            if n == 1:  # a single-entry table returns 0 and still draws: two words each
                _mt0, pos0 = device_form(states)
                assert ((pos - pos0) % 624 == 2 * reps).all() and (got == 0).all()


RANDBELOW_N = (1, 2, 3, 51, 64, 65, 76, 127, 128, 129, 4096)


@pytest.mark.gpu
@pytest.mark.parametrize("rand_n", RANDBELOW_N)
@pytest.mark.parametrize("lanes", [64, 8])
def test_randint_rejection_loop(lanes, rand_n):
    """_randbelow as next_service writes it, on natural words and on crafted runs of rejected words that start at window offset s
    and end with the accepted word as the last word of a window, the first of the next, and up to three windows on."""
    W = 32 if lanes == 64 else 16
    rb = mc.rand_bits_of(rand_n)
    reps = W + 2
    states = [mc.craft((c * 53 + rand_n) % 625, [], 700 + c) for c in range(32)]
    placed = []
    for s in (0, 1, 3, W - 1):
        for a in (W - 1, W, W + 1, 2 * W - 1, 2 * W, 3 * W - 1, 3 * W):
            if a < s:
                continue
            outs = [mc.accept_word(rand_n, rb, k % rand_n, low=k) for k in range(s)]
            outs += [mc.reject_word(rand_n, rb, k, low=77 * k) for k in range(a - s)] + [mc.accept_word(rand_n, rb, rand_n - 1, low=a)]
            states.append(mc.craft((len(states) * 19 + 500) % 625, outs, 800 + len(states)))
            placed.append((len(states) - 1, s, a))
    states = pad8(states)
    rngs = [mc.py_rng(s) for s in states]
    exp = np.array([[g.randint(0, rand_n - 1) for _ in range(reps)] for g in rngs], np.uint64)
    for c, s, a in placed:  # draw number s of the case consumed the run: its accepted word is stream word a
        assert exp[c, s] == rand_n - 1 and (s == 0 or exp[c, s - 1] == (s - 1) % rand_n)
    got, mt, pos = draw(lanes, states, OP_RANDBELOW, reps, rand_n=rand_n, rand_bits=rb)
    tag = "rand_n = %d, %d lanes" % (rand_n, lanes)
    values_equal(tag, got, exp)
    check_final(tag, rngs, mt, pos)  # (the position: the words consumed)


# ---- gpu: svc_generate ----------------------------------------------------------------------------------------------------------
KIND_FAMILY = {0: "RMSA", 1: "RMSA", 2: "RWA"}
SVC_POSITIONS = [0, 1] + list(range(520, 624))


def node_tables(N, skewed):
    rs = np.random.RandomState(N)
    probs = np.full(N, 1.0 / N) if not skewed else rs.dirichlet(np.full(N, 0.5)) + 1e-9
    cum_src = mc.cum_weights(probs)
    cum_dst = np.array([mc.cum_weights(mc.dst_weights(probs, s)) for s in range(N)])
    return probs, cum_src, np.ascontiguousarray(cum_dst)


def svc_cfg(kind, N, rand_n=76, skewed=False):
    probs, cum_src, cum_dst = node_tables(N, skewed)
    cfg = dict(probs=probs, lambda_a=1 / (1 / float(10 / float(10800.0))), lambda_h=1 / 10800.0, cum_src=cum_src, cum_dst=cum_dst)
    if kind == 0:
        cfg.update(mode="continuous", lo=0, hi=rand_n - 1, rand_n=rand_n, rand_bits=mc.rand_bits_of(rand_n))
    elif kind == 1:
        cfg.update(mode="discrete", bit_rates=[10, 40, 100, 400], bit_rate_probs=[0.25, 0.5, 0.0, 0.25])
        cfg["cum_br"] = mc.cum_weights(cfg["bit_rate_probs"])
    return cfg


def run_svc(tuned, kind, cfg, cases):
    """cases: list of dict(state, n_want, active, rates or None).  Launches svc_generate once over them (padded with inactive
    groups to whole wavefronts) and compares everything it returns with CPython.  Returns got per case, and the states the active
    cases were left in (as CPython states) for a second call."""
    K = consts()
    fam = KIND_FAMILY[kind]
    cases = list(cases)
    while len(cases) % 8:
        cases.append(dict(state=cases[0]["state"], n_want=8, active=False, rates=cases[0].get("rates")))
    nc = len(cases)
    mt, pos = device_form([c["state"] for c in cases])
    mt0 = mt.copy()
    rs = np.random.RandomState(nc)
    rec = rs.randint(0, 2**62, size=(nc, K["scal_words"])).astype(np.uint64)
    rec[:, K["mtpos"]] = (np.arange(nc) + 7).astype(np.uint64) | (pos.astype(np.uint64) << np.uint64(32))
    rec[:, K["flags"]] = np.uint64(1) | (np.uint64(4) << np.uint64(32))  # (new_service set; another flag that must survive)
    rec0 = rec.copy()
    n_want = np.array([c["n_want"] for c in cases], np.int32)
    active = np.array([c["active"] for c in cases], np.uint8)
    per_env = cases[0].get("rates") is not None
    rates = np.ascontiguousarray(np.array([c["rates"] for c in cases], np.float64)) if per_env else None
    q, ht = np.zeros((nc, 8), np.uint64), np.zeros((nc, 8), np.uint64)
    pk, cnt = np.zeros((nc, 8), np.uint32), np.zeros((nc, 8), np.int32)
    rc = harness(tuned).rg_svc(kind, len(cfg["probs"]), _p(cfg["cum_src"]), _p(cfg["cum_dst"]), cfg.get("rand_n", 0), cfg.get("rand_bits", 0),
                               len(cfg.get("bit_rates", [])), _p(cfg.get("cum_br")), cfg["lambda_a"], cfg["lambda_h"], _p(rates), nc,
                               _p(rec), _p(mt), _p(n_want), _p(active), _p(q), _p(ht), _p(pk), _p(cnt))
    assert rc == 0, "HIP error %d" % rc
    gots, after = [], []
    for c, case in enumerate(cases):
        tag = "case %d (pos %d, n_want %d)" % (c, pos[c], n_want[c])
        e_q = np.full(8, K["sent_f64"], np.uint64)
        e_ht, e_pk, e_cnt = e_q.copy(), np.full(8, K["sent_pk"], np.uint32), np.full(8, K["sent_cnt"], np.int32)
        e_rec, e_mt = rec0[c].copy(), mt0[c]
        if not case["active"]:
            gots.append(None)
            after.append(None)
        else:
            ccfg = dict(cfg)
            if per_env:
                ccfg["lambda_a"], ccfg["lambda_h"] = case["rates"]
            d = mc.draw_services(mc.py_rng(case["state"]), fam, ccfg, int(n_want[c]))
            got = int((d["words"] <= K["window"]).sum())
            g = mc.py_rng(case["state"])
            mc.draw_services(g, fam, ccfg, got)
            after.append(mc.state_of(g))
            gots.append(got)
            e_mt, e_pos = mc.to_update_behind(after[-1])
            e_rec[K["mtpos"]] = (e_rec[K["mtpos"]] & np.uint64(0xFFFFFFFF)) | (np.uint64(e_pos) << np.uint64(32))
            e_cnt[:] = got << 8
            e_q[:got], e_ht[:got] = mc.bits(d["q"][:got]), mc.bits(d["ht"][:got])
            e_pk[:got] = d["src"][:got] | (d["dst"][:got] << 10) | (d["br_idx"][:got] << 20)
            if got == 0 and n_want[c] > 0:  # not even the first service fits the window: flagged, nothing drawn, empty services
                e_rec[K["flags"]] |= np.uint64(K["ev_overflow"]) << np.uint64(32)
                e_cnt[:] = int(n_want[c]) << 8
                e_q[:], e_ht[:], e_pk[:] = 0, 0, 0
        assert cnt[c].tolist() == e_cnt.tolist(), "%s: cnt %r, expected %r" % (tag, cnt[c], e_cnt)
        assert pk[c].tolist() == e_pk.tolist(), "%s: pk %r, expected %r" % (tag, pk[c], e_pk)
        assert q[c].tolist() == e_q.tolist(), "%s: inter-arrival times (bits) %r, expected %r" % (tag, q[c], e_q)
        assert ht[c].tolist() == e_ht.tolist(), "%s: holding times (bits) %r, expected %r" % (tag, ht[c], e_ht)
        assert rec[c].tolist() == e_rec.tolist(), "%s: record words differ at %r" % (tag, np.flatnonzero(rec[c] != e_rec))
        assert (mt[c] == e_mt).all(), "%s: state array differs first at word %d" % (tag, np.flatnonzero(mt[c] != e_mt)[0])
    return gots, after, cases


def natural_cases(seed, n_want=None, per_env=False):
    cases = []
    for k, p in enumerate(SVC_POSITIONS):
        cases.append(dict(state=mc.craft(p, [], seed + p), n_want=k % 9 if n_want is None else n_want, active=k % 11 != 5,
                          rates=(0.001 + 0.0007 * k, 1 / (20.0 + k)) if per_env else None))
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("tuned", [False, True], ids=["lib_flags", "spec_flags"])
@pytest.mark.parametrize("N", [2, 9, 10, 14, 50, 73, 74, 129])
@pytest.mark.parametrize("kind", [0, 1, 2], ids=["randint", "discrete", "rwa"])
def test_svc_generate_on_natural_streams(kind, N, tuned):
    """n_want 0 .. 8, the window's wrap at every offset (pos 520 .. 623), node tables on both sides of svc_choice's bounds (N - 1 = 8 / 9,
    72 / 73), inactive groups; per-env rates for every other table size, the two scalars for the rest; skewed tables for odd N."""
    cfg = svc_cfg(kind, N, skewed=bool(N & 1))
    gots, _after, cases = run_svc(tuned, kind, cfg, natural_cases(1000 * kind + N, per_env=N in (9, 14, 73, 129)))
    assert {c["n_want"] for c in cases if c["active"]} == set(range(9)) and any(not c["active"] for c in cases)
    assert any(g == c["n_want"] and g > 0 for g, c in zip(gots, cases) if g is not None)


@pytest.mark.gpu
@pytest.mark.parametrize("tuned", [False, True], ids=["lib_flags", "spec_flags"])
@pytest.mark.parametrize("rand_n", [1, 64, 65, 76])
def test_svc_generate_randint_ranges(rand_n, tuned):
    cfg = svc_cfg(0, 14, rand_n=rand_n)
    run_svc(tuned, 0, cfg, natural_cases(50 + rand_n, n_want=8))


def layout_state(p, ends, rn, rb, fill):
    """A state at index p in which service k's accepted randint word is stream word ends[k]: its 8 fixed words follow the service
    before it, every word between them and ends[k] is rejected."""
    runs, start = {}, 0
    for k, end in enumerate(ends):
        assert end >= start + 8
        runs[start + 8] = [mc.reject_word(rn, rb, i, low=31 * i + k) for i in range(end - start - 8)] + [mc.accept_word(rn, rb, (11 * k + end) % rn, low=end)]
        start = end + 1
    return mc.craft_many(p, runs, fill)


def placed_state(p, j, T, rn, rb, fill):
    """services 0 .. j - 1 take 9 words each (their randint word accepted at once), service j's accepted word is stream word T"""
    return layout_state(p, [9 * k + 8 for k in range(j)] + [T], rn, rb, fill)


@pytest.mark.gpu
@pytest.mark.parametrize("tuned", [False, True], ids=["lib_flags", "spec_flags"])
def test_svc_generate_at_the_end_of_the_window(tuned):
    """Service j's accepted randint word at stream word 63, 64, 65 (the 64-bit halves of the accept bits), 95 (the window's last word:
    the service is produced) and 96 (it does not fit: got == j, its words stay uncommitted and a second call draws it), for
    j = 0, 3, 7 where 9 j + 8 <= T (a service takes 8 words before its randint: service 7 cannot end before word 71).  88 and more
    rejected words behind the first service's 8: got == 0, the env is flagged ORL_FLAG_EV_OVERFLOW, its stream stays where it was,
    cnt == n_want << 8 with empty services.  random() == 0 and 1 - 2^-53 in the time draws: -0.0 and -log(2^-53) / lambd."""
    rn, rb = 76, 7
    cfg = svc_cfg(0, 14, rand_n=rn)
    cases, want = [], []
    for j in (0, 3, 7):
        for T in (63, 64, 65, 95, 96):
            if 9 * j + 8 > T:
                continue
            for p in (0, 560, 600, 623):
                cases.append(dict(state=placed_state(p, j, T, rn, rb, 40 * T + j + p), n_want=8, active=True))
                want.append(("placed", j, T))
    # the services before service j end with stream word O - 1, so that service j's randint words start at c = O + 8: c = 31 / 32
    # (below 32 the window's last words are looked up apart), 63 / 64 / 65 (the halves of the accept bits), 94 .. 98 (c = 95: the
    # last word the window has; c = 96: none is left); accepted at once, and after rejected words at the window's last word / behind it
    for O in (23, 24, 55, 56, 57, 86, 87, 88, 89, 90):
        j = 2 if O < 50 else 4
        before = [9 * k + 8 for k in range(j - 1)] + [O - 1]
        for T in sorted({O + 8, 95, 96}):
            if T < O + 8:
                continue
            for p in (0, 577):
                cases.append(dict(state=layout_state(p, before + [T], rn, rb, 1000 + 10 * O + T + p), n_want=8, active=True))
                want.append(("placed", j, T))
    for extra in (0, 1, 40):  # 88 + extra rejected words
        for n_want in (1, 8):
            for p in (3, 530, 622):
                runs = {8: [mc.reject_word(rn, rb, k, low=k) for k in range(88 + extra)] + [mc.accept_word(rn, rb, 5)]}
                cases.append(dict(state=mc.craft_many(p, runs, 7 * p + extra), n_want=n_want, active=True))
                want.append(("none", 0, 96 + extra))
    for j in (0, 2, 7):  # time-draw edges in service j (its first four words), accepted randint words around it
        for at, u in ((0, mc.U_ZERO), (2, mc.U_ZERO), (0, mc.U_MAX), (2, mc.U_MAX), (0, mc.U_ZERO + mc.U_ZERO)):
            runs = {9 * k + 8: [mc.accept_word(rn, rb, k, low=k)] for k in range(8)}
            runs[9 * j + at] = list(u)
            cases.append(dict(state=mc.craft_many(590 + j, runs, 60 + j + at), n_want=8, active=True))
            want.append(("edge", j, at))
    gots, after, cases = run_svc(tuned, 0, cfg, cases)
    second = []
    for (what, j, T), got, st, case in zip(want, gots, after, cases):
        if what == "placed":
            assert (got == j) if T >= 96 else (got > j), (what, j, T, got)  # (T <= 95: the service is produced)
            if T >= 96 and j > 0:
                second.append(dict(state=st, n_want=8 - j, active=True))
        elif what == "none":
            assert got == 0
        else:
            assert got == 8
            d = mc.draw_services(mc.py_rng(case["state"]), "RMSA", cfg, 8)
            field = d["q"] if T == 0 else d["ht"]
            assert mc.bits([field[j]])[0] in (NEG_ZERO, mc.bits([-math.log(2.0**-53) / (cfg["lambda_a"] if T == 0 else cfg["lambda_h"])])[0])
    real = [(g, c["n_want"]) for g, c in zip(gots, cases) if g is not None]
    assert any(g == w > 0 for g, w in real) and any(0 < g < w for g, w in real) and any(g == 0 and w > 0 for g, w in real)
    assert second
    gots2, _a, _c = run_svc(tuned, 0, cfg, second)  # the service that did not fit is drawn by the next call, from the same words
    assert all(g >= 1 for g in gots2 if g is not None)


@pytest.mark.gpu
@pytest.mark.parametrize("tuned", [False, True], ids=["lib_flags", "spec_flags"])
@pytest.mark.parametrize("kind", [1, 2], ids=["discrete", "rwa"])
def test_svc_generate_time_edges_without_randint(kind, tuned):
    """random() == 0 / 1 - 2^-53 in the time draws of services 0, 3 and 7 of the fixed-length families (10 / 8 words a service), and
    — discrete bit rates — random() == k / 4 on the bit-rate table's cumulative entries (one of them a duplicate)."""
    cfg = svc_cfg(kind, 10)
    fixed = 10 if kind == 1 else 8
    cases = []
    for j in (0, 3, 7):
        for at, u in ((0, mc.U_ZERO), (2, mc.U_ZERO), (0, mc.U_MAX), (2, mc.U_MAX)):
            runs = {fixed * j + at: list(u)}
            if kind == 1:
                runs[fixed * j + 8] = mc.u_exact(((j + at) % 4) << 51)
            cases.append(dict(state=mc.craft_many(540 + 9 * j + at, runs, 90 + j + at), n_want=8, active=True))
    gots, _after, cases = run_svc(tuned, kind, cfg, cases)
    assert all(g == 8 for g in gots if g is not None)
    d = [mc.draw_services(mc.py_rng(c["state"]), KIND_FAMILY[kind], cfg, 8) for c in cases if c["active"]]
    assert sum(int((mc.bits(x["q"]) == NEG_ZERO).sum() + (mc.bits(x["ht"]) == NEG_ZERO).sum()) for x in d) >= 6
