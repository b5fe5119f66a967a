"""Crafted MT19937 states: CPython's random.Random set to a state whose next outputs are words the test chose.

MT19937's tempering is a bijection on 32-bit words, and random.Random().setstate((3, words + (index,), None)) accepts any 624
words and any index in 0 .. 624, so a test can put any word at any place of the stream: a run of rejected randint draws of a
chosen length, random() == 0 or 1 - 2^-53, a choices() draw that lands exactly on a cumulative weight.  CPython's own random
module, set to the same state, is the reference of everything the device draws.  Pure Python + numpy, no GPU.

Written from the MT19937 definition (Matsumoto & Nishimura 1998; CPython Modules/_randommodule.c genrand_uint32): the state is
624 words mt[] and an index; output number k of a generation is temper(mt[k]); when the index reaches 624 the whole array is
replaced by the next generation, new[i] = new-or-old[(i + 397) % 624] ^ twist(upper bit of old[i], lower 31 bits of
old-or-new[i + 1]), computed in place for i = 0 .. 623."""
import itertools
import random

import numpy as np

N, M = 624, 397
MAG = 0x9908B0DF
MASK32 = 0xFFFFFFFF


def temper(y):
    y = int(y) & MASK32
    y ^= y >> 11
    y ^= (y << 7) & 0x9D2C5680
    y ^= (y << 15) & 0xEFC60000
    y ^= y >> 18
    return y & MASK32


def untemper(y):
    y = int(y) & MASK32
    y ^= y >> 18  # (the shifted-in part is the untouched top 18 bits)
    y ^= (y << 15) & 0xEFC60000  # (bits 15.. take bits 0..16, which this step does not change)
    x = y
    for _ in range(5):  # y = x ^ ((x << 7) & B): 7 more correct bits per round, from the bottom
        x = y ^ ((x << 7) & 0x9D2C5680)
    y = x & MASK32
    x = y
    for _ in range(3):  # y = x ^ (x >> 11): 11 more correct bits per round, from the top
        x = y ^ (x >> 11)
    return x & MASK32


def _twist(upper_of, lower_of):
    y = (int(upper_of) & 0x80000000) | (int(lower_of) & 0x7FFFFFFF)
    return (y >> 1) ^ (MAG if y & 1 else 0)


def _untwist(v):
    """y with _twist-of-y == v: the top bit of v is set exactly when y was odd (y >> 1 has none, MAG has one)"""
    return (((v ^ MAG) << 1) | 1) & MASK32 if v & 0x80000000 else (v << 1) & MASK32


def next_generation(words, upto=N):
    """new[0 .. upto) of the generation after `words` (uint32 [624]), as CPython regenerates it in place"""
    old = np.asarray(words, np.uint32).astype(np.uint64)
    new = old.copy()

    def tw(up, lo):
        y = (up & 0x80000000) | (lo & 0x7FFFFFFF)
        return (y >> 1) ^ np.where(y & 1, MAG, 0).astype(np.uint64)

    new[0:227] = old[397:624] ^ tw(old[0:227], old[1:228])
    new[227:454] = new[0:227] ^ tw(old[227:454], old[228:455])
    new[454:623] = new[227:396] ^ tw(old[454:623], old[455:624])
    new[623] = new[396] ^ tw(old[623:624], new[0:1])[0]
    out = old.copy()
    out[:upto] = new[:upto]  # (new[i] depends on old[] and on new[j], j < i, only)
    return out.astype(np.uint32)


def craft(p, outputs, filler_seed, at=0):
    """[625] uint32: a state with index p whose outputs number at .. at + len(outputs) - 1, counted from the state's position, are
    `outputs`; every other word comes from random.Random(filler_seed).  Words of the current generation (p + at + k < 624) are set
    directly; those of the next one (624 <= p + at + k < 1247) through the words of the current generation they are computed from."""
    return craft_many(p, {at: list(outputs)}, filler_seed)


def craft_many(p, runs, filler_seed):
    """craft() for several runs: {stream offset: outputs}.  The result is checked against CPython before it is returned."""
    assert 0 <= p <= N
    words = [int(w) for w in random.Random(filler_seed).getstate()[1][:N]]
    want = {}
    for at, outs in runs.items():
        for k, o in enumerate(outs):
            assert at + k not in want
            want[at + k] = int(o) & MASK32
    fixed = set()  # positions of the current generation that must keep their value
    for t in sorted(want):
        g = p + t
        if g < N:
            words[g] = untemper(want[t])
            fixed.add(g)
    later = sorted(t for t in want if p + t >= N)
    if later:
        new = {}

        def new_word(i):  # word i of the next generation from the current words
            if i not in new:
                far = words[i + M] if i < N - M else new_word(i - (N - M))
                new[i] = far ^ _twist(words[i], words[i + 1] if i < N - 1 else new_word(0))
            return new[i]

        for t in later:
            j = p + t - N
            assert j < N - 1, "word 623 of a generation has one free bit only: place the run elsewhere"
            target = untemper(want[t])
            new.clear()
            if j < N - M:  # new[j] = old[j + 397] ^ twist(old[j], old[j + 1])
                assert j + M not in fixed
                words[j + M] = target ^ _twist(words[j], words[j + 1])
                fixed.add(j + M)
            else:  # new[j] = new[j - 227] ^ twist(old[j], old[j + 1]): the top bit of old[j], the low 31 of old[j + 1]
                assert j not in fixed and j + 1 not in fixed
                y = _untwist(target ^ new_word(j - (N - M)))
                words[j] = (words[j] & 0x7FFFFFFF) | (y & 0x80000000)
                words[j + 1] = (words[j + 1] & 0x80000000) | (y & 0x7FFFFFFF)
    state = np.array(words + [p], np.uint32)
    rng = py_rng(state)
    got = [rng.getrandbits(32) for _ in range(max(want) + 1)] if want else []
    assert all(got[t] == o for t, o in want.items()), "crafted state does not give the prescribed words"
    return state


def to_update_behind(state625):
    """The layout the device keeps, (words[624] uint32, pos): a position holds the current generation's word until that word is
    handed out and the next generation's afterwards — positions below the index are advanced one generation; pos = index % 624."""
    st = np.asarray(state625, np.uint32)
    index = int(st[N])
    assert 0 <= index <= N
    return next_generation(st[:N], upto=index), index % N


def py_rng(state625):
    r = random.Random()
    r.setstate((3, tuple(int(w) for w in np.asarray(state625).reshape(N + 1)), None))
    return r


def state_of(rng):
    return np.array(rng.getstate()[1], np.uint32)


# ---- word patterns ------------------------------------------------------------------------------------------------------------
def rand_bits_of(rand_n):
    return int(rand_n).bit_length()  # _randbelow_with_getrandbits: k = n.bit_length(); getrandbits(k) until it is below n


def accept_word(rand_n, rand_bits, value=0, low=0):
    """a 32-bit output whose top rand_bits bits are `value` < rand_n: getrandbits(rand_bits) accepts it"""
    assert 0 <= value < rand_n and rand_bits == rand_bits_of(rand_n)
    return ((value << (32 - rand_bits)) | (low & ((1 << (32 - rand_bits)) - 1))) & MASK32


def reject_word(rand_n, rand_bits, k=0, low=0):
    """a 32-bit output whose top rand_bits bits are a value >= rand_n (the k-th such value, cyclically).  Every rand_n has one:
    rand_n < 2^rand_bits by the definition of the bit length."""
    assert rand_bits == rand_bits_of(rand_n)
    span = (1 << rand_bits) - rand_n
    assert span > 0
    value = rand_n + k % span
    return ((value << (32 - rand_bits)) | (low & ((1 << (32 - rand_bits)) - 1))) & MASK32


def u_exact(k, bits=53):
    """two outputs (a, b) whose random() = ((a >> 5) * 2^26 + (b >> 6)) / 2^53 is exactly k / 2^53"""
    assert bits == 53 and 0 <= k < (1 << 53)
    return [((k >> 26) << 5) & MASK32, ((k & ((1 << 26) - 1)) << 6) & MASK32]


U_ZERO = u_exact(0)                  # random() == 0.0: expovariate gives -0.0
U_MAX = u_exact((1 << 53) - 1)       # random() == 1 - 2^-53: expovariate gives -log(2^-53) / lambd


# ---- the reference's _next_service, draw by draw ---------------------------------------------------------------------------------
FAMILIES = ("RMSA", "DeepRMSA", "RMCSA", "RWA", "QoSConstrainedRA")


def dst_weights(probs, src):
    """_get_node_pair (optical_network_env.py:166-168), as envs.py builds cum_dst"""
    w = np.copy(np.asarray(probs, np.float64))
    w[src] = 0.0
    return w / np.sum(w)


def draw_services(rng, family, cfg, n):
    """n times _next_service's draws (rmsa_env.py:545-561, rwa_env.py:258-288, rmcsa_env.py:690-739, qos_constrained_ra.py:246-260)
    from `rng`, in the reference's order: inter-arrival time, holding time, source, destination (the source's weight zeroed, the
    rest renormalised), then randint(lo, hi) / choices(bit_rates, probs) / the service class; RWA draws nothing more.
    cfg: probs [N], lambda_a, lambda_h (the arguments of the two expovariate calls), and mode ("continuous": lo, hi;
    "discrete": bit_rates, bit_rate_probs) or class_probs.  Returns a dict of arrays: q, ht (float64), src, dst, br (the bit rate
    or class; 0 for RWA), br_idx (its index), words (stream words consumed by services 0 .. k, cumulative)."""
    assert family in FAMILIES
    probs = np.asarray(cfg["probs"], np.float64)
    nodes = list(range(len(probs)))
    out = dict(q=np.zeros(n), ht=np.zeros(n), src=np.zeros(n, np.int64), dst=np.zeros(n, np.int64), br=np.zeros(n, np.int64),
               br_idx=np.zeros(n, np.int64), words=np.zeros(n, np.int64))
    total = 0
    before = rng.getstate()[1][N]
    for k in range(n):
        out["q"][k] = rng.expovariate(cfg["lambda_a"])
        out["ht"][k] = rng.expovariate(cfg["lambda_h"])
        src = rng.choices(nodes, weights=probs)[0]
        dst = rng.choices(nodes, weights=dst_weights(probs, src))[0]
        out["src"][k], out["dst"][k] = src, dst
        if family == "RWA":
            pass
        elif family == "QoSConstrainedRA":
            c = rng.choices(list(range(len(cfg["class_probs"]))), cfg["class_probs"])[0]
            out["br"][k] = out["br_idx"][k] = c
        elif cfg.get("mode", "continuous") == "continuous":
            br = rng.randint(cfg["lo"], cfg["hi"])
            out["br"][k], out["br_idx"][k] = br, br - cfg["lo"]
        else:
            rates = list(cfg["bit_rates"])
            br = rng.choices(rates, cfg["bit_rate_probs"])[0]
            out["br"][k], out["br_idx"][k] = br, rates.index(br)
        after = rng.getstate()[1][N]
        total += (after - before) % N  # (the index runs 1 .. 624 and starts again at 1; a service takes far fewer than 624 words)
        before = after
        out["words"][k] = total
    return out


def bits(a):
    """float64 array as its bit patterns: comparisons of floats in the crafted-state tests are on these, never on the values
    (-0.0 == 0.0, nan != nan)"""
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def cum_weights(weights):
    """the cumulative table random.choices builds: list(itertools.accumulate(weights))"""
    return np.array(list(itertools.accumulate([float(w) for w in weights])), np.float64)


# ---- whole batches of crafted envs -------------------------------------------------------------------------------------------
INDICES = (0, 1, 227, 397, 623, 624, 226, 228, 396, 398, 560, 300, 63, 64, 65, 622)
KINDS = ("reject_run", "iat_zero", "ht_zero", "iat_max", "ht_max", "both_zero")


def traffic_cfg(family, n_nodes, load=None, mean_service_holding_time=None, mean_service_inter_arrival_time=0.1, probs=None, **kw):
    """draw_services' cfg for the reference constructor's arguments (optical_network_env.py:92-94, deeprmsa_env.py:22-32): the two
    rates as _next_service computes them, 1 / mean_service_inter_arrival_time and 1 / mean_service_holding_time, in Python floats"""
    if family == "DeepRMSA":
        mht = 25.0 if mean_service_holding_time is None else mean_service_holding_time
        load = mht / mean_service_inter_arrival_time
    else:
        mht = 10800.0 if mean_service_holding_time is None else mean_service_holding_time
        load = 10 if load is None else load
    miat = 1 / float(load / float(mht))
    cfg = dict(probs=np.full(n_nodes, 1.0 / n_nodes) if probs is None else np.asarray(probs, np.float64), lambda_a=1 / miat, lambda_h=1 / mht)
    if family == "QoSConstrainedRA":
        cfg["class_probs"] = list(kw.get("classes_arrival_probabilities", [1.0]))
    elif family != "RWA":
        if kw.get("bit_rate_selection", "continuous") == "discrete":
            rates = list(kw.get("bit_rates", [10, 40, 100]))
            cfg.update(mode="discrete", bit_rates=rates, bit_rate_probs=list(kw.get("bit_rate_probabilities") or [1.0 / len(rates)] * len(rates)))
        else:
            cfg.update(mode="continuous", lo=int(kw.get("bit_rate_lower_bound", 25)), hi=int(kw.get("bit_rate_higher_bound", 100)))
    return cfg


def seeks(family, cfg):
    """the family draws its bit rate with randint: a rejection loop"""
    return family in ("RMSA", "DeepRMSA", "RMCSA") and cfg.get("mode") == "continuous"


def crafted_batch(n, family, cfg, run_len=40, seed0=5000, s_max=24):
    """n crafted envs: env i starts at index INDICES[i] (then spread over 0 .. 624) and holds one crafted event in service
    s_i in 1 .. s_max (service 0 is the one the constructor draws): a run of `run_len` rejected randint words before the accepted
    one (families that draw with randint; the others get a time edge), or random() == 0 / 1 - 2^-53 in the inter-arrival or the
    holding time draw.  Returns (states [n][625], info): info[i] = dict(p, s, kind, first, last) — the stream offsets of the
    env's first and last crafted word."""
    states = np.zeros((n, N + 1), np.uint32)
    info = []
    seek = seeks(family, cfg)
    rn = cfg["hi"] + 1 - cfg["lo"] if seek else 0
    rb = rand_bits_of(rn) if seek else 0
    for i in range(n):
        p = INDICES[i] if i < len(INDICES) else (i * 37 + 11) % (N + 1)
        kind = KINDS[(i // s_max + i) % len(KINDS)]  # (every kind at every service number: s_i depends on i % s_max)
        if kind == "reject_run" and not seek:
            kind = "both_zero"
        s = 1 + (i * 7) % s_max
        for attempt in range(8):
            fill = seed0 + 97 * i + 13 * attempt
            state, found = craft(p, [], fill), False
            for _ in range(6):  # crafting words of the next generation changes earlier words: until the service's offset holds
                start = int(draw_services(py_rng(state), family, cfg, s)["words"][s - 1])
                if kind == "reject_run":
                    at, outs = start + 8, [reject_word(rn, rb, k, low=0x155555 * k) for k in range(run_len)] + [accept_word(rn, rb, (i * 5) % rn, low=i)]
                elif kind == "both_zero":
                    at, outs = start, U_ZERO + U_ZERO
                else:
                    at, outs = start + (0 if kind.startswith("iat") else 2), (U_ZERO if kind.endswith("zero") else U_MAX)
                try:
                    state = craft(p, outs, fill, at=at)
                except AssertionError:  # (a placement craft() cannot make: another filler, then another service)
                    break
                if int(draw_services(py_rng(state), family, cfg, s)["words"][s - 1]) == start:
                    found = True
                    break
            if found:
                break
            state = None
            s = 1 + s % s_max
        assert state is not None, "no placement found for env %d" % i
        states[i] = state
        info.append(dict(p=p, s=s, kind=kind, first=at, last=at + len(outs) - 1))
    return states, info


def expected_services(state, family, cfg, n):
    """services() of the first n services of an env started from `state`, as the oracle and the device report them: columns
    arrival time (the running sum current_time + expovariate, from 0.0), holding time, source, destination, bit rate / class"""
    d = draw_services(py_rng(state), family, cfg, n)
    out = np.zeros((n, 5))
    now = 0.0
    for k in range(n):
        now = now + float(d["q"][k])
        out[k] = (now, d["ht"][k], d["src"][k], d["dst"][k], d["br"][k])
    return out, d
