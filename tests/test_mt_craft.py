"""tests/mt_craft.py against CPython's random module, and the CPU oracle against CPython on crafted generator states: any index
0 .. 624 at construction, runs of 40 rejected randint words, random() == 0 and 1 - 2^-53 (expovariate == -0.0: compared as bit
patterns), randint ranges of 1, 64, 65 and 76 values.  No GPU; the harness of tests/test_rng_prims.py is cross-compiled here."""
import os
import random
import shutil

import numpy as np
import pytest

from tests import mt_craft as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_SET = (0, 1, 226, 227, 396, 397, 560, 623, 624)


def test_untemper_inverts_temper():
    r = random.Random(1)
    for x in [0, 0xFFFFFFFF, 1, 0x80000000] + [r.getrandbits(32) for _ in range(10000)]:
        assert mc.untemper(mc.temper(x)) == x and mc.temper(mc.untemper(x)) == x


def test_temper_is_cpythons():
    st = random.Random(7).getstate()[1]
    r = random.Random(7)
    # (index 624: the first draw regenerates; the generation after the seeding one through next_generation)
    new = mc.next_generation(np.array(st[:624], np.uint32))
    assert [r.getrandbits(32) for _ in range(624)] == [mc.temper(w) for w in new]


@pytest.mark.parametrize("p", P_SET)
def test_craft_gives_cpython_the_prescribed_words(p):
    r = random.Random(100 + p)
    # in the current generation, up to its last word
    for length in sorted({0, min(1, 624 - p), min(7, 624 - p), min(97, 624 - p), 624 - p}):
        outs = [r.getrandbits(32) for _ in range(length)]
        state = mc.craft(p, outs, filler_seed=p)
        assert int(state[624]) == p
        g = mc.py_rng(state)
        assert [g.getrandbits(32) for _ in range(length)] == outs
        fill = random.Random(p).getstate()[1]
        assert all(int(state[i]) == fill[i] for i in range(624) if not (p <= i < p + length))
    # later in the stream, across the end of the generation and wholly inside the next one
    for at in (3, 624 - p - 5, 624 - p, 700 - p, 1000 - p):
        if at < 0 or p + at + 60 >= 1247:
            continue
        outs = [r.getrandbits(32) for _ in range(60)]
        g = mc.py_rng(mc.craft(p, outs, filler_seed=p + 1, at=at))
        assert [g.getrandbits(32) for _ in range(at + 60)][at:] == outs


def test_word_patterns():
    for rn in (1, 2, 3, 51, 64, 65, 76, 127, 128, 129, 4096):
        rb = mc.rand_bits_of(rn)
        for k in range(5):
            a, rj = mc.accept_word(rn, rb, k % rn, low=12345 * k), mc.reject_word(rn, rb, k, low=999 * k)
            assert (a >> (32 - rb)) == k % rn and (rj >> (32 - rb)) >= rn and a < 2**32 and rj < 2**32
        g = mc.py_rng(mc.craft(5, [mc.reject_word(rn, rb, k) for k in range(9)] + [mc.accept_word(rn, rb, rn - 1)], 1))
        assert g.randint(10, 10 + rn - 1) == 10 + rn - 1 and g.getstate()[1][624] == 15
    for k in (0, 1, 2**26, 2**53 - 1, 2**52, 12345678901234):
        g = mc.py_rng(mc.craft(0, mc.u_exact(k), 2))
        assert g.random() == k / 2.0**53
    g = mc.py_rng(mc.craft(9, mc.U_ZERO + mc.U_MAX, 3))
    assert mc.bits([g.expovariate(3.0)])[0] == 1 << 63  # -0.0
    assert g.getstate()[1][624] == 11 and abs(g.expovariate(1.0) - 53 * np.log(2.0)) < 1e-12  # -log(2^-53)


def _update_behind_words(words, pos, n):
    """n outputs from the update-behind form: hand out the word at pos, then replace it by its next generation"""
    mt, out = [int(w) for w in words], []
    for _ in range(n):
        i, i1, im = pos, (pos + 1) % 624, (pos + 397) % 624
        out.append(mc.temper(mt[i]))
        y = (mt[i] & 0x80000000) | (mt[i1] & 0x7FFFFFFF)
        mt[i] = mt[im] ^ (y >> 1) ^ (mc.MAG if y & 1 else 0)
        pos = i1
    return out, mt, pos


@pytest.mark.parametrize("n", [0, 1, 623, 624, 625, 1300])
def test_to_update_behind_continues_cpythons_stream(n):
    r = random.Random(33)
    for _ in range(n):
        r.getrandbits(32)
    words, pos = mc.to_update_behind(mc.state_of(r))
    got, mt, pos2 = _update_behind_words(words, pos, 1500)
    assert got == [r.getrandbits(32) for _ in range(1500)]
    # and the form is closed under drawing: what the generator holds after 1500 draws is the conversion of CPython's state
    words2, pos3 = mc.to_update_behind(mc.state_of(r))
    assert pos2 == pos3 and mt == [int(w) for w in words2]


def test_to_update_behind_from_crafted_indices():
    for p in P_SET:
        state = mc.craft(p, [], 50 + p)
        words, pos = mc.to_update_behind(state)
        assert pos == p % 624
        g = mc.py_rng(state)
        assert _update_behind_words(words, pos, 700)[0] == [g.getrandbits(32) for _ in range(700)]


# ---- the oracle against CPython ------------------------------------------------------------------------------------------------
QOS_KW = dict(num_service_classes=3, classes_arrival_probabilities=[0.2, 0.5, 0.3], classes_reward=[10.0, 2.0, 1.0])
ORACLE_CASES = {
    "rmsa_76": ("RMSA", dict(), "SAP_FF"),
    "rmsa_64": ("RMSA", dict(bit_rate_lower_bound=25, bit_rate_higher_bound=88), "SAP_FF"),
    "rmsa_65": ("RMSA", dict(bit_rate_lower_bound=25, bit_rate_higher_bound=89), "SAP_FF"),
    "rmsa_1": ("RMSA", dict(bit_rate_lower_bound=40, bit_rate_higher_bound=40), "SAP_FF"),
    "rmsa_discrete": ("RMSA", dict(bit_rate_selection="discrete"), "SAP_FF"),
    "deeprmsa": ("DeepRMSA", dict(j=2), "SAP"),
    "rmcsa": ("RMCSA", dict(), "SAP_BM_FC_FF"),
    "rwa": ("RWA", dict(), "SAP_FF"),
    "qos": ("QoSConstrainedRA", QOS_KW, "SAP_FF"),
}


def check_services(tag, t, got, exp, n_cols=5):
    """services() rows against expected ones: floats as bit patterns"""
    gb, eb = mc.bits(np.asarray(got)[:, :n_cols]), mc.bits(np.asarray(exp)[:, :n_cols])
    bad = np.flatnonzero((gb != eb).any(axis=1))
    assert len(bad) == 0, "%s: service %d: %d envs differ, first env %d:\n got %r\n exp %r" % (tag, t, len(bad), bad[0], got[bad[0]], exp[bad[0]])


@pytest.mark.parametrize("name", sorted(ORACLE_CASES))
def test_oracle_equals_cpython_on_crafted_states(name):
    from oracle.oracle import OracleBatch

    fam, kw, policy = ORACLE_CASES[name]
    cfg = mc.traffic_cfg(fam, 14, **kw)
    n, T = 24, 40
    states, info = mc.crafted_batch(n, fam, cfg)
    assert {0, 1, 227, 397, 623, 624} <= {d["p"] for d in info}
    exp = [mc.expected_services(states[i], fam, cfg, T) for i in range(n)]
    kinds = {d["kind"] for d in info}
    assert ("reject_run" in kinds) == mc.seeks(fam, cfg) and {"iat_zero", "ht_zero", "iat_max", "ht_max", "both_zero"} <= kinds
    for i, d in enumerate(info):  # the crafted words are consumed inside the services compared, by the service they were placed in
        w = exp[i][1]["words"]
        assert (w[d["s"] - 1] if d["s"] else 0) <= d["first"] and d["last"] < w[d["s"]] and d["s"] < T, (i, d)
        if d["kind"] == "reject_run":
            assert w[d["s"]] - w[d["s"] - 1] == 8 + 40 + 1
        if d["kind"] in ("ht_zero", "both_zero"):
            assert mc.bits([exp[i][0][d["s"], 1]])[0] == 1 << 63  # the holding time is -0.0
    ora = OracleBatch(fam, "nsfnet_chen", mt_state=states, **kw)
    for t in range(T):
        check_services(name, t, ora.services(), np.array([e[0][t] for e in exp]))
        ora.step(ora.policy(policy))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_harness_cross_compiles_for_gfx950():
    from tests import test_rng_prims as trp

    for tuned in (False, True):
        path = trp.harness_path(tuned)
        assert os.path.exists(path) and os.path.getsize(path) > 0
        rel = os.path.relpath(path, ROOT)
        assert rel.startswith(os.path.join("optical_rl_gym_amd", "build")), rel
        with open(path, "rb") as f:
            blob = f.read()
        for sym in ("rg_log", "rg_words", "rg_draw", "rg_svc", "k_words64", "k_words8", "k_draw64", "k_draw8", "k_svc"):
            assert sym.encode() in blob
