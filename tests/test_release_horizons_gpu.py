"""Release horizons on the device (include/orl.h, orl_batch_release_horizons; k_release_horizons in csrc/orl_horizon.h) against the numpy
restatement (tests/horizon_restate.py), bit for bit: from the release-time model's lists (tests/horizon_model.py, pinned to the oracle in
tests/test_release_horizons.py) on the walks that test establishes the kinds on; from the device's own pending() after every way of
stepping; in forced rounds; under graph capture; over a regrown buffer, two shards and the pad columns; and the refusal."""
import numpy as np
import pytest

from tests import horizon_model as hm
from tests import horizon_restate as hr
from tests import slot_agent
from tests.test_release_horizons import SHAPES, check_restatement

pytestmark = pytest.mark.gpu

TOPOLOGY = slot_agent.TOPOLOGY
SC_EV = 19  # word of the scalar record (section 0 of a snapshot, 32 words per env): high-water mark | count << 32 of the release table


def make(name, n=None, **over):
    import optical_rl_gym_amd as orl

    fam, kw, S, n_envs, seeds = hm.walk_config(name)
    kw.update(over)
    n = n_envs if n is None else n
    env = orl.make(fam, topology=TOPOLOGY, num_envs=n, seeds=[hm.SEED0 + e for e in range(n)], **kw)
    return env, fam, (slot_agent.rmcsa_tables(name) if fam == "RMCSA" else None), kw.get("num_spatial_resources", 1), S


def device_pending(env):
    return [env.pending(e) for e in range(env.num_envs)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def compare(env, fam, tab, C, S, pending, what, seen=None):
    """Every layout, j and (RMCSA) modulation of the present state against the restatement from `pending`, on every env, on the bit
    patterns; the shapes as defined"""
    seen = {} if seen is None else seen
    want = check_restatement(fam, tab, hm.avail_of(env, C, S), env.services(), pending, env.topology, seen)
    n, R = env.num_envs, env.k_paths * C
    for (layout, j, mod), rows in want.items():
        width = S if layout == "slots" else 2 * j
        dim = R * width + 1
        assert env.release_horizons_shape(layout, j) == (R, width, dim, (dim + 3) // 4 * 4), (what, layout, j)
        got = env.release_horizons(layout, j, mod)
        assert got.dtype == np.float32 and got.shape == (n, dim), (what, layout, j, mod)
        bad = np.flatnonzero((bits(got) != bits(rows)).any(axis=1))
        if len(bad):
            e = int(bad[0])
            col = int(np.flatnonzero(bits(got[e]) != bits(rows[e]))[0])
            raise AssertionError("%s, %s, j = %d, modulation %r: %d envs differ; env %d column %d (row %d, %d): got %r, want %r"
                                 % (what, layout, j, mod, len(bad), e, col, col // width, col % width, got[e, col], rows[e, col]))
    return want


@pytest.mark.parametrize("name", [n for names in SHAPES.values() for n in names])
def test_both_layouts_equal_the_restatement_from_the_model_on_the_walks(name):
    """The walk of tests/test_release_horizons.py on a device batch, the model beside it: at every checkpoint pending(e) of a sample of
    envs is the model's list as a multiset (== on the float64 times), and both layouts equal the restatement from the model's lists."""
    env, fam, tab, C, S = make(name)
    n = env.num_envs
    model = hm.Model(fam, env.topology, n, tab)
    seen = {"holes": 0}
    assert env.state_layout()[0] == 256

    def checkpoint(tag):
        for e in (0, 7, n - 1):
            t, rec = env.pending(e)
            # (pair, path, first slot, slots, core); one wavelength of RWA counts as one slot on either side
            key = lambda a, r: (float(a), int(r[0]), int(r[1]), int(r[2]), max(int(r[3]), 1), int(r[4]))
            got = sorted(key(a, r) for a, r in zip(t, rec))
            want = sorted(key(a, r) for a, r in zip(model.times(e), model.records(e)))
            assert got == want, (name, tag, e)
        compare(env, fam, tab, C, S, [(model.times(e), model.records(e)) for e in range(n)], "%s, %s" % (name, tag), seen)
        ev = env.get_state()[:n * 256].view(np.uint64).reshape(n, 32)[:, SC_EV]
        seen["holes"] += int(((ev & np.uint64(0xffffffff)) > (ev >> np.uint64(32))).sum())

    acc, ref = hm.walk(name, env, model, checkpoint)
    assert acc > 0 and ref > 0
    env.reset(full=True)
    model.reset_full()
    checkpoint("reset")
    print(name, seen)
    assert seen["holes"] > 0  # a release table with a hole: high-water mark above the count
    assert not (env.flags() & 2).any()
    env.check()
    env.close()


@pytest.mark.parametrize("name", ["rmcsa_c7_s64", "rmsa_nsf_s129"])
def test_forced_rounds_equal_the_plans_own_form(name):
    env, fam, tab, C, S = make(name)
    env.run(hm.HEURISTIC[fam], 300)
    own = compare(env, fam, tab, C, S, device_pending(env), name)
    keys = [k for k in own if k[1] in (1, 3)]
    for rows in (1, 3, 8, 0):
        assert env.lib.orl_debug_set_horizon_rows(env._h, rows) == 0
        for layout, j, mod in keys:
            got = env.release_horizons(layout, j, mod)
            assert np.array_equal(bits(got), bits(own[layout, j, mod])), (name, rows, layout, j, mod)
    assert env.lib.orl_debug_set_horizon_rows(env._h, -1) != 0
    env.check()
    env.close()


@pytest.mark.parametrize("name", ["rmsa_nsf_s65", "rwa_nsf_s129", "rmcsa_c7_s64"])
def test_the_view_follows_every_way_of_stepping(name):
    """After a device-resident run, policy_step, seed, set_state to an earlier snapshot and copy_envs the view equals the restatement
    from pending(), the slot maps and services() of that moment: it reads the release table, not a cache."""
    env, fam, tab, C, S = make(name, load=150) if name == "rwa_nsf_s129" else make(name)
    pol = hm.HEURISTIC[fam]
    here = lambda what: compare(env, fam, tab, C, S, device_pending(env), "%s, %s" % (name, what))
    here("construction")
    env.run(pol, 60)
    early = here("run")
    snap = env.get_state()
    for _ in range(5):
        env.policy_step(pol, auto_reset=True, fetch=False)
    here("policy_step")
    env.run(pol, 40)
    later = here("second run")
    assert not np.array_equal(early["slots", 1, None], later["slots", 1, None])
    env.set_state(snap)
    back = here("set_state")
    assert np.array_equal(bits(back["slots", 1, None]), bits(early["slots", 1, None]))
    env.run(pol, 25)
    env.copy_envs(np.array([0, 0, 3]), np.array([1, 2, 4]))
    forked = here("copy_envs")["slots", 1, None]
    assert np.array_equal(bits(forked[1]), bits(forked[0])) and np.array_equal(bits(forked[4]), bits(forked[3]))
    env.seed(np.arange(900, 900 + env.num_envs))
    here("seed")
    for _ in range(8):
        env.policy_step(pol, auto_reset=True, fetch=False)
    here("seed, stepped")
    env.check()
    env.close()


def test_a_pair_with_fewer_paths_than_k_gets_rows_of_minus_one(tmp_path):
    """star129 (tests/envelope.py): every pair has fewer than k = 5 paths, so rows of -1 in both layouts"""
    import optical_rl_gym_amd as orl
    from tests import envelope

    c = envelope.CASE_BY_NAME["star129_rmsa"]
    S = c.kw["num_spectrum_resources"]
    env = orl.make("RMSA", topology=envelope.topology_npz(c.topo, c.k, tmp_path), num_envs=24, seeds=list(range(24)), **c.kw)
    env.run("SAP_FF", 200)
    want = compare(env, "RMSA", None, 1, S, device_pending(env), "star129_rmsa")
    assert (want["slots", 1, None][:, :-1].reshape(24, c.k, S)[:, -1] == -1.0).all()
    assert (want["blocks", 3, None][:, :-1].reshape(24, c.k, 6)[:, -1] == -1.0).all()
    env.check()
    env.close()


def test_deeprmsa_rows_are_those_of_rmsa_on_the_same_state():
    """A DeepRMSA batch (its own j = 4) against the restatement under RMSA's rule, which is DeepRMSA's"""
    import optical_rl_gym_amd as orl

    case = slot_agent.CASE_BY_NAME["deep_s129_j4"]
    env = orl.make("DeepRMSA", topology=TOPOLOGY, num_envs=24, seeds=list(range(100, 124)), **case.kw)
    env.run("SAP", 150)
    compare(env, "RMSA", None, 1, 129, device_pending(env), "deep_s129_j4")
    env.check()
    env.close()


def test_view_and_step_captured_in_one_graph():
    """{release_horizons(fetch=False); step(None, fetch=False)} captured on the batch's stream after a first call outside the capture and
    replayed 20 times: the buffer after the last replay is the restatement of the state BEFORE that replay's step; no flag is raised."""
    import torch

    env, fam, tab, C, S = make("rmsa_nsf_s65", n=40)
    twin = make("rmsa_nsf_s65", n=40)[0]
    env.run("SAP_FF", 100)
    twin.set_state(env.get_state())
    s = env.torch_stream()
    acts = env.device_tensor("actions")

    def chain(e):
        e.release_horizons("blocks", 3, fetch=False)
        e.release_horizons("slots", fetch=False)
        e.step(None, auto_reset=True, fetch=False)

    first = env.policy("SAP_FF")  # the action every replay steps: accepted at first, refused once its slots are taken
    with torch.cuda.stream(s):
        chain(env)
    torch.cuda.synchronize()
    twin.step(first, auto_reset=True)
    g = torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=s):
        chain(env)
    torch.cuda.synchronize()
    for it in range(20):
        before = (device_pending(twin), hm.avail_of(twin, C, S), twin.services())
        g.replay()
        torch.cuda.synchronize()
        twin.step(first, auto_reset=True)
    assert np.array_equal(acts.cpu().numpy(), first)
    assert np.array_equal(env.get_state(), twin.get_state())
    want = hr.slots_layout(before[0], before[2], env.topology, C, S)
    got = env.device_tensor("release_horizons").cpu().numpy()
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
    assert not (env.flags() & 2).any()
    env.check()
    env.close()
    twin.close()


def test_buffer_regrown_pad_columns_and_two_shards():
    import torch

    from optical_rl_gym_amd._lib import OrlError
    from optical_rl_gym_amd.envs import _RawDeviceArray
    from optical_rl_gym_amd.sharding import MultiDeviceBatch

    env, fam, tab, C, S = make("rmcsa_c2_s129", n=30, load=150)
    with pytest.raises(OrlError, match=r"call release_horizons\(\)"):
        env.device_tensor("release_horizons")
    env.run("SAP_BM_FC_FF", 120)
    pend = device_pending(env)
    # a larger j after a smaller one, then the largest rows of all: the buffer is regrown twice
    small = env.release_horizons("blocks", 1)
    t1 = env.device_tensor("release_horizons")
    big = env.release_horizons("blocks", 8)
    t8 = env.device_tensor("release_horizons")
    assert t1.shape == (30, 10 * 2 + 1) and t8.shape == (30, 10 * 16 + 1) and t8.data_ptr() != t1.data_ptr()
    want = compare(env, fam, tab, C, S, pend, "regrown")
    assert np.array_equal(bits(small), bits(want["blocks", 1, None])) and np.array_equal(bits(big), bits(want["blocks", 8, None]))
    # pad columns 0 and nothing written past B * pitch: the whole buffer filled with junk first, read back through a flat view
    for layout, j in (("slots", 1), ("blocks", 3), ("blocks", 1)):
        rows, width, dim, pitch = env.release_horizons_shape(layout, j)
        env.release_horizons(layout, j, fetch=False)
        view = env.device_tensor("release_horizons")
        assert view.shape == (30, dim) and view.stride() == (pitch, 1)
        cap = 30 * env.release_horizons_shape("slots")[3]  # the buffer holds the largest call so far
        flat = torch.as_tensor(_RawDeviceArray({"shape": (cap,), "typestr": "<f4", "data": (view.data_ptr(), False), "version": 2, "strides": None}),
                               device=view.device)
        with torch.cuda.stream(env.torch_stream()):
            flat.fill_(-7.0)
            env.release_horizons(layout, j, fetch=False)
        env.sync()
        whole = flat.cpu().numpy()
        body = whole[:30 * pitch].reshape(30, pitch)
        assert np.array_equal(bits(body[:, :dim]), bits(want[layout, j, None])), (layout, j)
        assert (body[:, dim:] == 0).all() and (whole[30 * pitch:] == -7.0).all(), (layout, j)
    env.close()
    # two shards on one device against the unsharded batch
    n, cut = 40, 13
    whole = make("rmsa_nsf_s65", n=n)[0]
    seeds = [hm.SEED0 + e for e in range(n)]
    fam, kw, S, _, _ = hm.walk_config("rmsa_nsf_s65")
    import optical_rl_gym_amd as orl

    mk = lambda sd: orl.make(fam, topology=TOPOLOGY, num_envs=len(sd), seeds=sd, **kw)
    multi = MultiDeviceBatch.from_shards([mk(seeds[:cut]), mk(seeds[cut:])])
    for _ in range(80):
        a = whole.policy("SAP_FF")
        whole.step(a, auto_reset=True)
        multi.step(a, auto_reset=True)
    for layout, j in (("slots", 1), ("blocks", 4)):
        assert multi.release_horizons_shape(layout, j) == whole.release_horizons_shape(layout, j)
        a, b = whole.release_horizons(layout, j), multi.release_horizons(layout, j)
        assert (a[:, :-1] > 0).any() and np.array_equal(bits(a), bits(b)), (layout, j)
        assert multi.release_horizons(layout, j, fetch=False) is None
    multi.close()
    whole.close()


def test_refusals_leave_the_batch_as_it_was():
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd._lib import OrlError

    qos = orl.make("QoSConstrainedRA", topology=TOPOLOGY, num_envs=16, seeds=list(range(16)), load=10)
    snap, flags = qos.get_state(), qos.flags().copy()
    for call in (lambda: qos.release_horizons(), lambda: qos.release_horizons("blocks", 2, fetch=False), lambda: qos.release_horizons_shape("blocks", 1)):
        with pytest.raises(OrlError, match="QoSConstrainedRA"):
            call()
    with pytest.raises(OrlError, match=r"call release_horizons\(\)"):
        qos.device_tensor("release_horizons")
    assert np.array_equal(qos.get_state(), snap) and np.array_equal(qos.flags(), flags)
    qos.close()
    env, fam, tab, C, S = make("rmcsa_c7_s64")
    env.run("SAP_BM_FC_FF", 30)
    snap = env.get_state()
    M = len(env.modulation_formats)
    for args in ((2, 1, -1), (-1, 1, -1), (1, 0, -1), (1, 9, -1), (0, 2, -1), (0, 1, 0), (1, 1, M), (1, 1, -2)):
        assert env.lib.orl_batch_release_horizons(env._h, *args, None) != 0, args  # (ORL_E_INVALID, past the Python-side checks)
    with pytest.raises(OrlError):
        env.release_horizons("blocks", 1, modulation=M)
    with pytest.raises(OrlError, match=r"call release_horizons\(\)"):  # nothing was queued, no buffer exists
        env.device_tensor("release_horizons")
    assert np.array_equal(env.get_state(), snap)
    env.close()
    flat, _, _, _, _ = make("rmsa_nsf_s65")
    with pytest.raises(OrlError, match="RMCSA only"):
        flat.release_horizons("blocks", 1, modulation=0)
    flat.close()
    one = orl.RMCSAEnv(topology=TOPOLOGY, seed=3, load=100, num_spectrum_resources=64, num_spatial_resources=7)
    one.reset()
    H, ht = one.release_horizons()
    Bk, ht2 = one.release_horizons("blocks", 2)
    assert H.shape == (35, 64) and H.dtype == np.float32 and Bk.shape == (35, 2, 2) and ht == ht2 == float(np.float32(one.batch.services()[0, 1]))
    assert (H == 0).all() or (H >= 0).all()
    one.close()
