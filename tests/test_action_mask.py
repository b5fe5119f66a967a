"""Action masks (include/orl.h, orl_batch_action_mask) without a GPU: the ABI surface, the kernels in the code object, the numpy
restatement the GPU tests compare with (checked against the oracle's own step), and the sb3-contrib form OpticalVecEnv and the
single-env facades hand out, over the CPU oracle."""
import os
import re
import shutil
import sys

import numpy as np
import pytest

from optical_rl_gym_amd import _lib
from optical_rl_gym_amd.vec_env import OpticalVecEnv
from tests.mask_restate import restate, restate_fast, row_words, unpack_slots
from tests.oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RMSA_KW = dict(load=300, mean_service_holding_time=25, episode_length=25, num_spectrum_resources=64)
DEEP_KW = dict(load=300, mean_service_holding_time=25, episode_length=25, num_spectrum_resources=64, j=3)
RWA_KW = dict(load=60, mean_service_holding_time=25, episode_length=25, num_spectrum_resources=16)


class MaskedOracle(OracleBackend):
    """The oracle stand-in with an `action_mask` of its own: the numpy restatement on its read-back state."""

    def __init__(self, env_type, topology, seeds, **kw):
        super().__init__(env_type, topology, seeds, **kw)
        self._cw = kw.get("channel_width", 50.0 if env_type == "RWA" else 12.5)

    def action_mask(self, layout="joint", fetch=True):
        avail = np.stack([self.slots(i)[0] for i in range(self.n)]).astype(bool)
        return restate(self.ENV_TYPE, avail, self.services(), self.topology, self.k, self.S, self.j, self._cw,
                       self.allow_rejection, layout)


def _random_steps(batch, n_steps, seed=0):
    rng = np.random.default_rng(seed)
    for _ in range(n_steps):
        if batch.ENV_TYPE == 1:
            a = rng.integers(0, batch.k * batch.j + 1, size=batch.n)
        else:
            # mostly first fit, some random (path, slot) pairs: states with occupied spectrum and some rejects
            a = batch.policy("SAP_FF")[:, :2].copy()
            pick = rng.random(batch.n) < 0.3
            a[pick, 0] = rng.integers(0, batch.k, size=pick.sum())
            a[pick, 1] = rng.integers(0, batch.S, size=pick.sum())
        batch.step(a, auto_reset=True)


def test_header_and_binding_declare_the_mask_api():
    h = open(os.path.join(ROOT, "include", "orl.h")).read()
    assert re.search(r"int orl_batch_action_mask_shape\(const orl_batch\* b, int layout, int32_t\* dim, int32_t\* pitch\);", h)
    assert re.search(r"int orl_batch_action_mask\(orl_batch\* b, int layout, uint8_t\* out\);", h)
    assert re.search(r"#define ORL_BUF_ACTION_MASK 7\b", h)
    assert re.search(r"#define ORL_MASK_JOINT 0\b", h) and re.search(r"#define ORL_MASK_PATH 1\b", h)
    assert re.search(r"#define ORL_ABI_VERSION 2\b", h)
    assert "orl_batch_action_mask" in _lib.EXPORTS and "orl_batch_action_mask_shape" in _lib.EXPORTS
    assert len(_lib.EXPORTS["orl_batch_action_mask"][1]) == 3 and len(_lib.EXPORTS["orl_batch_action_mask_shape"][1]) == 4


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_mask_kernels_exist_for_every_row_width_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs

    from optical_rl_gym_amd import _build

    lib = _build.build()
    found = {}
    for k in kernel_regs.kernels(lib):
        full = kernel_regs.demangle(k["name"])
        m = re.match(r"(?:void )?k_action_mask<(\d+)>", full)
        if m:
            found[int(m.group(1))] = k
    assert sorted(found) == list(_build.ROW_WIDTHS)
    for w, k in found.items():
        assert int(k["vgpr_spill_count"]) == 0 and int(k["private_segment_fixed_size"]) == 0, (w, k)


@pytest.mark.parametrize("fam,kw", [("RMSA", RMSA_KW), ("DeepRMSA", DEEP_KW), ("RWA", RWA_KW)])
def test_restatement_fast_form_equals_the_reference_loop(fam, kw):
    b = MaskedOracle(fam, "nsfnet_chen", list(range(20, 52)), **kw)
    _random_steps(b, 30)
    avail = unpack_slots(b.slots_packed(), b.E, b.S, row_words(b.S))
    assert np.array_equal(avail, np.stack([b.slots(i)[0] for i in range(b.n)]).astype(bool))
    layouts = ("joint",) if fam == "DeepRMSA" else ("joint", "path")
    for lay in layouts:
        slow = restate(b.ENV_TYPE, avail, b.services(), b.topology, b.k, b.S, b.j, b._cw, b.allow_rejection, lay)
        fast = restate_fast(b.ENV_TYPE, avail, b.services(), b.topology, b.k, b.S, b.j, b._cw, b.allow_rejection, lay)
        assert np.array_equal(slow, fast), lay
        if lay == "joint":
            assert slow[:, :-1].sum() < slow[:, :-1].size  # (the states have occupied spectrum)


@pytest.mark.parametrize("fam,kw", [("RMSA", RMSA_KW), ("DeepRMSA", DEEP_KW), ("RWA", RWA_KW)])
def test_restatement_predicts_the_oracle_step(fam, kw):
    """A column of the restated joint mask is 1 exactly when stepping it provisions the service (the oracle is the reference's
    step() in C): every mask-1 column and a sample of the others, one env state per column."""
    seeds = list(range(60, 64))
    probe = MaskedOracle(fam, "nsfnet_chen", seeds, **kw)
    _random_steps(probe, 12, seed=1)
    mask = probe.action_mask()
    dim = mask.shape[1]
    rng = np.random.default_rng(2)
    for i in range(len(seeds)):
        if mask[i, :-1].all():
            continue  # a fallback row: nothing provisions
        cols = list(np.flatnonzero(mask[i, :-1])[:12]) + list(rng.choice(np.flatnonzero(~mask[i, :-1]), 12))
        for c in cols:
            b = MaskedOracle(fam, "nsfnet_chen", seeds, **kw)
            _random_steps(b, 12, seed=1)
            before = b.counters()[i, 1]  # services_accepted
            if fam == "DeepRMSA":
                a = np.full((len(seeds), 1), dim - 1)
                a[i, 0] = c
            else:
                S = b.S
                a = np.tile([b.k, S], (len(seeds), 1)) if fam == "RMSA" or b.allow_rejection else np.zeros((len(seeds), 2), int)
                a[i] = (c // S, c % S)
                if c // S >= b.topology.n_paths[int(b.services()[i, 2]), int(b.services()[i, 3])]:
                    continue  # (IndexError in the reference: the mask says 0)
            b.step(a)
            assert b.counters()[i, 1] - before == int(mask[i, c]), (fam, i, c)


def _factored(joint, k, S, rej):
    body = joint[:, : k * S].reshape(len(joint), k, S)
    parts = [body.any(2)] + ([joint[:, -1:]] if rej else []) + [body.any(1)] + ([joint[:, -1:]] if rej else [])
    return np.concatenate(parts, axis=1)


@pytest.mark.parametrize("fam,kw", [("RMSA", RMSA_KW), ("RMSA", dict(RMSA_KW, allow_rejection=True)), ("DeepRMSA", DEEP_KW),
                                    ("RWA", RWA_KW)])
def test_vecenv_action_masks_in_the_sb3_contrib_form(fam, kw):
    batch = MaskedOracle(fam, "nsfnet_chen", list(range(30, 38)), **kw)
    venv = OpticalVecEnv(batch)
    venv.reset()
    _random_steps(batch, 20)
    joint = batch.action_mask()
    masks = np.stack(venv.env_method("action_masks"))
    if fam == "DeepRMSA":
        n = venv.action_space.n
        assert masks.shape == (8, n) and np.array_equal(masks, joint[:, :n])
    else:
        nvec = np.asarray(venv.action_space.nvec)
        assert masks.shape == (8, int(nvec.sum()))
        rej = 1 if batch.allow_rejection else 0
        want = _factored(joint, batch.k, batch.S, rej)
        assert np.array_equal(masks, want)
        if not rej:  # fallback rows are all ones
            assert masks[joint[:, :-1].all(1)].all()
    assert masks.dtype == np.bool_
    sub = venv.env_method("action_masks", indices=[5, 1])
    assert len(sub) == 2 and np.array_equal(sub[0], masks[5]) and np.array_equal(sub[1], masks[1])
    assert np.array_equal(venv.env_method("action_masks", indices=3)[0], masks[3])
    got = venv.get_attr("action_masks")
    assert len(got) == 8 and np.array_equal(got[2](), masks[2])
    assert np.array_equal(venv.action_masks(), masks)


def test_single_env_facades_hand_out_masks():
    import optical_rl_gym_amd as orl

    kw = dict(RMSA_KW)
    env = orl.RMSAEnv(topology="nsfnet_chen", seed=7, _backend=MaskedOracle("RMSA", "nsfnet_chen", [7], **kw), **kw)
    env.reset()
    for _ in range(10):
        env.step(env.policy_action("SAP_FF"))
    joint = env.batch.action_mask()
    m = env.action_masks()
    assert m.shape == (env.k_paths + env.num_spectrum_resources,) and np.array_equal(m, _factored(joint, 5, 64, 0)[0])
    w = orl.PathOnlyFirstFitAction(env)
    pm = w.action_masks()
    assert pm.shape == (w.action_space.n,) and np.array_equal(pm, env.batch.action_mask("path")[0][:5])
