"""A batch seen through its device views (device_array / device_tensor) goes with its last reference, not whenever the cycle
collector next runs.  The batch's page-locked staging buffers are given back with it (hipHostFree), and a hipHostFree that falls
into somebody else's stream capture invalidates the capture: the object device_array hands out must therefore not sit in a
reference cycle that keeps the batch alive past the test, or the agent loop, that made it."""
import gc
import weakref

import numpy as np
import pytest


class _Owner:
    pass


def test_a_device_array_holds_its_owner_without_a_cycle():
    from optical_rl_gym_amd.envs import _DeviceArray

    cai = {"shape": (4, 2), "typestr": "<i4", "data": (4096, False), "version": 2, "strides": None}
    gc.collect()
    gc.disable()
    try:
        owner = _Owner()
        gone = weakref.ref(owner)
        arr = _DeviceArray(cai, 3, owner)
        assert arr.__cuda_array_interface__ is cai and arr._owner is owner and arr.__dlpack_device__() == (10, 3)
        del owner
        assert gone() is not None  # the array keeps its batch alive ...
        del arr
        assert gone() is None  # ... and lets go of it at once, with the collector off
    finally:
        gc.enable()


@pytest.mark.gpu
def test_a_batch_goes_with_its_last_device_view():
    import optical_rl_gym_amd as orl
    import torch

    gc.collect()
    gc.disable()
    try:
        env = orl.make("RMSA", topology="nsfnet_chen", num_envs=64, seeds=list(range(64)), load=100, num_spectrum_resources=64)
        gone = weakref.ref(env)
        env.action_mask(fetch=False)
        acts = env.device_tensor("actions")
        mask = env.device_tensor("action_mask")
        rew = torch.from_dlpack(env.device_array("reward"))
        assert acts.shape == (64, 4) and mask.dtype == torch.bool and rew.shape == (64,)
        env.sync()
        assert np.array_equal(mask.cpu().numpy(), env.action_mask())
        env.close()
        del env
        assert gone() is not None  # (a view keeps the batch object alive)
        del acts, mask, rew
        assert gone() is None
    finally:
        gc.enable()
