"""Batched optical-network environments on MI355X: host-side mirror of the reference's env classes.

Each class takes the reference constructor's kwargs (same names, same defaults, same derivations) plus
`num_envs`, `seeds` and `device_id`, flattens them into the tables of include/orl.h and drives the HIP
library through ctypes.  Env i of a batch behaves exactly like a reference env built with seed=seeds[i].

reference constructors: optical_network_env.py:14-94, rmsa_env.py:29-161, deeprmsa_env.py:10-46,
rwa_env.py:19-94, rmcsa_env.py:29-207.
"""
import ctypes as C
import itertools
import math
import os
import random

import numpy as np

from . import _build, _lib
from .topology import Topology

POLICIES = {"SP_FF": 0, "SAP_FF": 1, "KSP_FF": 1, "LLP_FF": 2, "SAP_LF": 3, "SP": 0, "SAP": 1, "SAP_BM_FC_FF": 1,
            "PATH_FF": 4}

RMSA_INFO_KEYS = ["service_blocking_rate", "episode_service_blocking_rate", "bit_rate_blocking_rate",
                  "episode_bit_rate_blocking_rate", "network_compactness", "network_compactness_difference",
                  "avg_link_compactness", "avg_link_utilization"]
COUNTER_NAMES = ["services_processed", "services_accepted", "episode_services_processed",
                 "episode_services_accepted", "bit_rate_requested", "bit_rate_provisioned",
                 "episode_bit_rate_requested", "episode_bit_rate_provisioned"]


def mt_states(seeds):
    """optical_network_env.py:205-210: rng = random.Random(seed or 41) -> [n][625] uint32 MT19937 state."""
    out = np.empty((len(seeds), 625), np.uint32)
    for i, s in enumerate(seeds):
        out[i] = random.Random(41 if s is None else int(s)).getstate()[1]
    return out


def _ptr(a):
    return None if a is None else a.ctypes.data


def per_env_values(value, num_envs, name):
    """A per-env argument (load, mean_service_holding_time, ...): None for a scalar — one value for the whole batch — else
    the values as a float64 array of length num_envs.  ValueError for any other shape and for values that are not positive
    and finite."""
    if value is None or np.isscalar(value) or (isinstance(value, np.ndarray) and value.ndim == 0):
        return None
    a = np.array(value, dtype=np.float64)
    if a.ndim != 1 or a.shape[0] != int(num_envs):
        raise ValueError("%s must be a scalar or one value per env (length %d), got shape %r" % (name, num_envs, a.shape))
    if not (np.isfinite(a).all() and (a > 0).all()):
        raise ValueError("%s must be positive and finite for every env" % name)
    return a


def _check_scalar(value, name):
    v = float(value)
    if not (math.isfinite(v) and v > 0):
        raise ValueError("%s must be positive and finite" % name)
    return value


def derive_rates(load, mean_service_holding_time):
    """set_load (optical_network_env.py:92-94) and the two rates _next_service divides by (rmsa_env.py:548-553), per env, in
    Python floats with the reference's own expressions: (mean_service_inter_arrival_time, lambda_arrival, lambda_holding) as
    float64 arrays for the arrays `load` and `mean_service_holding_time`."""
    n = len(load)
    miat, lam_a, lam_h = np.empty(n, np.float64), np.empty(n, np.float64), np.empty(n, np.float64)
    for i in range(n):
        ld, mht = float(load[i]), float(mean_service_holding_time[i])
        miat[i] = 1 / float(ld / float(mht))
        lam_a[i] = 1 / miat[i]
        lam_h[i] = 1 / mht
    return miat, lam_a, lam_h



def refuse_endless_episodes(steps_per_episode, episode_length):
    """evaluate() plays until `done`: ValueError where an episode of the configuration can never end.  The soft reset in front of
    every episode of the harness (utils.py:103-141) counts the pending service (rmsa_env.py:314, rmcsa_env.py:414), and `done` is
    episode_services_processed == episode_length after the next one was counted: with episode_length=1 the counter stands at 1
    when the episode starts and never equals it again — the reference harness would loop forever."""
    if steps_per_episode < 1:
        raise ValueError("evaluate: with episode_length=%r an episode of this env family never returns done (the soft reset that "
                         "starts an episode already counts the pending service), so no number of steps finishes one; use "
                         "episode_length >= %d" % (episode_length, episode_length - steps_per_episode + 1))


class _PinnedBlock:
    """Owner of one page-locked host allocation (orl_host_alloc); numpy views keep it alive through their base chain."""

    def __init__(self, lib, ptr):
        self.lib, self.ptr = lib, ptr

    def __del__(self):
        try:
            self.lib.orl_host_free(self.ptr)
        except Exception:
            pass


class _RawDeviceArray:  # what torch.as_tensor consumes
    def __init__(self, cai):
        self.__cuda_array_interface__ = cai


class _DeviceArray:
    """Device-resident array of a batch: `__cuda_array_interface__` (torch.as_tensor, CuPy) and DLPack (`torch.from_dlpack`,
    `cupy.from_dlpack`, jax): no copy either way; the batch owns the memory.  A plain object without a reference cycle: it, and the
    batch it keeps alive, go when the last reference does, not whenever the cycle collector next runs — a batch's page-locked
    buffers are given back with it (hipHostFree), which must not fall into somebody's stream capture."""

    def __init__(self, cai, device_id, owner):
        self.__cuda_array_interface__ = cai
        self._device_id = device_id
        self._owner = owner  # keeps the batch alive

    def __dlpack_device__(self):
        return (10, self._device_id)  # kDLROCM

    def __dlpack__(self, stream=None, **kw):
        import torch

        t = torch.as_tensor(_RawDeviceArray(self.__cuda_array_interface__), device="cuda:%d" % self._device_id)
        t._orl_owner = self._owner
        return t.__dlpack__() if stream is None else t.__dlpack__(stream=stream)


class BatchedOpticalEnv:
    """Common machinery; use one of the four family classes below."""

    ENV_TYPE = None
    N_ACTION = 2

    # ---- construction --------------------------------------------------------------------------
    def _setup(self, topology, num_envs, seeds, device_id, *, episode_length, load, mean_service_holding_time,
               num_spectrum_resources, allow_rejection, node_request_probabilities, channel_width,
               bit_rate_selection="continuous", bit_rates=(10, 40, 100), bit_rate_probabilities=None,
               bit_rate_lower_bound=25, bit_rate_higher_bound=100, j=1, num_spatial_resources=1,
               modulations=None, worst_xt=None, event_capacity=0, action_histograms=False, num_service_classes=1,
               classes_arrival_probabilities=(1.0,), classes_reward=(1.0,), mt_state=None):
        self.lib = _lib.lib()  # ORL_LIB_VARIANT=alt selects the -DORL_ALT_IMPLS build (cross-implementation tests)
        self.action_histograms = bool(action_histograms)
        self.topology = Topology.load(topology) if isinstance(topology, str) else topology
        t = self.topology
        self.num_envs = int(num_envs)
        if mt_state is not None:
            # the generators' states themselves instead of seeds: [num_envs][625] uint32, random.Random.getstate()[1] of every env
            # (624 MT19937 words + the index 0 .. 624, include/orl.h orl_batch_create)
            if seeds is not None:
                raise ValueError("seeds or mt_state, not both")
            mt_state = np.ascontiguousarray(mt_state, np.uint32)
            if mt_state.shape != (self.num_envs, 625) or (mt_state[:, 624] > 624).any():
                raise ValueError("mt_state must be [num_envs][625] uint32: 624 words and an index of at most 624 per env")
        self._mt_state = mt_state
        if seeds is None:
            seeds = [None] * self.num_envs
        elif np.isscalar(seeds):
            seeds = [int(seeds) + i for i in range(self.num_envs)]
        assert len(seeds) == self.num_envs
        self.seeds = list(seeds)
        self.device_id = device_id
        self.episode_length = episode_length
        self.allow_rejection = bool(allow_rejection)
        self.reject_action = 1 if allow_rejection else 0
        self.num_spectrum_resources = num_spectrum_resources
        self.num_spatial_resources = num_spatial_resources
        self.k_paths = t.k_paths
        self.channel_width = channel_width
        self.j = j
        # set_load (optical_network_env.py:76-94)
        load_v = per_env_values(load, self.num_envs, "load")
        mht_v = per_env_values(mean_service_holding_time, self.num_envs, "mean_service_holding_time")
        if load_v is None and mht_v is None:
            self.load = load
            self.mean_service_holding_time = mean_service_holding_time
            self.mean_service_inter_arrival_time = 1 / float(load / float(mean_service_holding_time))
            lambda_a = 1 / self.mean_service_inter_arrival_time  # rmsa_env.py:548-550
            lambda_h = 1 / self.mean_service_holding_time        # rmsa_env.py:553
            self._rate_arrays = (None, None)
        else:
            # one pair per env: env i as a reference env constructed with load[i], mean_service_holding_time[i]
            if load_v is None:
                load_v = np.full(self.num_envs, float(_check_scalar(load, "load")), np.float64)
            if mht_v is None:
                mht_v = np.full(self.num_envs, float(_check_scalar(mean_service_holding_time, "mean_service_holding_time")), np.float64)
            self.load, self.mean_service_holding_time = load_v, mht_v
            self.mean_service_inter_arrival_time, lam_a, lam_h = derive_rates(load_v, mht_v)
            self._rate_arrays = (lam_a, lam_h)
            # the configuration's scalar pair is that of the env with the largest load: what sizes the pending-release arrays
            # (event_capacity=0), and with them the specialisation flags, for the whole batch
            top = int(np.argmax(lam_a / lam_h))
            lambda_a, lambda_h = float(lam_a[top]), float(lam_h[top])
        # node pair tables (optical_network_env.py:68-74, 156-173)
        N = t.n_nodes
        if node_request_probabilities is None:
            probs = np.full(N, fill_value=1.0 / N)
        else:
            probs = np.asarray(node_request_probabilities, dtype=np.float64)
            assert len(probs) == N
        self.node_request_probabilities = probs
        cum_src = np.array(list(itertools.accumulate(probs)), np.float64)
        cum_dst = np.zeros((N, N), np.float64)
        for s in range(N):
            w = np.copy(probs)
            w[s] = 0.0
            w = w / np.sum(w)
            cum_dst[s] = list(itertools.accumulate(w))
        # bit rates (rmsa_env.py:78-99)
        self.bit_rate_selection = bit_rate_selection
        mods = list(t.modulations if modulations is None else modulations)
        self.modulation_formats = mods
        M = len(mods)
        if self.ENV_TYPE in (2, 4):
            table_rates, cum_br, mode = [0], None, 0
            lo = hi = 0
        elif bit_rate_selection == "continuous":
            lo, hi = int(bit_rate_lower_bound), int(bit_rate_higher_bound)
            assert lo == bit_rate_lower_bound and hi == bit_rate_higher_bound
            table_rates, cum_br, mode = list(range(lo, hi + 1)), None, 0
        else:
            assert bit_rate_selection == "discrete"
            if bit_rate_probabilities is None:
                bit_rate_probabilities = [1.0 / len(bit_rates) for _ in range(len(bit_rates))]
            assert len(bit_rates) == len(bit_rate_probabilities)
            self.bit_rates = list(bit_rates)
            self.bit_rate_probabilities = list(bit_rate_probabilities)
            table_rates = [int(b) for b in bit_rates]
            cum_br = np.array(list(itertools.accumulate(bit_rate_probabilities)), np.float64)
            mode, lo, hi = 1, 0, 0
        # get_number_slots (rmsa_env.py:610-621): ceil(bit_rate / (se * channel_width)) + 1
        n_slots = np.zeros((len(table_rates), M), np.uint8)
        if self.ENV_TYPE not in (2, 4):
            for i, br in enumerate(table_rates):
                for m, mod in enumerate(mods):
                    n_slots[i, m] = math.ceil(br / (mod.spectral_efficiency * channel_width)) + 1
        # RMCSA reach tables (_crosstalk_is_acceptable, rmcsa_env.py:341-384), evaluated with the reference's
        # own float expressions for every (modulation, bit rate)
        lmax_snr = lmax_xt = None
        if self.ENV_TYPE == 3:
            self.worst_xt = worst_xt
            lmax_snr = np.zeros((M, len(table_rates)), np.float64)
            lmax_xt = np.zeros(M, np.float64)
            average_power = 1
            nf_db = 5.5
            nf = 10.0 ** (nf_db / 10.0)
            amp_spam = 100
            amp_gain_db = 20
            amp_gain = 10.0 ** (amp_gain_db / 10.0)
            lambda_ = 1550
            h = 6.626068e-34
            f_hz = 2.99e8 / (lambda_ * 1e-9)
            for m, mod in enumerate(mods):
                SNR_min_calc = 10 ** ((mod.minimum_osnr + 2) / 10)
                for i, br in enumerate(table_rates):
                    v = (average_power * amp_spam) / (
                        SNR_min_calc * h * f_hz * amp_gain * nf * (br / mod.spectral_efficiency) * 1e9)
                    lmax_snr[m, i] = v / 1000
                lmax_xt[m] = 10 ** ((mod.inband_xt - worst_xt - 4) / 10)
        cum_class = class_reward = None
        if self.ENV_TYPE == 4:  # qos_constrained_ra.py:43-47, 262-265
            assert num_service_classes == len(classes_arrival_probabilities)
            self.num_service_classes = int(num_service_classes)
            self.classes_arrival_probabilities = list(classes_arrival_probabilities)
            self.classes_reward = list(classes_reward)
            cum_class = np.array(list(itertools.accumulate(classes_arrival_probabilities)), np.float64)
            class_reward = np.array(classes_reward, np.float64)
        path_mod = t.path_best_mod if modulations is None else t.path_modulation_for(mods)
        # ---- hand everything to the C ABI ----
        keep = dict(
            n_paths=np.ascontiguousarray(t.n_paths, np.int32), path_hops=np.ascontiguousarray(t.path_hops, np.int32),
            path_links=np.ascontiguousarray(t.path_links, np.int32),
            path_length=np.ascontiguousarray(t.path_length, np.float64),
            path_mod=np.ascontiguousarray(path_mod, np.int32),
            edge_iter_order=np.ascontiguousarray(t.edge_iter_order, np.int32),
            cum_src=cum_src, cum_dst=np.ascontiguousarray(cum_dst), bit_rates=np.array(table_rates, np.int32),
            cum_br=cum_br, n_slots=np.ascontiguousarray(n_slots), lmax_snr=lmax_snr, lmax_xt=lmax_xt,
            cum_class=cum_class, class_reward=class_reward)
        self._keep = keep
        desc = _lib.TopologyDesc(t.n_nodes, t.n_links, t.k_paths, t.max_hops, M, _ptr(keep["n_paths"]),
                                 _ptr(keep["path_hops"]), _ptr(keep["path_links"]), _ptr(keep["path_length"]),
                                 _ptr(keep["path_mod"]), _ptr(keep["edge_iter_order"]))
        cfg = _lib.EnvConfig(C.sizeof(_lib.EnvConfig), self.ENV_TYPE, num_spectrum_resources, num_spatial_resources, episode_length,
                             int(self.allow_rejection), j, mode, lo, hi, len(table_rates), event_capacity,
                             int(self.action_histograms),
                             lambda_a, lambda_h, _ptr(cum_src), _ptr(keep["cum_dst"]), _ptr(keep["bit_rates"]),
                             _ptr(cum_br), _ptr(keep["n_slots"]), _ptr(lmax_snr), _ptr(lmax_xt),
                             int(num_service_classes) if self.ENV_TYPE == 4 else 0, 0, _ptr(cum_class), _ptr(class_reward))
        if getattr(self, "_derive_only", False):  # spec_flags(): the configuration without a device
            self._cfg, self._desc, self._h, self._topo_h = cfg, desc, None, None
            return
        self._topo_h = C.c_void_p()
        self._ck(self.lib.orl_topology_create(C.byref(desc), device_id, C.byref(self._topo_h)))
        self._cfg, self._desc = cfg, desc  # (kept: what orl_multi_create takes to build the same envs over several devices)
        self._h = C.c_void_p()
        int_seeds = [41 if s_ is None else int(s_) for s_ in self.seeds]
        lam_a, lam_h = self._rate_arrays
        if mt_state is None and all(-2**63 < s_ < 2**63 for s_ in int_seeds):
            # device-side random.Random(seed): no 2.5 KB/env upload, no Python loop over envs
            sd = np.array(int_seeds, np.int64)
            if lam_a is None:
                self._ck(self.lib.orl_batch_create_seeded(C.byref(cfg), self._topo_h, self.num_envs, sd.ctypes.data,
                                                            C.byref(self._h)))
            else:
                self._ck(self.lib.orl_batch_create_with_rates(C.byref(cfg), self._topo_h, self.num_envs, None, sd.ctypes.data,
                                                                lam_a.ctypes.data, lam_h.ctypes.data, C.byref(self._h)))
        else:  # given states; seeds beyond 64 bits: let CPython expand them
            st = mt_states(self.seeds) if mt_state is None else mt_state
            if lam_a is None:
                self._ck(self.lib.orl_batch_create(C.byref(cfg), self._topo_h, self.num_envs, st.ctypes.data,
                                                     C.byref(self._h)))
            else:
                self._ck(self.lib.orl_batch_create_with_rates(C.byref(cfg), self._topo_h, self.num_envs, st.ctypes.data, None,
                                                                lam_a.ctypes.data, lam_h.ctypes.data, C.byref(self._h)))
        self.n_info = self.lib.orl_batch_info_dim(self._h)
        self.obs_dim = self.lib.orl_batch_obs_dim(self._h)
        self.specialised = self._attach_specialisation()
        n = self.num_envs
        # host-side I/O arrays in page-locked memory: every step() moves actions in and reward/done/info(/obs) out
        self._act = self._host_array((n, 4), np.int32)
        self._act_in = self._host_array((n, 4), np.int32)
        self._reward = self._host_array((n,), np.float64)
        self._done = self._host_array((n,), np.uint8)
        self._info = self._host_array((n, self.n_info), np.float64)
        self._obs = self._host_array((n, self.obs_dim), np.float64) if self.obs_dim else None

    # ---- the persistent kernel with this configuration's sizes as compile-time constants ------------------------------
    JIT_MIN_ENVS = 4096

    def _attach_specialisation(self):
        """Attach the specialisation library of this configuration (include/orl.h, orl_batch_load_spec): a cached one whenever
        it exists; built on first use (~15 s of hipcc, once per configuration and source state) for batches of at least
        JIT_MIN_ENVS envs — where 5-12 % of the device loop are worth it — or whenever ORL_JIT_SPEC=1; ORL_JIT_SPEC=0: never.
        Returns whether one is attached.  Default library only (the cross-implementation builds keep the generic kernels)."""
        mode = os.environ.get("ORL_JIT_SPEC", "")
        variant = os.environ.get("ORL_LIB_VARIANT", "default")
        if mode == "0" or variant not in ("default", "exp") or (_build._extra() and variant != "exp"):
            return False
        buf = C.create_string_buffer(1024)
        if self.lib.orl_batch_spec_flags(self._h, buf, len(buf)) <= 0:
            return False
        flags = buf.value.decode()
        if os.environ.get("ORL_SPEC_EXTRA"):  # A/B experiments on the specialised kernels only: extra compiler flags (part of the cache key)
            flags += " " + os.environ["ORL_SPEC_EXTRA"]
        path = _build.spec_path(flags)
        from_cache = True
        if os.environ.get("ORL_SPEC_LIB"):  # A/B: a specialisation library built elsewhere (e.g. from another commit's device code)
            path = os.environ["ORL_SPEC_LIB"]
            from_cache = False  # (the user's file: never deleted, whatever the library says about it)
        if not os.path.exists(path):
            if not (mode == "1" or self.num_envs >= self.JIT_MIN_ENVS):
                return False
            try:
                path = _build.build_spec(flags)
            except Exception as exc:  # no compiler on this machine: the generic kernel runs
                import warnings

                warnings.warn("optical_rl_gym_amd: specialisation not built (%s); the generic persistent kernel runs" % exc)
                return False
        try:
            self._ck(self.lib.orl_batch_load_spec(self._h, path.encode()))
        except _lib.OrlError as exc:  # a cached library that no longer loads (another ROCm, a damaged file): optional, never fatal
            import warnings

            warnings.warn("optical_rl_gym_amd: specialisation %s not attached (%s); the generic persistent kernel runs"
                          % (os.path.basename(path), exc))
            # a cache entry that cannot be opened or is not a specialisation library is dropped (it would fail again every time);
            # one that is merely for another configuration or layout stays, and so does anything the user named
            if from_cache and any(t in str(exc) for t in ("dlopen", "not a specialisation", "other sources")):
                try:
                    os.unlink(path)
                except OSError:
                    pass
            return False
        return True

    @classmethod
    def spec_flags(cls, batch=1 << 20, **kwargs):
        """The -D flags of this configuration's specialisation for a batch of `batch` envs (the kernel form depends on it),
        computed without a device (pre-building, __graft_entry__.build)."""
        self = cls._derived(**kwargs)
        buf = C.create_string_buffer(1024)
        n = self.lib.orl_spec_flags_for_batch(C.byref(self._cfg), C.byref(self._desc), int(batch), buf, len(buf))
        return buf.value.decode() if n > 0 else None

    @classmethod
    def _derived(cls, **kwargs):
        """This configuration as the C ABI takes it (_cfg, _desc), without a device or a batch."""
        self = cls.__new__(cls)
        self._derive_only = True
        self.__init__(num_envs=1, **kwargs)
        return self

    PERSIST_CHOICE_FIELDS = ("form", "lds_arg", "waves", "rw", "inner", "evl", "window_bytes", "launch_lds_bytes", "wgs_per_cu")

    def persist_choice(self, batch, tuned=True, variant=None):
        """What the launcher of the persistent kernel chooses for a batch of `batch` envs of this configuration (include/orl.h,
        orl_debug_persist_choice; no device needed): a tuple in the order of PERSIST_CHOICE_FIELDS, None where the persistent
        kernel does not serve the configuration.  `variant`: the library build asked ("alt" carries forms 2 and 3)."""
        out = (C.c_int32 * len(self.PERSIST_CHOICE_FIELDS))()
        lib = _lib.lib(variant) if variant else self.lib
        n = lib.orl_debug_persist_choice(C.byref(self._cfg), C.byref(self._desc), int(batch), int(bool(tuned)), out)
        return tuple(out) if n > 0 else None

    RUN_PLAN_FIELDS = ("persist", "two_kernel", "agent_step", "item_masks", "rel_limit", "chunk", "parts", "half", "log_cap", "elog_cap",
                       "clear_counters")

    def run_plan(self, batch, n_steps, tuned=True, n_cu=256, log_cap_have=0, run_base=0, wg_dirty=False, variant=None):
        """The step route of a batch of `batch` envs of this configuration and the plan of a device-resident run of `n_steps` steps
        (include/orl.h, orl_debug_run_plan; no device needed): a tuple in the order of RUN_PLAN_FIELDS, None for a configuration
        the library refuses."""
        out = (C.c_int32 * len(self.RUN_PLAN_FIELDS))()
        lib = _lib.lib(variant) if variant else self.lib
        n = lib.orl_debug_run_plan(C.byref(self._cfg), C.byref(self._desc), int(batch), int(n_steps), int(bool(tuned)), int(n_cu),
                                   int(log_cap_have), int(run_base), int(bool(wg_dirty)), out)
        return tuple(out) if n > 0 else None

    def _ck(self, rc):
        _lib.check(rc, self.lib)

    def host_array(self, shape, dtype):
        """A page-locked numpy array (copies to and from it run at the full PCIe rate), e.g. for `step(obs_out=...)`."""
        return self._host_array(shape, dtype)

    def _host_array(self, shape, dtype):
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        ptr = C.c_void_p()
        self._ck(self.lib.orl_host_alloc(max(nbytes, 1), C.byref(ptr)))
        buf = (C.c_ubyte * max(nbytes, 1)).from_address(ptr.value)
        buf._block = _PinnedBlock(self.lib, ptr)  # freed when the last numpy view of it is gone, not at close()
        return np.frombuffer(buf, dtype=np.uint8, count=nbytes).view(dtype).reshape(shape)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.orl_batch_destroy(self._h)
            self._h = None
        if getattr(self, "_topo_h", None):
            self.lib.orl_topology_destroy(self._topo_h)
            self._topo_h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the gym surface, batched ---------------------------------------------------------------
    def reset(self, full=False, mask=None):
        """reset(only_episode_counters = not full) for the envs selected by `mask` (default: all)."""
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self._ck(self.lib.orl_batch_reset(self._h, int(full), _ptr(m)))
        return self.observation() if self.obs_dim else None

    def set_paths(self, paths):
        """The path each env's agent chose (PathOnlyFirstFitAction's Discrete(k + reject) action) for policy "PATH_FF"."""
        p = np.ascontiguousarray(np.asarray(paths).reshape(self.num_envs), np.int32)
        self._ck(self.lib.orl_batch_set_paths(self._h, p.ctypes.data))

    def policy(self, policy, fetch=True, paths=None):
        """On-device heuristic; returns [num_envs, 4] int32 actions (or None with fetch=False: they stay on
        the GPU for the next step(None)).  policy "PATH_FF" (PathOnlyFirstFitAction, rmsa_env.py:840-874 /
        rwa_env.py:505-536) takes the agents' path choices in `paths` (or from a previous set_paths / the "paths"
        device array)."""
        pid = POLICIES[policy] if isinstance(policy, str) else int(policy)
        if paths is not None:
            self.set_paths(paths)
        self._ck(self.lib.orl_batch_policy(self._h, pid, self._act.ctypes.data if fetch else None))
        return self._act if fetch else None

    def step(self, actions, auto_reset=False, fetch=True, obs_out=None, fetch_info=True):
        """actions: [num_envs, n_action] ints, or None to use the device-resident result of policy(fetch=False).
        Returns (obs, reward, done, info) arrays; info is [num_envs, n_info] in `info_keys` order.  The arrays are this
        object's page-locked staging buffers, overwritten by the next step.  `obs_out`: a caller-owned [num_envs, obs_dim]
        float64 or float32 array (ideally from `host_array`) that receives the observation instead — float32 is cast on the
        device (half the PCIe bytes, no host pass).  `fetch_info=False`: info stays on the device (None is returned for it);
        `info_rows(indices)` reads the rows that are needed afterwards."""
        if fetch:
            # the same call in its two halves (orl_batch_step_async / _wait): the action rows are checked and widened in ONE pass
            # inside the library instead of a strided numpy copy here and a second pass there (0.33 -> 0.2 ms at 65 536 envs)
            self.step_async(actions, auto_reset=auto_reset, obs_out=obs_out, fetch_info=fetch_info)
            return self.step_wait()
        a = None
        if actions is not None:
            actions = np.asarray(actions)
            if actions.ndim == 1:
                actions = actions[:, None]
            a = self._act_in  # columns beyond the family's action width stay zero from allocation
            a[:, : actions.shape[1]] = actions
        self._ck(self.lib.orl_batch_step(self._h, _ptr(a), int(auto_reset), None, None, None, None))
        return None

    def policy_step(self, policy, auto_reset=False, fetch=True, paths=None):
        """policy(policy) and step() on its actions in one call (include/orl.h, orl_batch_policy_step): ONE launch where the
        8-lanes-per-env step kernel serves the batch — the slot scan is its first phase.  Returns (actions, obs, reward, done,
        info) like policy() / step(), or None with fetch=False (everything stays on the GPU; nothing is synchronised)."""
        pid = POLICIES[policy] if isinstance(policy, str) else int(policy)
        if paths is not None:
            self.set_paths(paths)
        if not fetch:
            self._ck(self.lib.orl_batch_policy_step(self._h, pid, int(auto_reset), None, None, None, None, None))
            return None
        self._ck(self.lib.orl_batch_policy_step(self._h, pid, int(auto_reset), self._act.ctypes.data, _ptr(self._obs), self._reward.ctypes.data,
                                                  self._done.ctypes.data, self._info.ctypes.data))
        return self._act, self._obs, self._reward, self._done, self._info

    def set_info_mode(self, rates_only):
        """rates_only=True: the 8-lanes-per-env step kernel writes the blocking rates of info only (include/orl.h,
        orl_batch_set_info_mode); the compactness entries and the two link means keep whatever was written before."""
        self._ck(self.lib.orl_batch_set_info_mode(self._h, 1 if rates_only else 0))

    def action_bounds(self):
        """Exclusive upper bound per action column (None: any integer) — the index ranges of the reference's actions_output
        arrays that orl_batch_step checks before it modifies anything (rmsa_env.py:126-137, 167; rwa_env.py:52-58, 103;
        rmcsa_env.py:145-153, 219; qos_constrained_ra.py:101; DeepRMSA decodes any integer, deeprmsa_env.py:48-58)."""
        K, S, rej = self.k_paths, self.num_spectrum_resources, 1 if self.allow_rejection else 0
        t = self.ENV_TYPE
        if t == 0:
            return (K + 1, S + 1)
        if t == 2:
            return (K + rej, S + rej)
        if t == 3:
            return (K + 1, len(self.modulation_formats) + 1, self.num_spatial_resources + 1, S + 1)
        if t == 4:
            return (K + rej,)
        return (None,)

    def validate_actions(self, actions):
        """Raises the IndexError step() would, without touching the batch (a MultiDeviceBatch checks every shard's slice before it
        queues a step on any of them)."""
        if actions is None:
            return
        a = np.asarray(actions)
        if a.ndim == 1:
            a = a[:, None]
        for c, hi in enumerate(self.action_bounds()[: a.shape[1]]):
            if hi is None:
                continue
            bad = np.flatnonzero((a[:, c] < 0) | (a[:, c] >= hi))
            if len(bad):
                raise IndexError("action %s of env %d is outside the action space" % (tuple(int(v) for v in a[bad[0]]), int(bad[0])))

    def step_sync_abi(self, actions, auto_reset=False):
        """The synchronous entry point `orl_batch_step` with every output, as a C caller would use it ([num_envs][4] int32 action
        rows; tests compare it with the two-halves path)."""
        a = self._act_in
        a[:] = 0
        actions = np.asarray(actions)
        if actions.ndim == 1:
            actions = actions[:, None]
        a[:, : actions.shape[1]] = actions
        self._ck(self.lib.orl_batch_step(self._h, a.ctypes.data, int(auto_reset), _ptr(self._obs), self._reward.ctypes.data,
                                           self._done.ctypes.data, self._info.ctypes.data))
        return self._obs, self._reward, self._done, self._info

    def step_async(self, actions, auto_reset=False, obs_out=None, fetch_info=True):
        """First half of step() (include/orl.h, orl_batch_step_async): checks the actions, queues the copies and the kernel on
        the batch's stream and returns at once.  `step_wait()` collects what `step()` would have returned."""
        a, width, esz = None, 0, 0
        if actions is not None:
            a = np.asarray(actions)
            if a.ndim == 1:
                a = a[:, None]
            if a.dtype not in (np.int32, np.int64) or not a.flags.c_contiguous:
                a = np.ascontiguousarray(a, np.int64)
            assert a.shape[0] == self.num_envs and 1 <= a.shape[1] <= 4
            width, esz = a.shape[1], a.dtype.itemsize
            self._pending_actions = a  # (kept alive until the call returns: the library copies it before it does)
        obs64 = obs32 = None
        if self.obs_dim:
            obs = self._obs if obs_out is None else obs_out
            assert obs.shape == (self.num_envs, self.obs_dim) and obs.flags.c_contiguous
            if obs.dtype == np.float32:
                obs32 = obs
            else:
                assert obs.dtype == np.float64
                obs64 = obs
        else:
            obs = None
        self._ck(self.lib.orl_batch_step_async(self._h, _ptr(a), width, esz, int(auto_reset), _ptr(obs64), _ptr(obs32), self._reward.ctypes.data,
                                                 self._done.ctypes.data, self._info.ctypes.data if fetch_info else None))
        # (a refused call — bad action, a step still pending — leaves what step_wait() returns as it was)
        self._pending_obs, self._pending_info = obs, (self._info if fetch_info else None)

    def step_wait(self):
        self._ck(self.lib.orl_batch_step_wait(self._h))
        return self._pending_obs, self._reward, self._done, self._pending_info

    def info_rows(self, indices):
        """Rows `indices` of the info array the last step left on the device: [len(indices), n_info] float64 (gathered on the
        device; a VecEnv needs the rows of the envs that just finished an episode, not 4 MB of info per step)."""
        idx = np.ascontiguousarray(indices, np.int64)
        out = np.empty((len(idx), self.n_info), np.float64)
        if len(idx):
            self._ck(self.lib.orl_batch_get_info_rows(self._h, idx.ctypes.data, len(idx), out.ctypes.data))
        return out

    def run(self, policy, n_steps, time_kernels=False):
        """n_steps x (policy; step with auto reset) without leaving the device; returns RunStats."""
        pid = POLICIES[policy] if isinstance(policy, str) else int(policy)
        st = _lib.RunStats()
        self._ck(self.lib.orl_batch_run(self._h, pid, int(n_steps), int(time_kernels), C.byref(st)))
        return st

    def sync(self):
        self._ck(self.lib.orl_batch_sync(self._h))

    # ---- evaluate_heuristic on the device (utils.py:103-141) ---------------------------------------------------
    def steps_per_episode(self):
        """RMSA / DeepRMSA / RMCSA episodes last episode_length - 1 steps (the soft reset counts the pending service again,
        rmsa_env.py:310-315), RWA episodes episode_length steps (rwa_env.py:135-136, 160)."""
        return self.episode_length if self.ENV_TYPE in (2, 4) else self.episode_length - 1

    def evaluate(self, policy, n_eval_episodes=10):
        """n_eval_episodes episodes of every env under the on-device heuristic `policy`, with the reference harness's
        accounting (reset -> loop until done -> sum of rewards): returns (episode_rewards [num_envs, n_eval_episodes],
        episode_lengths).  One device-resident run; the kernels log each finished episode."""
        n = int(n_eval_episodes)
        refuse_endless_episodes(self.steps_per_episode(), self.episode_length)  # (before the batch is touched)
        self._ck(self.lib.orl_batch_reset(self._h, 0, None))  # the harness's reset() before the first episode (soft)
        self._ck(self.lib.orl_batch_episode_log(self._h, n))
        L = self.steps_per_episode()
        counts = np.zeros(self.num_envs, np.int32)
        acc = np.zeros((self.num_envs, n), np.int32)
        try:
            # the harness stops at the last done without resetting: all steps but the last in one device-resident run (auto
            # reset between episodes = the harness's reset() at the start of the next one), the last one without auto reset
            if n * L > 1:
                self.run(policy, n * L - 1)
            self.policy(policy, fetch=False)
            self.step(None, auto_reset=False, fetch=False)
            self.check()
            self._ck(self.lib.orl_batch_get_episode_log(self._h, counts.ctypes.data, acc.ctypes.data))
            qos_rewards = None
            if self.ENV_TYPE == 4:  # class rewards: the kernels kept the float64 sums (qos_constrained_ra.py:131-136)
                qos_rewards = np.zeros((self.num_envs, n), np.float64)
                self._ck(self.lib.orl_batch_get_episode_rewards(self._h, qos_rewards.ctypes.data))
        finally:  # whatever happened above, the next run must not append to a log nobody reads
            self._ck(self.lib.orl_batch_episode_log(self._h, 0))
        assert (counts == n).all(), "every env finishes exactly n episodes in n * steps_per_episode steps"
        rewards = acc.astype(np.float64) if qos_rewards is None else qos_rewards
        if self.ENV_TYPE == 1:  # DeepRMSA: +1 accepted, -1 otherwise (deeprmsa_env.py:123-124)
            rewards = 2.0 * rewards - L
        return rewards, np.full((self.num_envs, n), L, np.int64)

    def check(self):
        """Synchronise and raise what the kernels flagged since the last report: IndexError for a device-resident action
        outside the action space (rmsa_env.py:167), OverflowError when an env ran out of pending-release slots."""
        self._ck(self.lib.orl_batch_check(self._h))

    def seed(self, seeds, mask=None):
        """seed(seed) of the selected envs (optical_network_env.py:205-210): env i continues with the stream of
        random.Random(seeds[i]); a scalar means seed + i.  Nothing else of the state changes."""
        if np.isscalar(seeds):
            seeds = [int(seeds) + i for i in range(self.num_envs)]
        sd = np.array([41 if x is None else int(x) for x in seeds], np.int64)
        assert sd.shape == (self.num_envs,)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self._ck(self.lib.orl_batch_reseed(self._h, sd.ctypes.data, _ptr(m)))
        for i in range(self.num_envs):
            if m is None or m[i]:
                self.seeds[i] = int(sd[i])

    # ---- traffic load (include/orl.h, orl_batch_set_rates) ---------------------------------------------
    def _derive_set_load(self, load=None, mean_service_holding_time=None, mask=None):
        """What set_load hands to the library and keeps: (load, mean_service_holding_time, mean_service_inter_arrival_time,
        lambda_arrival[num_envs], lambda_holding[num_envs], mask or None).  Host only; ValueError for a bad argument."""
        n = self.num_envs
        m = None
        if mask is not None:
            m = np.ascontiguousarray(mask, np.uint8)
            if m.shape != (n,):
                raise ValueError("mask must have one entry per env (length %d), got shape %r" % (n, m.shape))
        load_v = per_env_values(load, n, "load")
        mht_v = per_env_values(mean_service_holding_time, n, "mean_service_holding_time")
        if load is not None and load_v is None:
            _check_scalar(load, "load")
        if mean_service_holding_time is not None and mht_v is None:
            _check_scalar(mean_service_holding_time, "mean_service_holding_time")
        uniform = m is None and load_v is None and mht_v is None and np.isscalar(self.load) and np.isscalar(self.mean_service_holding_time)
        if uniform:  # one pair for the whole batch, as the reference env's set_load (optical_network_env.py:86-94)
            new_load = self.load if load is None else load
            new_mht = self.mean_service_holding_time if mean_service_holding_time is None else mean_service_holding_time
            miat = 1 / float(new_load / float(new_mht))
            return new_load, new_mht, miat, np.full(n, 1 / miat, np.float64), np.full(n, 1 / new_mht, np.float64), None
        sel = np.ones(n, bool) if m is None else m != 0
        new_load = np.array(np.broadcast_to(np.asarray(self.load, np.float64), (n,)))
        new_mht = np.array(np.broadcast_to(np.asarray(self.mean_service_holding_time, np.float64), (n,)))
        if load is not None:
            new_load[sel] = load_v[sel] if load_v is not None else float(load)
        if mean_service_holding_time is not None:
            new_mht[sel] = mht_v[sel] if mht_v is not None else float(mean_service_holding_time)
        miat, lam_a, lam_h = derive_rates(new_load, new_mht)
        return new_load, new_mht, miat, lam_a, lam_h, m

    def set_load(self, load=None, mean_service_holding_time=None, mask=None):
        """set_load (optical_network_env.py:76-94) of the envs selected by `mask` (default: all): scalars or one value per env.
        Per env a given load replaces the env's load, a given holding time its holding time, and the mean inter-arrival time
        follows from the two; services drawn from now on use them, the pending service and everything else stay.  ValueError
        for a bad value; the library refuses (nothing changed) a load the batch's event_capacity is too small for."""
        new_load, new_mht, miat, lam_a, lam_h, m = self._derive_set_load(load, mean_service_holding_time, mask)
        self._ck(self.lib.orl_batch_set_rates(self._h, lam_a.ctypes.data, lam_h.ctypes.data, _ptr(m)))
        self.load, self.mean_service_holding_time, self.mean_service_inter_arrival_time = new_load, new_mht, miat

    def event_capacity_in_force(self):
        """Pending releases per env this batch has room for (include/orl.h, orl_batch_event_capacity)."""
        return int(self.lib.orl_batch_event_capacity(self._h))

    @staticmethod
    def capacity_needed(load):
        """The pending releases the library gives an env at `load` Erlang room for — what set_load's load must fit into."""
        return int(load + 10.0 * math.sqrt(load) + 64.0)

    def rates(self):
        """(lambda_arrival, lambda_holding) = (1 / mean_service_inter_arrival_time, 1 / mean_service_holding_time) of every
        env as the device holds them: two float64 arrays of length num_envs."""
        la, lh = np.zeros(self.num_envs, np.float64), np.zeros(self.num_envs, np.float64)
        self._ck(self.lib.orl_batch_get_rates(self._h, la.ctypes.data, lh.ctypes.data))
        return la, lh

    # ---- the views of the pending service: action masks, MatrixObservationWithPaths, path features ---------------------------
    def _view_rows(self, call, dim, dtype, fetch, out=None):
        """The rows of one view: `call(host pointer or None)` queues the launch and, given a pointer, fetches [num_envs, dim()] items
        of `dtype` into it.  fetch=False only queues (returns None); otherwise the rows land in `out` or in a fresh array."""
        if not fetch:
            call(None)
            return None
        shape = (self.num_envs, dim())
        if out is None:
            out = np.empty(shape, dtype)
        elif out.shape != shape or out.dtype != dtype or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous %s array of shape %r" % (np.dtype(dtype).name, shape))
        call(out.ctypes.data)
        return out

    # ---- action masks (include/orl.h, orl_batch_action_mask) -------------------------------------------
    MASK_LAYOUTS = {"joint": 0, "path": 1, "path_modulation": 2, "core_slot": 3}

    def action_mask_shape(self, layout="joint"):
        """(dim, pitch) of the rows of `layout`: dim columns per env, rows pitch bytes apart in the device buffer."""
        d, p = C.c_int32(), C.c_int32()
        self._ck(self.lib.orl_batch_action_mask_shape(self._h, self.MASK_LAYOUTS[layout], C.byref(d), C.byref(p)))
        return d.value, p.value

    def action_mask(self, layout="joint", fetch=True, given=None):
        """Action mask of the pending service of every env, computed on the device: bool [num_envs, dim].  "joint": RMSA / RWA
        column p * S + s = action (p, s), DeepRMSA column i = action i; "path": PathOnlyFirstFitAction's Discrete(k + 1).  RMCSA has
        the two stages of its (path, modulation, core, slot) action instead: "path_modulation", column p * M + m = some (core,
        slot) provisions under that pair, and "core_slot", column c * S + s = (c, s) provisions under the env's pair — `given`,
        an int array [num_envs, 2] of (path, modulation), or with given=None columns 0 and 1 of device_array("actions"), where an
        agent on the GPU writes its stage-1 choice; a pair out of range or beyond reach has no provisioning column.  The
        last column is the reject action (= allow_rejection); a row without a provisioning action and allow_rejection=False is
        all ones but for it (every action rejects then).  fetch=False only queues the launch on the batch's stream — read the
        rows in place with device_array("action_mask") / device_tensor("action_mask")."""
        lay = self.MASK_LAYOUTS[layout]
        g = None
        if given is not None:
            if layout != "core_slot":
                raise ValueError("given (path, modulation) pairs belong to the \"core_slot\" layout, not %r" % (layout,))
            g = np.asarray(given)
            if g.shape != (self.num_envs, 2) or g.dtype.kind not in "iu":
                raise ValueError("given must be an int array of shape %r, got %s %r" % ((self.num_envs, 2), g.dtype, g.shape))
            g = np.ascontiguousarray(g, np.int32)
        gp = None if g is None else g.ctypes.data
        out = self._view_rows(lambda p: self._ck(self.lib.orl_batch_action_mask_given(self._h, lay, gp, p)),
                              lambda: self.action_mask_shape(layout)[0], np.uint8, fetch)
        self._mask_layout = layout
        return None if out is None else out.view(np.bool_)

    # ---- first-fit completion of partial RMCSA actions (include/orl.h, orl_batch_complete_actions) ------------------------------
    @staticmethod
    def completion_prefix(given, n_given, num_envs):
        """(int32 [num_envs, g] or None, g) from the arguments of complete_actions(); ValueError for a bad shape or dtype."""
        if given is None:
            if n_given is None:
                raise ValueError("n_given is required with given=None (the prefix is read from the actions buffer)")
            return None, int(n_given)
        g = np.asarray(given)
        if g.ndim == 1:
            g = g[:, None]
        if g.ndim != 2 or g.shape[0] != num_envs or not 1 <= g.shape[1] <= 3 or g.dtype.kind not in "iu":
            raise ValueError("given must be an int array of shape (%d, 1 .. 3) or (%d,), got %s %r" % (num_envs, num_envs, g.dtype, g.shape))
        n = g.shape[1] if n_given is None else int(n_given)
        if n != g.shape[1] and 1 <= n <= 3:  # (an n_given outside 1 .. 3 is the library's to refuse, with or without `given`)
            raise ValueError("n_given = %d, but given has %d columns" % (n, g.shape[1]))
        return np.ascontiguousarray(g, np.int32), n

    def complete_actions(self, given=None, n_given=None, fetch=True):
        """RMCSA: complete a prefix of every env's (path, modulation, core, first slot) action first-fit on the device, under the
        rule of the two-stage masks: int32 [num_envs, 4], left in device_array("actions") for the next step(None).  `given`: an int
        array [num_envs, g], g = 1 (the path; a 1-D array too), 2 (+ modulation) or 3 (+ core); given=None with n_given = 0 .. 3
        reads the prefix from columns 0 .. n_given - 1 of device_array("actions"), where an agent on the GPU writes it (n_given=0: a
        reach-aware first fit over all paths).  g = 2 yields the lowest set column of the pair's "core_slot" row; g = 1 takes the
        modulation within reach that needs the fewest slots, and provisions iff any of the path's M columns of the
        "path_modulation" row is set.  No completion (a column out of range, a pair beyond reach, no room) is the reject action
        (k, M, C, S).  Env state and flags are not touched.  fetch=False only queues the launch on the batch's stream (returns
        None; graph-capturable with given=None)."""
        g, n = self.completion_prefix(given, n_given, self.num_envs)
        out = self._act if fetch else None
        self._keep_given = g  # (alive until the call returns: the library copies it before it does)
        self._ck(self.lib.orl_batch_complete_actions(self._h, n, None if g is None else g.ctypes.data, None if out is None else out.ctypes.data))
        return None if out is None else out.copy()

    # ---- spectrum-assignment rules for RMSA / RWA actions (include/orl.h, orl_batch_assign_spectrum) ---------------------------
    ASSIGN_RULES = {"first": 0, "last": 1, "best": 2, "exact": 3, "most_used": 4, "least_used": 5}

    @staticmethod
    def _named_id(what, names, value):
        """The id of a name out of `names` (an int passes through: an unknown id is the library's to refuse)."""
        if isinstance(value, str):
            if value not in names:
                raise ValueError("%s must be one of %s, got %r" % (what, ", ".join(map(repr, names)), value))
            return names[value]
        return int(value)

    @classmethod
    def assignment_rule(cls, rule):
        """The ORL_ASSIGN_* id of a rule's name (an int passes through: an unknown id is the library's to refuse)."""
        return cls._named_id("rule", cls.ASSIGN_RULES, rule)

    @staticmethod
    def assignment_paths(paths, n_given, num_envs):
        """(int32 [num_envs] or None, n_given) from the arguments of assign_spectrum(); ValueError for a bad shape or dtype."""
        if paths is None:
            return None, 0 if n_given is None else int(n_given)
        p = np.asarray(paths)
        if p.ndim != 1 or p.shape[0] != num_envs or p.dtype.kind not in "iu":
            raise ValueError("paths must be an int array of shape (%d,), got %s %r" % (num_envs, p.dtype, p.shape))
        return np.ascontiguousarray(p, np.int32), 1 if n_given is None else int(n_given)

    def assign_spectrum(self, rule="first", paths=None, n_given=None, fetch=True):
        """RMSA / RWA: choose every env's first slot (RWA: wavelength) on the device under a spectrum-assignment rule — "first",
        "last", "best", "exact", "most_used" or "least_used" (include/orl.h, ORL_ASSIGN_*) — among the starts at which stepping
        the action provisions, the set columns of the path's part of the "joint" mask (s = S - n included, which "PATH_FF" never
        tries): int32 [num_envs, 4] rows (path, slot, 0, 0), left in device_array("actions") for the next step(None).  `paths`: a
        1-D int array, the path per env; paths=None with n_given=1 reads column 0 of device_array("actions"), where an agent on
        the GPU writes it; paths=None with n_given=0 (the default) takes the first path in order on which the service fits, then
        the rule on that path.  No completion (a path out of range, no room) is the reject action (k, S).  Env state and flags are
        not touched.  fetch=False only queues the launch on the batch's stream (returns None; graph-capturable with paths=None)."""
        p, n = self.assignment_paths(paths, n_given, self.num_envs)
        out = self._act if fetch else None
        self._keep_given = p  # (alive until the call returns: the library copies it before it does)
        self._ck(self.lib.orl_batch_assign_spectrum(self._h, self.assignment_rule(rule), n, None if p is None else p.ctypes.data,
                                                    None if out is None else out.ctypes.data))
        return None if out is None else out.copy()

    # ---- routing rules and the per-path assignment table (include/orl.h, orl_batch_route_spectrum): RMSA and RWA ---------------
    ROUTE_RULES = dict(ASSIGN_RULES, min_cuts=6)
    ROUTES = {"ksp": 0, "best": 1, "least_loaded": 2}

    @classmethod
    def route_ids(cls, rule, route):
        """The (ORL_ASSIGN_*, ORL_ROUTE_*) ids of a rule's and a route's names (ints pass through: an unknown id is the library's to
        refuse)."""
        return cls._named_id("rule", cls.ROUTE_RULES, rule), cls._named_id("route", cls.ROUTES, route)

    def assign_table_shape(self):
        """(rows, width, pitch) of the per-path assignment table: rows = k blocks of width = 4 int32 per env, rows of the device
        buffer pitch = 4 k int32 apart."""
        r, w, p = C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self.lib.orl_batch_assign_table_shape(self._h, C.byref(r), C.byref(w), C.byref(p)))
        return r.value, w.value, p.value

    def route_spectrum(self, rule="first", route="best", fetch=True, table=False):
        """RMSA / RWA: choose every env's path AND first slot (RWA: wavelength) on the device.  For every candidate path the kernel
        computes the winner (s*, c*) of `rule` — "first", "last", "best", "exact", "most_used", "least_used" (assign_spectrum's) or
        "min_cuts" (the start that splits the fewest free runs of the path's links) — c* being the rule's integer cost of that
        choice (include/orl.h), and `route` picks among the paths that fit: "ksp" the lowest path (assign_spectrum's choice),
        "best" the smallest c* ("first" + "best" is FF-KSP: the lowest slot over all paths), "least_loaded" the path with the most
        free slots.  Returns int32 [num_envs, 4] rows (path, slot, 0, 0), left in device_array("actions") for the next step(None);
        the reject action (k, S) where no path fits.  table=True: (actions, table), table int32 [num_envs, k, 4] with row p =
        (s*, c*, slots needed on p, free slots of p) — (S, 0x7fffffff, ., .) for a path without a fit, (S, 0x7fffffff, 0, 0) for a
        path the pair does not have — which stays on the device as device_array("assign_table") ([num_envs, 4 k]).  Env state and
        flags are not touched.  fetch=False only queues the launch on the batch's stream (returns None; graph-capturable after
        the first call)."""
        rid, tid = self.route_ids(rule, route)
        out = self._act if fetch else None
        tab = np.empty((self.num_envs, self.k_paths, 4), np.int32) if fetch and table else None
        self._ck(self.lib.orl_batch_route_spectrum(self._h, rid, tid, None if out is None else out.ctypes.data,
                                                   None if tab is None else tab.ctypes.data))
        if out is None:
            return None
        return (out.copy(), tab) if table else out.copy()

    # ---- core and spectrum rules and the (path, core) table (include/orl.h, orl_batch_route_cores): RMCSA ----------------------
    CORE_RULES = {"first": 0, "last": 1, "best": 2, "exact": 3, "min_cuts": 6}
    CORE_ROUTES = dict(ROUTES, ksp_best_core=3, ksp_least_loaded_core=4)

    @classmethod
    def core_route_ids(cls, rule, route):
        """The (ORL_ASSIGN_*, ORL_ROUTE_*) ids of a rule's and a route's names for route_cores() (ints pass through: an unknown id is
        the library's to refuse)."""
        return cls._named_id("rule", cls.CORE_RULES, rule), cls._named_id("route", cls.CORE_ROUTES, route)

    @staticmethod
    def core_prefix(paths, cores, n_given, num_envs):
        """(int32 [num_envs, g] or None, g) from the arguments of route_cores(); ValueError for a bad shape or dtype, or cores
        without paths."""
        if paths is None:
            if cores is not None:
                raise ValueError("cores without paths: the prefix is (path) or (path, core)")
            return None, 0 if n_given is None else int(n_given)
        cols = [np.asarray(paths)] + ([] if cores is None else [np.asarray(cores)])
        for what, c in zip(("paths", "cores"), cols):
            if c.ndim != 1 or c.shape[0] != num_envs or c.dtype.kind not in "iu":
                raise ValueError("%s must be an int array of shape (%d,), got %s %r" % (what, num_envs, c.dtype, c.shape))
        n = len(cols) if n_given is None else int(n_given)
        if n != len(cols) and 1 <= n <= 2:  # (an n_given outside 1 .. 2 is the library's to refuse, with or without a prefix)
            raise ValueError("n_given = %d, but %d prefix column(s) given" % (n, len(cols)))
        return np.ascontiguousarray(np.stack(cols, axis=1), np.int32), n

    def core_table_shape(self):
        """(rows, width, pitch) of the (path, core) table: rows = k * cores blocks of width = 4 int32 per env, rows of the device
        buffer pitch = 4 k cores int32 apart."""
        r, w, p = C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self.lib.orl_batch_core_table_shape(self._h, C.byref(r), C.byref(w), C.byref(p)))
        return r.value, w.value, p.value

    def route_cores(self, rule="first", route="best", paths=None, cores=None, n_given=None, modulation=None, fetch=True, table=False):
        """RMCSA: choose every env's path, core AND first slot on the device.  For every (path, core) pair the kernel computes the
        winner (s*, c*) of `rule` — "first", "last", "best", "exact" or "min_cuts" (route_spectrum's; "most_used" and "least_used"
        have no form over cores) — on the path's free slots in that core, for the slots of the path's modulation: `modulation`
        None = each path's best within reach (complete_actions' choice), m in [0, M) = that modulation for every path, usable
        only where it is within reach.  `route` picks among the pairs that fit: "ksp" the first path and its first core
        (complete_actions' order), "best" the smallest cost c* over all pairs, "least_loaded" the pair with the most free slots,
        "ksp_best_core" / "ksp_least_loaded_core" the first path with a fit and among its cores the smallest c* / the most free
        slots.  `paths` (and `cores`): 1-D int arrays that fix the path (and the core) per env; paths=None with n_given = 1 or 2
        reads them from columns 0 and 2 of device_array("actions"), where an agent on the GPU writes them.  Returns int32
        [num_envs, 4] rows (path, modulation, core, slot), left in device_array("actions") for the next step(None); the reject
        action (k, M, C, S) where no pair fits or a given column is out of range.  table=True: (actions, table), table int32
        [num_envs, k * cores, 4] with row p * cores + c = (s*, c*, slots needed on p, free slots of p in core c) — (S, 0x7fffffff,
        ., .) for a pair without a fit, (S, 0x7fffffff, 0, 0) for a path the service cannot use — always for every pair, whatever
        the prefix; it stays on the device as device_array("core_table") ([num_envs, 4 k cores]).  Env state and flags are not
        touched.  fetch=False only queues the launch on the batch's stream (returns None; graph-capturable with paths=None after
        the first call)."""
        rid, tid = self.core_route_ids(rule, route)
        g, n = self.core_prefix(paths, cores, n_given, self.num_envs)
        mod = -1 if modulation is None else int(modulation)
        out = self._act if fetch else None
        tab = np.empty((self.num_envs, self.k_paths * self.num_spatial_resources, 4), np.int32) if fetch and table else None
        self._keep_given = g  # (alive until the call returns: the library copies it before it does)
        self._ck(self.lib.orl_batch_route_cores(self._h, rid, tid, mod, n, None if g is None else g.ctypes.data,
                                                None if out is None else out.ctypes.data, None if tab is None else tab.ctypes.data))
        if out is None:
            return None
        return (out.copy(), tab) if table else out.copy()

    # ---- block actions (include/orl.h, orl_batch_block_table / orl_batch_select_blocks): RMSA, DeepRMSA, RWA and RMCSA --------
    BLOCK_PLACEMENTS = {"first": 0, "last": 1}

    def block_table_shape(self, j=1):
        """(rows, width, table_pitch, mask_dim, mask_pitch) of the block table and its mask for `j` blocks per row: rows = k (RMCSA:
        k * cores) rows of width = 2 + 2 j int32 per env, rows of the table's device buffer table_pitch int32 apart; the mask has
        mask_dim = rows * j + 1 columns, its rows mask_pitch bytes apart."""
        v = [C.c_int32() for _ in range(5)]
        self._ck(self.lib.orl_batch_block_table_shape(self._h, int(j), *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def block_table(self, j=1, modulation=None, fetch=True):
        """DeepRMSA's (row, free block) action space of every env's pending service, computed on the device: (table, mask).  table
        int32 [num_envs, rows, 2 + 2 j], row r (the path, RMCSA: p * cores + c, the row order of path_features) = (slots needed,
        free slots, start_0, length_0, ..., start_{j-1}, length_{j-1}): the first j maximal free runs that fit the service, in slot
        order; (S, 0) for a block that does not exist, (0, 0, S, 0, ...) for a row the service cannot use.  mask bool [num_envs,
        rows * j + 1]: column r * j + b is set iff block b of row r exists — the columns select_blocks() turns into an action that
        provisions; the last column is the reject action (allow_rejection), and a row without a set column and no rejection gets
        every other column set.  `j` in [1, 8]; on a DeepRMSA batch with its own j the mask is action_mask("joint").  `modulation`
        (RMCSA only): None = each path's best within reach, m in [0, M) = that modulation where it is within reach.  fetch=False
        only queues the launch on the batch's stream (returns None) — read the rows in place with device_array("block_table") /
        device_tensor("block_mask")."""
        j, mod = int(j), -1 if modulation is None else int(modulation)
        tab = msk = None
        if fetch:
            rows, width, _, dim, _ = self.block_table_shape(j)
            tab, msk = np.empty((self.num_envs, rows, width), np.int32), np.empty((self.num_envs, dim), np.uint8)
        self._ck(self.lib.orl_batch_block_table(self._h, j, mod, None if tab is None else tab.ctypes.data, None if msk is None else msk.ctypes.data))
        self._bt_j = j
        return (tab, msk.view(np.bool_)) if fetch else None

    @staticmethod
    def block_indices(blocks, num_envs):
        """int32 [num_envs] or None from the `blocks` of select_blocks(); ValueError for a bad shape or dtype."""
        if blocks is None:
            return None
        a = np.asarray(blocks)
        if a.ndim != 1 or a.shape[0] != num_envs or a.dtype.kind not in "iu":
            raise ValueError("blocks must be an int array of shape (%d,), got %s %r" % (num_envs, a.dtype, a.shape))
        return np.ascontiguousarray(a, np.int32)

    def select_blocks(self, blocks=None, j=1, modulation=None, placement="first", fetch=True):
        """RMSA / RWA / RMCSA: decode every env's block index — a column r * j + b of block_table(j)'s mask — into the env's action on
        the device: the service goes into block b of row r, at the block's lower end (placement "first", DeepRMSA's decode) or its
        upper end ("last").  Returns int32 [num_envs, 4] rows (path, slot, 0, 0), RMCSA (path, modulation, core, slot), left in
        device_array("actions") for the next step(None); the family's reject action for an index < 0 or >= rows * j or a block that
        does not exist.  `blocks`: a 1-D int array; None reads column 0 of device_array("actions"), where an agent on the GPU
        writes its choice.  The kernel recomputes from the slot maps: no block_table() call is needed first, and `j` and
        `modulation` must be those the index was chosen under.  Env state and flags are not touched.  fetch=False only queues the
        launch on the batch's stream (returns None; graph-capturable with blocks=None)."""
        a = self.block_indices(blocks, self.num_envs)
        mod = -1 if modulation is None else int(modulation)
        out = self._act if fetch else None
        self._keep_given = a  # (alive until the call returns: the library copies it before it does)
        self._ck(self.lib.orl_batch_select_blocks(self._h, int(j), mod, self._named_id("placement", self.BLOCK_PLACEMENTS, placement),
                                                  None if a is None else a.ctypes.data, None if out is None else out.ctypes.data))
        return None if out is None else out.copy()

    # ---- MatrixObservationWithPaths (include/orl.h, orl_batch_matrix_paths_observation): QoSConstrainedRA only ---------------
    def matrix_paths_obs_shape(self):
        """(dim, pitch): dim = links * S * (k + 1) + 1 columns per env, rows pitch bytes apart in the device buffer."""
        d, p = C.c_int32(), C.c_int32()
        self._ck(self.lib.orl_batch_matrix_paths_obs_shape(self._h, C.byref(d), C.byref(p)))
        return d.value, p.value

    def matrix_observation_with_paths(self, fetch=True, out=None):
        """MatrixObservationWithPaths (qos_constrained_ra.py:440-493) of every env's pending service, built on the device:
        uint8 [num_envs, dim] — per link a run of ones for its used units, then per path block the usage the link would have
        with the service on that path; the service class in the last column.  `out` (a C-contiguous uint8 [num_envs, dim]
        array) receives the rows instead of a fresh array.  fetch=False only queues the launch on the batch's stream — read
        the rows in place with device_array("matrix_paths_obs") / device_tensor("matrix_paths_obs")."""
        return self._view_rows(lambda p: self._ck(self.lib.orl_batch_matrix_paths_observation(self._h, p)),
                               lambda: self.matrix_paths_obs_shape()[0], np.uint8, fetch, out)

    # ---- path features (include/orl.h, orl_batch_path_features): RMSA, DeepRMSA, RWA and RMCSA --------------------------------
    def path_features_shape(self, j=1):
        """(dim, rows, pitch) of the path-feature rows for `j` blocks per row: dim = 1 + 2 N + rows * (2 j + 3) float32 columns per
        env, rows = k (RMCSA: k * cores), rows of the device buffer pitch FLOATS apart."""
        d, r, p = C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self.lib.orl_batch_path_features_shape(self._h, int(j), C.byref(d), C.byref(r), C.byref(p)))
        return d.value, r.value, p.value

    def path_features(self, j=1, modulation=None, fetch=True, out=None):
        """Path features of every env's pending service, computed on the device: float32 [num_envs, dim] — the feature table of
        DeepRMSAEnv.observation (deeprmsa_env.py:60-121) for every slot-map family.  Column 0 = bit_rate / 100 (RWA: 0), then the
        one-hots of min(src, dst) and max(src, dst), then per candidate path (RMCSA: per path and core, row p * cores + c) a
        block of 2 j + 3 values: start and length of the first j free blocks that fit the service, the slots it needs, the free
        slots and the mean free-run length, normalised as the reference does; -1.0 where a value does not exist.  `j` in [1, 8]
        is independent of a DeepRMSA batch's own j.  `modulation` (RMCSA only): None = each path's best modulation, as SAP_BM_FC_FF;
        m in [0, M) = that modulation for every path.  `out` (a C-contiguous float32 [num_envs, dim] array) receives the rows
        instead of a fresh array.  fetch=False only queues the launch on the batch's stream — read the rows in place with
        device_array("path_features") / device_tensor("path_features")."""
        j, mod = int(j), -1 if modulation is None else int(modulation)
        out = self._view_rows(lambda p: self._ck(self.lib.orl_batch_path_features(self._h, j, mod, p)),
                              lambda: self.path_features_shape(j)[0], np.float32, fetch, out)
        self._pf_j = j
        return out

    # ---- release horizons (include/orl.h, orl_batch_release_horizons): RMSA, DeepRMSA, RWA and RMCSA --------------------------
    HORIZON_LAYOUTS = {"slots": 0, "blocks": 1}

    @classmethod
    def horizon_args(cls, layout, j=1, modulation=None):
        """(layout id, j, modulation or -1) of release_horizons(); ValueError for an unknown layout name, a j outside 1 .. 8, and
        layout "slots" with j != 1 or a modulation."""
        lay, j = cls._named_id("layout", cls.HORIZON_LAYOUTS, layout), int(j)
        if not 1 <= j <= 8:
            raise ValueError("release horizons list j = 1 .. 8 blocks per row, got j = %d" % j)
        if lay == 0 and (j != 1 or modulation is not None):
            raise ValueError('layout "slots" takes neither a block count j nor a modulation')
        return lay, j, -1 if modulation is None else int(modulation)

    def release_horizons_shape(self, layout="slots", j=1):
        """(rows, width, dim, pitch) of the release-horizon rows: rows = k (RMCSA: k * cores), width = S ("slots") or 2 j
        ("blocks"), dim = rows * width + 1 float32 columns per env, rows of the device buffer pitch FLOATS apart."""
        lay, j, _ = self.horizon_args(layout, j)
        r, w, d, p = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        self._ck(self.lib.orl_batch_release_horizons_shape(self._h, lay, j, C.byref(r), C.byref(w), C.byref(d), C.byref(p)))
        return r.value, w.value, d.value, p.value

    def release_horizons(self, layout="slots", j=1, modulation=None, fetch=True, out=None):
        """When each slot frees, for every env's pending service, computed on the device from the env's pending releases (what
        pending(env) reads back one env at a time): float32 [num_envs, dim].  With now = the service's arrival time
        (services()[:, 0]) and the rows of path_features (r = p; RMCSA: r = p * cores + c), H[r, s] = the largest release_time -
        now over the running services that hold slot s (RMCSA: in core c) on a link of candidate path p; 0.0 where none does —
        exactly the free slots of the path's AND-row; -1.0 throughout a row whose path does not exist.  layout "slots": H row by
        row, dim = rows * S + 1.  layout "blocks": for block b < j of row r of block_table(j, modulation) the pair (H[r, start -
        1], H[r, start + length]) at columns r * 2 j + 2 b and + 1 — +inf for a neighbour beyond the spectrum's edge, (-1, -1)
        for a block that does not exist or a row the service cannot use; dim = rows * 2 j + 1.  The last column of both is the
        pending service's holding time.  `out` (a C-contiguous float32 [num_envs, dim] array) receives the rows instead of a fresh
        array.  fetch=False only queues the launch on the batch's stream — read the rows in place with
        device_array("release_horizons") / device_tensor("release_horizons")."""
        lay, j, mod = self.horizon_args(layout, j, modulation)
        out = self._view_rows(lambda p: self._ck(self.lib.orl_batch_release_horizons(self._h, lay, j, mod, p)),
                              lambda: self.release_horizons_shape(lay, j)[2], np.float32, fetch, out)
        self._rh = (lay, j)
        return out

    # ---- link features (include/orl.h, orl_batch_link_features): RMSA, DeepRMSA, RWA and RMCSA --------------------------------
    def link_features_shape(self):
        """(dim, rows, width, pitch) of the link-feature rows: dim = 1 + 2 N + rows * width float32 columns per env, rows = links
        (RMCSA: cores * links, block c * links + l), width = 10 + k, rows of the device buffer pitch FLOATS apart."""
        d, r, w, p = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self.lib.orl_batch_link_features_shape(self._h, C.byref(d), C.byref(r), C.byref(w), C.byref(p)))
        return d.value, r.value, w.value, p.value

    def link_features(self, fetch=True, out=None):
        """The state per link for every env's pending service, computed on the device: float32 [num_envs, dim] — what a graph
        network over the topology reads.  The header of path_features (bit_rate / 100, RWA: 0; one-hots of min(src, dst) and
        max(src, dst)), then per slot row, in the order of the slot maps (link l of topology.path_links and link_stats_all();
        RMCSA: block c * links + l), a block of 10 + k values: free slots / S, free runs / S, longest free run / S, first free slot
        / S and (last free slot + 1) / S (-1.0 for a row without a free slot), the external fragmentation and the compactness of
        the row as it stands (the reference's _update_link_stats expressions), the link's running utilization, external
        fragmentation and compactness (link_stats_all() columns 0 .. 2), and per candidate path p of the pending pair 1.0 where
        the link is on it.  `out` (a C-contiguous float32 [num_envs, dim] array) receives the rows instead of a fresh array.
        fetch=False only queues the launch on the batch's stream — read the rows in place with device_array("link_features") /
        device_tensor("link_features")."""
        return self._view_rows(lambda p: self._ck(self.lib.orl_batch_link_features(self._h, p)),
                               lambda: self.link_features_shape()[0], np.float32, fetch, out)

    # ---- network capacity (include/orl.h, orl_batch_network_capacity): RMSA, DeepRMSA, RWA and RMCSA --------------------------
    CAPACITY_LAYOUTS = {"paths": 0, "serviceable": 1, "counts": 2}

    def network_capacity_shape(self, layout="paths"):
        """(rows, width, dim, pitch) of the network-capacity rows of `layout`: (N N k C', 2) for "paths", (N N, n_cls) for
        "serviceable", (1, n_cls + N N) for "counts"; dim = rows * width columns per env, rows of the device buffer pitch ITEMS
        apart.  C' = cores for RMCSA, else 1; n_cls = 1 for RWA, else the rows of the batch's bit-rate table."""
        lay = self._named_id("layout", self.CAPACITY_LAYOUTS, layout)
        r, w, d, p = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        self._ck(self.lib.orl_batch_network_capacity_shape(self._h, lay, C.byref(r), C.byref(w), C.byref(d), C.byref(p)))
        return r.value, w.value, d.value, p.value

    def network_capacity(self, layout="paths", fetch=True, out=None):
        """What every env's network can still carry, computed on the device from its slot maps, for EVERY ordered node pair (not the
        pending one alone): [num_envs, dim].  With pidx = (src * N + dst) * k + p the index of the topology's path tables, C' =
        cores for RMCSA, else 1, and n_cls classes (RWA: one; else the rows of the bit-rate table, what the pending service's br_idx
        indexes):
        "paths"        int32; reshape(num_envs, N, N, k, C', 2): (longest free run, free slots) of the AND of the path's link rows
                       in core c; (-1, -1) where the path does not exist (p >= n_paths[src, dst], the diagonal included)
        "serviceable"  bool; reshape(num_envs, N, N, n_cls): True where a service of class r between (src, dst) finds room now —
                       some path of the pair, in some core, has a free run of the slots class r needs on it (its best modulation;
                       RMCSA: the fewest-slots modulation within reach, as complete_actions takes it; RWA: one wavelength)
        "counts"       int32; [:, :n_cls]: per class the ordered pairs with paths that are NOT serviceable; [:, n_cls:].reshape(
                       num_envs, N, N): per pair its serviceable classes — the marginals of "serviceable"
        `out` (a C-contiguous [num_envs, dim] array of that type; uint8 for "serviceable") receives the rows instead of a fresh
        array.  fetch=False only queues the launch on the batch's stream — read the rows in place with device_array / device_tensor
        ("path_capacity", "serviceable", "capacity_counts"); every layout has a buffer of its own."""
        lay = self._named_id("layout", self.CAPACITY_LAYOUTS, layout)
        out = self._view_rows(lambda p: self._ck(self.lib.orl_batch_network_capacity(self._h, lay, p)),
                              lambda: self.network_capacity_shape(lay)[2], np.uint8 if lay == 1 else np.int32, fetch, out)
        return out.view(np.bool_) if out is not None and lay == 1 else out

    # ---- capacity_after (include/orl.h, orl_batch_capacity_after): RMSA, DeepRMSA, RWA and RMCSA -------------------------------
    AFTER_LAYOUTS = {"classes": 0, "total": 1}
    AFTER_SOURCES = {"route": 0, "blocks": 1, "given": 2}
    AFTER_MAX_CANDIDATES = 1024

    def capacity_after_shape(self, source="route", layout="total", j=1, n_candidates=0):
        """(Q, width, dim, pitch) of the capacity_after rows: Q candidates per env — k C' for "route", rows * j for "blocks",
        n_candidates for "given" — and Q + 1 rows (the last is the baseline) of width n_cls ("classes") or 1 ("total"); dim =
        (Q + 1) * width columns per env, rows of the device buffer pitch int32 apart."""
        src = self._named_id("source", self.AFTER_SOURCES, source)
        lay = self._named_id("layout", self.AFTER_LAYOUTS, layout)
        q, w, d, p = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        self._ck(self.lib.orl_batch_capacity_after_shape(self._h, src, int(j), lay, int(n_candidates), C.byref(q), C.byref(w), C.byref(d), C.byref(p)))
        return q.value, w.value, d.value, p.value

    def capacity_after(self, source="route", layout="total", j=1, placement="first", candidates=None, fetch=True, out=None):
        """What the network of every env would still carry if the PENDING service went to each of Q candidate placements, in one
        launch on the device: int32 [num_envs, dim].  A candidate is (row, s, n): row = p * C' + c in the row order of the path
        features (path p of the pending service's pair, core c), and the window of slots [s, s + n).  It is present iff 0 <= row <
        k * C', p < n_paths[pair], n >= 1, s >= 0 and s + n <= S.  With A the env's slot maps and A - cand the same maps with the
        window taken on every link of p in core c (free or not),
            after(q)[r] = network_capacity("counts")[:n_cls] evaluated on A - cand_q
        the ordered pairs with paths for which class r is not serviceable; -1 throughout for an absent candidate.  Row Q, one past the
        last candidate, is the baseline on A itself.
        "classes"  reshape(num_envs, Q + 1, n_cls): row q = after(q)
        "total"    [num_envs, Q + 1]: the sum of a row over the classes, -1 for an absent candidate
        Sources of the candidates:
        "route"   the table route_spectrum (RMSA, RWA) or route_cores (RMCSA) last wrote: Q = k * C', candidate q = (q, column 0,
                  column 2) of row q; a row on which nothing fits is absent
        "blocks"  the table block_table(j) last wrote (every family): Q = rows * j, candidate q = r * j + b — the column of the block
                  mask, the index select_blocks decodes — placed at the block's lower ("first") or upper end ("last")
        "given"   `candidates`: an int array [num_envs, Q, 3] of (row, s, n) from the host (not graph-capturable)
        A table that was never written is refused; a stale one is the caller's business.  At most AFTER_MAX_CANDIDATES per env.
        This is NOT the counts of a forked child after its step: a step also runs the releases that fall due before the next
        arrival.  Env state and flags are not touched.  `out` (C-contiguous int32 [num_envs, dim]) receives the rows instead of a
        fresh array.  fetch=False only queues the launch on the batch's stream (graph-capturable after a first call of that source
        and layout) — read the rows in place with device_tensor("capacity_after_classes" / "capacity_after_total") and, say,
        torch.argmin over "total" written into column 0 of device_tensor("actions") before select_blocks(blocks=None)."""
        src = self._named_id("source", self.AFTER_SOURCES, source)
        lay = self._named_id("layout", self.AFTER_LAYOUTS, layout)
        g, nq = None, 0
        if candidates is not None:
            if src != 2:
                raise ValueError("candidates belong to the \"given\" source, not %r" % (source,))
            g = np.asarray(candidates)
            if g.ndim != 3 or g.shape[0] != self.num_envs or g.shape[2] != 3 or g.dtype.kind not in "iu":
                raise ValueError("candidates must be an int array of shape (%d, Q, 3), got %s %r" % (self.num_envs, g.dtype, g.shape))
            g = np.ascontiguousarray(g, np.int32)
            nq = g.shape[1]
        elif src == 2:
            raise ValueError("the \"given\" source needs candidates: an int array [num_envs, Q, 3] of (row, s, n)")
        jj, pl = int(j), self._named_id("placement", self.BLOCK_PLACEMENTS, placement)
        sh = self.capacity_after_shape(src, lay, jj, nq)
        self._keep_given = g  # (alive until the call returns: the library copies it before it does)
        res = self._view_rows(lambda p: self._ck(self.lib.orl_batch_capacity_after(self._h, src, jj, pl, lay, None if g is None else g.ctypes.data, nq, p)),
                              lambda: sh[2], np.int32, fetch, out)
        return res

    def _capacity_after_last(self, layout):
        """(dim, pitch) of the rows the last capacity_after call of `layout` left on the device, as the library holds them"""
        d, p = C.c_int64(), C.c_int64()
        self._ck(self.lib.orl_batch_capacity_after_last(self._h, layout, C.byref(d), C.byref(p)))
        return d.value, p.value

    # ---- zero-copy device views (an agent on the same GPU: no PCIe in the loop) -------------------------
    _BUFFERS = {"actions": (0, "<i4", 4), "reward": (1, "<f8", 0), "done": (2, "|u1", 0), "info": (3, "<f8", -1),
                "obs": (4, "<f8", -2), "terminal_obs": (5, "<f8", -2), "paths": (6, "<i4", 0), "action_mask": (7, "|b1", None),
                "matrix_paths_obs": (8, "|u1", None), "path_features": (9, "<f4", None),
                "link_features": (10, "<f4", None), "assign_table": (11, "<i4", None), "core_table": (12, "<i4", None),
                "block_table": (13, "<i4", None), "block_mask": (14, "|b1", None), "release_horizons": (15, "<f4", None)}
    # the network capacity's rows, one buffer per layout (a table of their own beside the I/O arrays and the pending service's views)
    _CAPACITY_BUFFERS = {"path_capacity": (16, "<i4", None), "serviceable": (17, "|b1", None), "capacity_counts": (18, "<i4", None)}
    # capacity_after's rows, one buffer per layout, at the last call's pitch
    _AFTER_BUFFERS = {"capacity_after_classes": (19, "<i4", None), "capacity_after_total": (20, "<i4", None)}
    # The views of the pending service: [num_envs, dim] rows of the last call at the device pitch.  name -> (the message while no
    # call has been made, (dim, pitch in items) of those rows, item size).  Every mask layout and every j of the path features has
    # a buffer of its own: a view taken after a "joint" call keeps showing the joint rows (as the last "joint" call left them)
    # after "path" calls.
    _VIEWS = {"action_mask": ("no action mask yet: call action_mask() (fetch=False only queues it) first",
                              lambda self: self.action_mask_shape(getattr(self, "_mask_layout", "joint")), 1),
              "matrix_paths_obs": ("no MatrixObservationWithPaths yet: call matrix_observation_with_paths() (fetch=False only "
                                   "queues it) first", lambda self: self.matrix_paths_obs_shape(), 1),
              "path_features": ("no path features yet: call path_features() (fetch=False only queues it) first",
                                lambda self: self.path_features_shape(self._pf_j)[::2], 4),
              "link_features": ("no link features yet: call link_features() (fetch=False only queues it) first",
                                lambda self: self.link_features_shape()[::3], 4),
              "assign_table": ("no assignment table yet: call route_spectrum() (fetch=False only queues it) first",
                               lambda self: (4 * self.assign_table_shape()[0], self.assign_table_shape()[2]), 4),
              "core_table": ("no (path, core) table yet: call route_cores() (fetch=False only queues it) first",
                             lambda self: (4 * self.core_table_shape()[0], self.core_table_shape()[2]), 4),
              "block_table": ("no block table yet: call block_table() (fetch=False only queues it) first",
                              lambda self: (lambda sh: (sh[0] * sh[1], sh[2]))(self.block_table_shape(self._bt_j)), 4),
              "block_mask": ("no block mask yet: call block_table() (fetch=False only queues it) first",
                             lambda self: self.block_table_shape(self._bt_j)[3:], 1),
              "release_horizons": ("no release horizons yet: call release_horizons() (fetch=False only queues it) first",
                                   lambda self: self.release_horizons_shape(*self._rh)[2:], 4),
              "path_capacity": ("no path capacity yet: call network_capacity(\"paths\") (fetch=False only queues it) first",
                                lambda self: self.network_capacity_shape(0)[2:], 4),
              "serviceable": ("no serviceable matrix yet: call network_capacity(\"serviceable\") (fetch=False only queues it) first",
                              lambda self: self.network_capacity_shape(1)[2:], 1),
              "capacity_counts": ("no capacity counts yet: call network_capacity(\"counts\") (fetch=False only queues it) first",
                                  lambda self: self.network_capacity_shape(2)[2:], 4),
              "capacity_after_classes": ("no capacity_after rows yet: call capacity_after(layout=\"classes\") (fetch=False only queues it) first",
                                         lambda self: self._capacity_after_last(0), 4),
              "capacity_after_total": ("no capacity_after totals yet: call capacity_after(layout=\"total\") (fetch=False only queues it) first",
                                       lambda self: self._capacity_after_last(1), 4)}

    def device_array(self, name):
        """The batch's device-resident I/O array `name` as an object with `__cuda_array_interface__` (what
        `torch.as_tensor(x, device="cuda")` and CuPy consume without a copy).  Write actions into "actions", call
        `step(None, fetch=False)`, `sync()`, read "reward" / "done" / "info" / "obs" in place."""
        which, typestr, cols = (self._BUFFERS[name] if name in self._BUFFERS else
                                self._CAPACITY_BUFFERS[name] if name in self._CAPACITY_BUFFERS else self._AFTER_BUFFERS[name])
        ptr, n = C.c_void_p(), C.c_int64()
        self._ck(self.lib.orl_batch_device_buffer(self._h, which, C.byref(ptr), C.byref(n)))
        strides = None
        if name in self._VIEWS:
            not_yet, shape_of, item = self._VIEWS[name]
            if n.value == 0 or not ptr.value:
                raise _lib.OrlError(not_yet)
            cols, pitch = shape_of(self)
            strides = (item * pitch, item)
        cols = {-1: self.n_info, -2: self.obs_dim}.get(cols, cols)
        if n.value == 0 or not ptr.value:
            raise _lib.OrlError("this env family has no '%s' array" % name)
        shape = (self.num_envs, cols) if cols else (self.num_envs,)

        cai = {"shape": shape, "typestr": typestr, "data": (int(ptr.value), False), "version": 2, "strides": strides}
        return _DeviceArray(cai, self.device_id, self)

    def device_tensor(self, name):
        """`device_array(name)` wrapped as a torch tensor on this batch's GPU (no copy)."""
        import torch

        return torch.as_tensor(self.device_array(name), device="cuda:%d" % self.device_id)

    def stream_ptr(self):
        """The HIP stream (an integer hipStream_t) this batch queues its launches on."""
        p = C.c_void_p()
        self._ck(self.lib.orl_batch_stream(self._h, C.byref(p)))
        return int(p.value or 0)

    def torch_stream(self):
        """The batch's stream as a `torch.cuda.ExternalStream`: inside `with torch.cuda.stream(env.torch_stream()):` an agent's
        kernels and `step(None, fetch=False)` are ordered by the stream — no synchronisation between the policy network and
        the step kernel, the host only queues work."""
        import torch

        return torch.cuda.ExternalStream(self.stream_ptr(), device="cuda:%d" % self.device_id)

    def observation(self):
        if not self.obs_dim:
            return None
        self._ck(self.lib.orl_batch_observation(self._h, self._obs.ctypes.data))
        return self._obs

    # ---- state read-back -------------------------------------------------------------------------
    def services(self):
        out = np.zeros((self.num_envs, 6))
        self._ck(self.lib.orl_batch_get_services(self._h, out.ctypes.data))
        return out

    def counters(self):
        out = np.zeros((self.num_envs, 8), np.int64)
        self._ck(self.lib.orl_batch_get_counters(self._h, out.ctypes.data))
        return out

    def slots(self, env=0):
        out = np.zeros((self.num_spatial_resources, self.topology.n_links, self.num_spectrum_resources), np.uint8)
        self._ck(self.lib.orl_batch_get_slots(self._h, env, out.ctypes.data))
        return out

    def spectrum(self, env=0):
        """QoSConstrainedRA: topology.graph["available_spectrum"] (free units per link)."""
        out = np.zeros(self.topology.n_links, np.int32)
        self._ck(self.lib.orl_batch_get_spectrum(self._h, env, out.ctypes.data))
        return out

    def link_stats(self, env=0):
        out = np.zeros((4, self.topology.n_links))
        self._ck(self.lib.orl_batch_get_link_stats(self._h, env, out.ctypes.data))
        return out

    def net_stats(self, env=0):
        out = np.zeros(4)
        self._ck(self.lib.orl_batch_get_net_stats(self._h, env, out.ctypes.data))
        return out

    def slots_packed(self):
        """The slot maps of every env as the device keeps them: [num_envs, map_words] uint64, bit s of word s // 64 of a
        (core, link) row set = slot s free (`orl_batch_row_words` words per row)."""
        out = np.zeros((self.num_envs, self.lib.orl_batch_map_words(self._h)), np.uint64)
        self._ck(self.lib.orl_batch_get_slots_packed(self._h, out.ctypes.data))
        return out

    def link_stats_all(self):
        """[num_envs, 4, links]: utilization, external_fragmentation, compactness, last_update of every link of every env."""
        out = np.zeros((self.num_envs, 4, self.topology.n_links))
        self._ck(self.lib.orl_batch_get_link_stats_all(self._h, out.ctypes.data))
        return out

    def net_stats_all(self):
        """[num_envs, 4]: throughput, compactness, last_update, current_time."""
        out = np.zeros((self.num_envs, 4))
        self._ck(self.lib.orl_batch_get_net_stats_all(self._h, out.ctypes.data))
        return out

    def active(self):
        out = np.zeros(self.num_envs, np.int32)
        self._ck(self.lib.orl_batch_get_active(self._h, out.ctypes.data))
        return out

    def n_active(self, env=0):
        return int(self.active()[env])

    def flags(self):
        out = np.zeros(self.num_envs, np.int32)
        self._ck(self.lib.orl_batch_get_flags(self._h, out.ctypes.data))
        return out

    def action_histograms_of(self, env=0):
        """(actions_output, actions_taken) of env `env` as [k_paths+1, slots+1] int arrays (rmsa_env.py:126-137; RWA's
        arrays are the top-left [k+reject, slots+reject] corner, rwa_env.py:52-58).  Needs action_histograms=True."""
        K1, S1 = self.k_paths + 1, self.num_spectrum_resources + 1
        shape = (2, K1, S1)
        if self.ENV_TYPE == 3:  # RMCSA: [k+1, modulations+1, cores+1, slots+1] (rmcsa_env.py:145-180)
            shape = (2, K1, len(self.modulation_formats) + 1, self.num_spatial_resources + 1, S1)
        out = np.zeros(shape, np.int32)
        self._ck(self.lib.orl_batch_get_action_histograms(self._h, env, out.ctypes.data))
        return out[0].astype(np.int64), out[1].astype(np.int64)

    def pending(self, env=0):
        """The pending releases of env `env` (the reference's `_events` heap, unordered): (release_time[n],
        records[n, 6] = (src*N+dst, path index, initial slot, number of slots, core, bit rate))."""
        n = self.lib.orl_batch_get_pending(self._h, env, 0, None, None)
        if n < 0:
            self._ck(n)
        t = np.zeros(max(n, 1), np.float64)
        rec = np.zeros((max(n, 1), 6), np.int32)
        n2 = self.lib.orl_batch_get_pending(self._h, env, n, t.ctypes.data, rec.ctypes.data)
        if n2 < 0:
            self._ck(n2)
        return t[:n], rec[:n]

    def matrix_observation(self):
        """SimpleMatrixObservation of every env, built on the device: uint8 [num_envs, 2N + C*E*S]."""
        dim = self.lib.orl_batch_matrix_obs_dim(self._h)
        out = np.zeros((self.num_envs, dim), np.uint8)
        self._ck(self.lib.orl_batch_matrix_observation(self._h, out.ctypes.data))
        return out

    def get_state(self):
        """Opaque snapshot of the whole batch (bytes); restore with set_state()."""
        buf = np.zeros(self.lib.orl_batch_state_bytes(self._h), np.uint8)
        self._ck(self.lib.orl_batch_get_state(self._h, buf.ctypes.data))
        return buf

    def set_state(self, buf):
        """Restore a get_state() snapshot of this batch.  The snapshot's size follows what the batch holds — the first seed() of
        a batch adds the second stream of every env — and the library takes no length: a snapshot of another size (taken before
        that seed(), or from a reseeded batch for a fresh one) is refused here with ValueError and nothing is changed."""
        buf = np.ascontiguousarray(buf, np.uint8)
        need = int(self.lib.orl_batch_state_bytes(self._h))
        if buf.size != need:
            raise ValueError("set_state: the snapshot holds %d bytes, this batch's state %d (a seed() between the two adds every "
                             "env's second stream to the state)" % (buf.size, need))
        self._ck(self.lib.orl_batch_set_state(self._h, buf.ctypes.data))

    def state_layout(self):
        """Bytes per env of every section of a get_state() snapshot, in snapshot order: section s occupies num_envs * layout[s]
        bytes, env i at i * layout[s] inside it (include/orl.h, orl_batch_state_layout).  Enough to cut one env out of a snapshot."""
        n = int(self.lib.orl_batch_state_layout(self._h, None, 0))
        if n < 0:
            self._ck(n)
        rows = np.zeros(n, np.int64)
        self._ck(min(int(self.lib.orl_batch_state_layout(self._h, rows.ctypes.data, n)), 0))
        return [int(r) for r in rows]

    def copy_envs(self, src, dst, source=None, keep_rng=False):
        """Fork env states on the device: for every pair, env dst[p] of THIS batch becomes a copy of env src[p] of `source`
        (default: this batch) — every per-env row a snapshot holds, byte for byte, so the copy continues exactly as its source
        does under the same actions or policy.  `src`, `dst`: equally long 1-D integer arrays; a scalar `src` is broadcast to
        len(dst), the fork of one env into many.  One source may feed many destinations.

        keep_rng=True: the destination takes the source's network state, clock, counters, pending service and pending
        releases but keeps its own random streams (and their positions, and whether it was reseeded): an honest lookahead
        child, which has not seen its parent's future arrivals, or a population that does not collapse onto one future.

        What does not travel: the traffic rates, which are configuration exactly as for set_state (`rates()` of both batches
        is unchanged; follow up with set_load(mask=...) to fork across loads); the path column of set_paths and the actions /
        reward / done / info / terminal-observation rows of the last step; the armed episode log; the info mode.  The env's
        flag word travels with its record.  The observation of this batch is rebuilt afterwards.

        Queued on this batch's stream (ordered with `source`'s stream both ways), without waiting for the device.  Refused by
        the library with nothing changed: an index out of range, a destination listed twice, inside one batch a destination
        that is also the source of another pair (src == dst pairs are no-ops; a permutation goes through a scratch batch),
        batches on different devices or of different per-env layout (family, topology, spectrum, cores, j, event capacity,
        bit-rate table, histograms), one batch reseeded and the other not (seed() the other first: an all-zero mask is
        enough), a batch whose last run was abandoned.  ValueError for index arrays of the wrong shape or type."""
        source = self if source is None else source
        if not isinstance(source, BatchedOpticalEnv) or source.lib is not self.lib:
            raise ValueError("copy_envs: source must be a batch of this library")
        d = np.asarray(dst)
        s = np.asarray(src)
        for name, a in (("src", s), ("dst", d)):
            if a.size and a.dtype.kind not in "iu":
                raise ValueError("copy_envs: %s must hold integers, got dtype %s" % (name, a.dtype))
        if d.ndim != 1:
            raise ValueError("copy_envs: dst must be 1-D, got shape %r" % (d.shape,))
        if s.ndim == 0:
            s = np.full(d.shape, s)
        if s.ndim != 1 or s.shape != d.shape:
            raise ValueError("copy_envs: src and dst must be 1-D and equally long, got shapes %r and %r" % (s.shape, d.shape))
        s = np.ascontiguousarray(s, np.int64)
        d = np.ascontiguousarray(d, np.int64)
        self._ck(self.lib.orl_batch_copy_envs(self._h, None if source is self else source._h, len(d), s.ctypes.data, d.ctypes.data,
                                              1 if keep_rng else 0))

    def totals(self):
        p, a = C.c_int64(), C.c_int64()
        self._ck(self.lib.orl_batch_totals(self._h, C.byref(p), C.byref(a)))
        return p.value, a.value


class BatchedRMSAEnv(BatchedOpticalEnv):
    """reference: RMSAEnv (rmsa_env.py:18-744); gym id "RMSA-v0"."""

    ENV_TYPE = 0

    def __init__(self, topology=None, num_envs=1, seeds=None, device_id=0, episode_length=1000, load=10,
                 mean_service_holding_time=10800.0, num_spectrum_resources=100, bit_rate_selection="continuous",
                 bit_rates=(10, 40, 100), bit_rate_probabilities=None, node_request_probabilities=None,
                 bit_rate_lower_bound=25.0, bit_rate_higher_bound=100.0, seed=None, allow_rejection=False,
                 reset=True, channel_width=12.5, event_capacity=0, action_histograms=False, mt_state=None):
        if seeds is None and seed is not None:
            seeds = seed
        self._setup(topology, num_envs, seeds, device_id, episode_length=episode_length, load=load, mt_state=mt_state,
                    mean_service_holding_time=mean_service_holding_time,
                    num_spectrum_resources=num_spectrum_resources, allow_rejection=allow_rejection,
                    node_request_probabilities=node_request_probabilities, channel_width=channel_width,
                    bit_rate_selection=bit_rate_selection, bit_rates=bit_rates,
                    bit_rate_probabilities=bit_rate_probabilities, bit_rate_lower_bound=bit_rate_lower_bound,
                    bit_rate_higher_bound=bit_rate_higher_bound, event_capacity=event_capacity,
                    action_histograms=action_histograms)
        self.info_keys = list(RMSA_INFO_KEYS)
        if bit_rate_selection == "discrete":
            self.info_keys += ["bit_rate_blocking_%s" % b for b in bit_rates] + ["fairness"]


class BatchedDeepRMSAEnv(BatchedOpticalEnv):
    """reference: DeepRMSAEnv (deeprmsa_env.py:9-132); gym id "DeepRMSA-v0"."""

    ENV_TYPE = 1
    N_ACTION = 1

    def __init__(self, topology=None, num_envs=1, seeds=None, device_id=0, j=1, episode_length=1000,
                 mean_service_holding_time=25.0, mean_service_inter_arrival_time=0.1, num_spectrum_resources=100,
                 node_request_probabilities=None, seed=None, allow_rejection=False, event_capacity=0,
                 action_histograms=False, mt_state=None):
        if seeds is None and seed is not None:
            seeds = seed
        mht_v = per_env_values(mean_service_holding_time, num_envs, "mean_service_holding_time")
        miat_v = per_env_values(mean_service_inter_arrival_time, num_envs, "mean_service_inter_arrival_time")
        if mht_v is None and miat_v is None:
            load = mean_service_holding_time / mean_service_inter_arrival_time  # deeprmsa_env.py:25
        else:  # the same division per env, in Python floats
            h = mht_v if mht_v is not None else [_check_scalar(mean_service_holding_time, "mean_service_holding_time")] * int(num_envs)
            a = miat_v if miat_v is not None else [_check_scalar(mean_service_inter_arrival_time, "mean_service_inter_arrival_time")] * int(num_envs)
            load = [float(h[i]) / float(a[i]) for i in range(int(num_envs))]
        self._setup(topology, num_envs, seeds, device_id, episode_length=episode_length,
                    load=load, mt_state=mt_state,
                    mean_service_holding_time=mean_service_holding_time,
                    num_spectrum_resources=num_spectrum_resources, allow_rejection=allow_rejection,
                    node_request_probabilities=node_request_probabilities, channel_width=12.5, j=j,
                    event_capacity=event_capacity, action_histograms=action_histograms)
        self.info_keys = list(RMSA_INFO_KEYS)


class BatchedRWAEnv(BatchedOpticalEnv):
    """reference: RWAEnv (rwa_env.py:15-400); gym id "RWA-v0"."""

    ENV_TYPE = 2

    def __init__(self, topology=None, num_envs=1, seeds=None, device_id=0, episode_length=1000, load=10,
                 mean_service_holding_time=10800.0, num_spectrum_resources=80, node_request_probabilities=None,
                 allow_rejection=True, seed=None, reset=True, channel_width=50.0, event_capacity=0,
                 action_histograms=False, mt_state=None):
        if seeds is None and seed is not None:
            seeds = seed
        self._setup(topology, num_envs, seeds, device_id, episode_length=episode_length, load=load, mt_state=mt_state,
                    mean_service_holding_time=mean_service_holding_time,
                    num_spectrum_resources=num_spectrum_resources, allow_rejection=allow_rejection,
                    node_request_probabilities=node_request_probabilities, channel_width=channel_width,
                    event_capacity=event_capacity, action_histograms=action_histograms)
        rej = self.reject_action
        self.info_keys = (["service_blocking_rate", "episode_service_blocking_rate"]
                          + ["path_action_probability[%d]" % i for i in range(self.k_paths + rej)]
                          + ["wavelength_action_probability[%d]" % i for i in range(num_spectrum_resources + rej)])


class BatchedRMCSAEnv(BatchedOpticalEnv):
    """reference: RMCSAEnv (rmcsa_env.py:18-879); gym id "RMCSA-v0"."""

    ENV_TYPE = 3
    N_ACTION = 4

    def __init__(self, topology=None, num_envs=1, seeds=None, device_id=0, episode_length=1000, load=10,
                 mean_service_holding_time=10800.0, num_spectrum_resources=100, num_spatial_resources=7,
                 modulation_formats=None, worst_xt=None, node_request_probabilities=None,
                 bit_rate_selection="continuous", bit_rates=(10, 40, 100), bit_rate_probabilities=None,
                 bit_rate_lower_bound=25, bit_rate_higher_bound=100, seed=None, allow_rejection=False, reset=True,
                 channel_width=12.5, event_capacity=0, action_histograms=False, mt_state=None):
        import copy

        if seeds is None and seed is not None:
            seeds = seed
        topo = Topology.load(topology) if isinstance(topology, str) else topology
        mods = copy.deepcopy(list(topo.modulations if modulation_formats is None else modulation_formats))
        if worst_xt is None:  # rmcsa_env.py:63-67, 119-122
            worst_xt = {7: -84.7, 12: -61.9, 19: -54.8}.get(num_spatial_resources)
        for m in mods:  # rmcsa_env.py:127-129: +4 dB margin on both limits
            m.inband_xt += 4
        worst_xt += 4
        self._setup(topo, num_envs, seeds, device_id, episode_length=episode_length, load=load, mt_state=mt_state,
                    mean_service_holding_time=mean_service_holding_time,
                    num_spectrum_resources=num_spectrum_resources, allow_rejection=allow_rejection,
                    node_request_probabilities=node_request_probabilities, channel_width=channel_width,
                    bit_rate_selection=bit_rate_selection, bit_rates=bit_rates,
                    bit_rate_probabilities=bit_rate_probabilities, bit_rate_lower_bound=bit_rate_lower_bound,
                    bit_rate_higher_bound=bit_rate_higher_bound, num_spatial_resources=num_spatial_resources,
                    modulations=mods, worst_xt=worst_xt, event_capacity=event_capacity, action_histograms=action_histograms)
        self.info_keys = RMSA_INFO_KEYS[:4]


class BatchedQoSConstrainedRA(BatchedOpticalEnv):
    """reference: QoSConstrainedRA (qos_constrained_ra.py:13-398); gym id "QoSConstrainedRA-v0".  Upstream its constructor
    raises (an unexpected `k_paths` keyword for the base class, :32-41, and a `service_class` field utils.Service lacks);
    the semantics here are the class's as written, pinned by fixtures captured from the reference with those two things
    repaired at import time (oracle/gen_golden_qos.py).  Actions: the path index; the service class of the pending service
    is column 4 of services()."""

    ENV_TYPE = 4
    N_ACTION = 1

    def __init__(self, topology=None, num_envs=1, seeds=None, device_id=0, episode_length=1000, load=10,
                 mean_service_holding_time=10800.0, num_spectrum_resources=80, num_service_classes=1,
                 classes_arrival_probabilities=(1.0,), classes_reward=(1.0,), node_request_probabilities=None,
                 allow_rejection=True, k_paths=5, seed=None, reset=True, event_capacity=0, mt_state=None):
        if seeds is None and seed is not None:
            seeds = seed
        self._setup(topology, num_envs, seeds, device_id, episode_length=episode_length, load=load, mt_state=mt_state,
                    mean_service_holding_time=mean_service_holding_time,
                    num_spectrum_resources=num_spectrum_resources, allow_rejection=allow_rejection,
                    node_request_probabilities=node_request_probabilities, channel_width=12.5,
                    event_capacity=event_capacity, num_service_classes=num_service_classes,
                    classes_arrival_probabilities=classes_arrival_probabilities, classes_reward=classes_reward)
        self.info_keys = ["service_blocking_rate", "episode_service_blocking_rate"]


ENV_CLASSES = {"RMSA": BatchedRMSAEnv, "DeepRMSA": BatchedDeepRMSAEnv, "RWA": BatchedRWAEnv, "RMCSA": BatchedRMCSAEnv,
               "RMSA-v0": BatchedRMSAEnv, "DeepRMSA-v0": BatchedDeepRMSAEnv, "RWA-v0": BatchedRWAEnv,
               "RMCSA-v0": BatchedRMCSAEnv, "QoSConstrainedRA": BatchedQoSConstrainedRA,
               "QoSConstrainedRA-v0": BatchedQoSConstrainedRA}


def make(env_id, device_ids=None, **kwargs):
    """Batch constructor by registry id (optical_rl_gym/__init__.py:3-26).  `device_ids=[0, 1, ...]` spreads the envs over
    several GPUs of the node behind one object (sharding.MultiDeviceBatch); default: one batch on `device_id`."""
    if device_ids is not None and len(device_ids) > 1:
        from .sharding import MultiDeviceBatch

        kwargs.pop("device_id", None)
        return MultiDeviceBatch(env_id, kwargs.pop("num_envs"), seeds=kwargs.pop("seeds", None), device_ids=device_ids, **kwargs)
    if device_ids is not None and len(device_ids) == 1:
        kwargs["device_id"] = int(device_ids[0])
    return ENV_CLASSES[env_id](**kwargs)
