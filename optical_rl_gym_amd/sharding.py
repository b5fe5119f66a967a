"""Multi-GPU: contiguous blocks of env indices per device, no data-path collective.

Envs are independent, so env i's trajectory depends only on seeds[i] and its action stream: the number of GPUs (and how
the batch is cut) never changes a result.  Two ways to use several GPUs of a node:

  * one process per GPU (bench.py --gpus N under torchrun): rank r builds the batch for global env indices
    [lo, hi) = shard_range(total, r, world) with seeds base + index;
  * one process, `MultiDeviceBatch(..., device_ids=[0, 1, ...])`: one batch per device behind the interface of a single
    batch — actions are scattered and rewards / dones / infos / observations gathered per shard, each shard driven by its
    own host thread on its own stream (the library calls release the GIL), so one VecEnv / one agent process can drive all
    GPUs.  The SURVEY's `n_devices, device_ids` arguments of the batch constructor live here, above the C ABI, because a
    handle of the ABI is bound to one device.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np


def shard_range(n_envs_total, rank, world):
    """Contiguous, balanced partition of range(n_envs_total)."""
    per, rem = divmod(n_envs_total, world)
    lo = rank * per + min(rank, rem)
    hi = lo + per + (1 if rank < rem else 0)
    return lo, hi


def shard_seeds(base_seed, n_envs_total, rank, world):
    lo, hi = shard_range(n_envs_total, rank, world)
    return [base_seed + i for i in range(lo, hi)]


def cut_per_env_kwargs(kwargs, names, num_envs, lo, hi):
    """`kwargs` for the shard that holds envs [lo, hi) of num_envs: the arguments `names` that carry one value per env (anything
    but a scalar) are cut to the shard's envs, everything else is passed on as it is.  ValueError for a wrong length."""
    out = dict(kwargs)
    for name in names:
        v = kwargs.get(name)
        if v is None or np.isscalar(v):
            continue
        a = np.asarray(v, np.float64)
        if a.ndim == 0:
            continue
        if a.ndim != 1 or a.shape[0] != num_envs:
            raise ValueError("%s must be a scalar or one value per env (length %d), got shape %r" % (name, num_envs, a.shape))
        out[name] = a[lo:hi]
    return out


class MultiRunStats:
    """RunStats of a run over several shards (see MultiDeviceBatch.run)."""

    def __init__(self, parts):
        self.shards = list(parts)
        get = lambda p, name: getattr(p, name, 0) or 0  # (shards need not be HIP batches: from_shards takes any batch object)
        self.ms_total = max(float(get(p, "ms_total")) for p in parts)
        self.ms_policy = max(float(get(p, "ms_policy")) for p in parts)
        self.ms_step = max(float(get(p, "ms_step")) for p in parts)
        self.launches = sum(int(get(p, "launches")) for p in parts)
        self.n_kernels = int(get(parts[0], "n_kernels"))

    def kernels(self):
        if not hasattr(self.shards[0], "kernels"):
            return []
        first = self.shards[0].kernels()
        return [(name, max(p.kernels()[i][1] for p in self.shards)) for i, (name, _) in enumerate(first)]


class MultiDeviceBatch:
    """`num_envs` envs spread over `device_ids` (contiguous shards), with the methods of `BatchedOpticalEnv`."""

    PER_ENV_KWARGS = ("load", "mean_service_holding_time", "mean_service_inter_arrival_time")

    def __init__(self, env_id, num_envs, seeds=None, device_ids=(0,), mt_state=None, **kwargs):
        from .envs import ENV_CLASSES

        if mt_state is not None:  # the generators' states instead of seeds ([num_envs][625] uint32): each shard gets its rows
            if seeds is not None:
                raise ValueError("seeds or mt_state, not both")
            mt_state = np.ascontiguousarray(mt_state, np.uint32)
            if mt_state.shape != (num_envs, 625):
                raise ValueError("mt_state must be [num_envs][625] uint32")
        if mt_state is not None:
            seeds = None
        elif seeds is None:
            seeds = [None] * num_envs
        elif np.isscalar(seeds):
            seeds = [int(seeds) + i for i in range(num_envs)]
        shards = []
        for r, dev in enumerate(device_ids):
            lo, hi = shard_range(num_envs, r, len(device_ids))
            kw = cut_per_env_kwargs(kwargs, self.PER_ENV_KWARGS, num_envs, lo, hi)
            if mt_state is not None:
                shards.append(ENV_CLASSES[env_id](num_envs=hi - lo, mt_state=mt_state[lo:hi], device_id=int(dev), **kw))
            else:
                shards.append(ENV_CLASSES[env_id](num_envs=hi - lo, seeds=list(seeds[lo:hi]), device_id=int(dev), **kw))
        self._init_from(shards)

    @classmethod
    def from_shards(cls, shards):
        """Wrap existing batches (any objects with the batch interface), in env-index order."""
        self = cls.__new__(cls)
        self._init_from(list(shards))
        return self

    def _init_from(self, shards):
        self.shards = shards
        self.bounds = np.cumsum([0] + [s.num_envs for s in shards])
        self.num_envs = int(self.bounds[-1])
        self._pool = ThreadPoolExecutor(max_workers=len(shards))
        first = shards[0]
        for name in ("topology", "info_keys", "obs_dim", "n_info", "ENV_TYPE", "N_ACTION", "episode_length", "allow_rejection",
                     "k_paths", "num_spectrum_resources", "num_spatial_resources", "j", "modulation_formats", "reject_action"):
            if hasattr(first, name):
                setattr(self, name, getattr(first, name))

    # ---- helpers ----
    def _map(self, fn):
        return list(self._pool.map(fn, range(len(self.shards))))

    def _cut(self, arr, r):
        return None if arr is None else np.asarray(arr)[self.bounds[r]:self.bounds[r + 1]]

    def _owner(self, env):
        r = int(np.searchsorted(self.bounds, env, side="right") - 1)
        return self.shards[r], int(env - self.bounds[r])

    @staticmethod
    def _cat(parts):
        return None if parts[0] is None else np.concatenate(parts, axis=0)

    # ---- the batch interface ----
    def reset(self, full=False, mask=None):
        return self._cat(self._map(lambda r: self.shards[r].reset(full=full, mask=self._cut(mask, r))))

    def seed(self, seeds, mask=None):
        if np.isscalar(seeds):
            seeds = [int(seeds) + i for i in range(self.num_envs)]
        self._map(lambda r: self.shards[r].seed(list(seeds[self.bounds[r]:self.bounds[r + 1]]), mask=self._cut(mask, r)))

    def set_load(self, load=None, mean_service_holding_time=None, mask=None):
        """set_load of every shard's envs (BatchedOpticalEnv.set_load): per-env arguments and the mask are cut per shard.  Every
        shard's slice is checked before any shard is changed: the arguments on the host (ValueError), and the resulting rates
        against each shard's pending-release capacity through a call that selects no env (the library validates nothing for
        unselected envs, so the loads are checked here with its formula).  What remains is a refusal only the library can give
        — a shard whose last device-resident run did not complete — which leaves the shards before it changed; the error says
        which shard."""
        n = self.num_envs

        def part(v, r, name):
            if v is None or np.isscalar(v):
                return v
            a = np.asarray(v, np.float64)
            if a.ndim != 1 or a.shape[0] != n:
                raise ValueError("%s must be a scalar or one value per env (length %d), got shape %r" % (name, n, a.shape))
            return a[self.bounds[r]:self.bounds[r + 1]]

        if mask is not None and np.asarray(mask).shape != (n,):
            raise ValueError("mask must have one entry per env (length %d)" % n)
        args = [(part(load, r, "load"), part(mean_service_holding_time, r, "mean_service_holding_time"), self._cut(mask, r))
                for r in range(len(self.shards))]
        for r, (sh, (ld, mht, m)) in enumerate(zip(self.shards, args)):
            if hasattr(sh, "_derive_set_load"):
                _l, _h, _i, lam_a, lam_h, mm = sh._derive_set_load(ld, mht, m)
                if hasattr(sh, "event_capacity_in_force"):
                    sel = np.ones(sh.num_envs, bool) if mm is None else mm != 0
                    need = [sh.capacity_needed(a / h) for a, h in zip(lam_a[sel], lam_h[sel])]
                    if need and max(need) > sh.event_capacity_in_force():
                        raise ValueError("shard %d: a load of its envs needs an event_capacity of %d, the shard was created with %d"
                                         % (r, max(need), sh.event_capacity_in_force()))

        def one(r):
            try:
                self.shards[r].set_load(load=args[r][0], mean_service_holding_time=args[r][1], mask=args[r][2])
            except Exception as exc:
                raise type(exc)("shard %d (envs %d..%d): %s" % (r, self.bounds[r], self.bounds[r + 1] - 1, exc)) from None

        for r in range(len(self.shards)):  # in order: a refusal of shard r leaves shards r.. untouched
            one(r)

    def rates(self):
        out = self._map(lambda r: self.shards[r].rates())
        return self._cat([o[0] for o in out]), self._cat([o[1] for o in out])

    def _per_env_attr(self, name):
        vals = [getattr(s, name) for s in self.shards]
        if all(np.isscalar(v) for v in vals) and all(v == vals[0] for v in vals):
            return vals[0]
        return np.concatenate([np.full(s.num_envs, v, np.float64) if np.isscalar(v) else np.asarray(v, np.float64)
                               for s, v in zip(self.shards, vals)])

    @property
    def load(self):
        return self._per_env_attr("load")

    @property
    def mean_service_holding_time(self):
        return self._per_env_attr("mean_service_holding_time")

    @property
    def mean_service_inter_arrival_time(self):
        return self._per_env_attr("mean_service_inter_arrival_time")

    def set_info_mode(self, rates_only):
        # (shards without the switch — the oracle stand-in of the CPU tests — always write every entry)
        self._map(lambda r: self.shards[r].set_info_mode(rates_only) if hasattr(self.shards[r], "set_info_mode") else None)

    def set_paths(self, paths):
        self._map(lambda r: self.shards[r].set_paths(self._cut(paths, r)))

    def policy(self, policy, fetch=True, paths=None):
        out = self._map(lambda r: self.shards[r].policy(policy, fetch=fetch, paths=self._cut(paths, r)))
        return self._cat(out) if fetch else None

    def step(self, actions, auto_reset=False, fetch=True, obs_out=None, fetch_info=True):
        """As a single batch's step().  `obs_out` (a caller-owned [num_envs, obs_dim] array: every shard writes its rows) and
        `fetch_info=False` (info stays on the devices, `info_rows` reads what is needed) are handed to shards that take them —
        the HIP batches — and emulated for others (the oracle stand-in of the CPU tests)."""
        import inspect

        for r, sh in enumerate(self.shards):  # (refused before anything is modified on any shard, like a single batch's step)
            if hasattr(sh, "validate_actions"):
                sh.validate_actions(self._cut(actions, r))

        def one(r):
            sh = self.shards[r]
            params = inspect.signature(sh.step).parameters
            kw = {}
            if fetch and obs_out is not None and "obs_out" in params:
                kw["obs_out"] = obs_out[self.bounds[r]:self.bounds[r + 1]]
            if fetch and not fetch_info and "fetch_info" in params:
                kw["fetch_info"] = False
            out = sh.step(self._cut(actions, r), auto_reset=auto_reset, fetch=fetch, **kw)
            if fetch and obs_out is not None and "obs_out" not in kw and out[0] is not None:
                obs_out[self.bounds[r]:self.bounds[r + 1]] = out[0]
            return out

        out = self._map(one)
        if not fetch:
            return None
        infos = [o[3] for o in out]
        self._info_parts = infos  # (a shard that ignored fetch_info=False returned its array: info_rows reads from it)
        self._info = None if any(i is None for i in infos) else self._cat(infos)
        obs = obs_out if (obs_out is not None and getattr(self, "obs_dim", 0)) else self._cat([o[0] for o in out])
        return obs, self._cat([o[1] for o in out]), self._cat([o[2] for o in out]), (self._info if fetch_info else None)

    def policy_step(self, policy, auto_reset=False, fetch=True, paths=None):
        """policy() and step() on its actions in one launch per shard (BatchedOpticalEnv.policy_step)."""
        out = self._map(lambda r: self.shards[r].policy_step(policy, auto_reset=auto_reset, fetch=fetch, paths=self._cut(paths, r)))
        if not fetch:
            return None
        return tuple(self._cat([o[k] for o in out]) for k in range(5))

    def step_async(self, actions, auto_reset=False, obs_out=None, fetch_info=True):
        """First half of step() on every shard (`BatchedOpticalEnv.step_async`): each device gets its slice of the actions and its
        step queued on its own stream, one shard after the other from this thread — the calls only queue work, so all devices run
        at once without host threads — and `step_wait()` collects them.  Shards without the two halves (the oracle stand-in of the
        CPU tests) step synchronously here."""
        # every shard's slice is checked BEFORE a step is queued on any of them: an action outside the action space is refused
        # with nothing modified anywhere (include/orl.h), not with shards 0..r-1 stepped and their steps left pending
        for r, sh in enumerate(self.shards):
            if hasattr(sh, "validate_actions"):
                try:
                    sh.validate_actions(self._cut(actions, r))
                except IndexError as exc:
                    raise IndexError("shard %d (envs %d..%d): %s" % (r, self.bounds[r], self.bounds[r + 1] - 1, exc)) from None
        self._async_obs = obs_out
        self._async_sync = {}
        queued = []
        try:
            for r, sh in enumerate(self.shards):
                a = self._cut(actions, r)
                oo = None if obs_out is None else obs_out[self.bounds[r]:self.bounds[r + 1]]
                if hasattr(sh, "step_async"):
                    sh.step_async(a, auto_reset=auto_reset, obs_out=oo, fetch_info=fetch_info)
                    queued.append(sh)
                else:
                    out = sh.step(a, auto_reset=auto_reset)
                    if oo is not None and out[0] is not None:
                        oo[:] = out[0]
                    self._async_sync[r] = out
        except Exception:
            # (a device error on one shard: the steps already queued are collected, so that no shard is left with a pending step;
            # the batch is no longer consistent — the earlier shards are one step ahead — and the error says so)
            for sh in queued:
                try:
                    sh.step_wait()
                except Exception:
                    pass
            raise

    def step_wait(self):
        out = [self._async_sync[r] if r in self._async_sync else sh.step_wait() for r, sh in enumerate(self.shards)]
        infos = [o[3] for o in out]
        self._info_parts = infos
        self._info = None if any(i is None for i in infos) else self._cat(infos)
        obs = self._async_obs if (self._async_obs is not None and getattr(self, "obs_dim", 0)) else self._cat([o[0] for o in out])
        return obs, self._cat([o[1] for o in out]), self._cat([o[2] for o in out]), self._info

    def info_rows(self, indices):
        """Rows `indices` of the info arrays the last step left on the devices, in the order asked for."""
        idx = np.asarray(indices, np.int64).reshape(-1)
        out = np.empty((len(idx), self.n_info), np.float64)
        owner = np.searchsorted(self.bounds, idx, side="right") - 1
        for r in np.unique(owner):
            sel = np.flatnonzero(owner == r)
            local = idx[sel] - self.bounds[r]
            part = getattr(self, "_info_parts", [None] * len(self.shards))[r]
            out[sel] = part[local] if part is not None else self.shards[r].info_rows(local)
        return out

    def host_array(self, shape, dtype):
        """Page-locked host memory when the shards offer it (copies from every device then run at the full PCIe rate)."""
        first = self.shards[0]
        return first.host_array(shape, dtype) if hasattr(first, "host_array") else np.zeros(shape, dtype)

    def run(self, policy, n_steps, time_kernels=False):
        """Every shard runs its own device-resident loop concurrently.  Returns ONE stats object with the fields of a single
        batch's RunStats — the shards run side by side, so times are the MAX over shards and launches the sum — plus
        `.shards`, the per-shard RunStats in env-index order."""
        parts = self._map(lambda r: self.shards[r].run(policy, n_steps, time_kernels))
        return MultiRunStats(parts)

    def evaluate(self, policy, n_eval_episodes=10):
        out = self._map(lambda r: self.shards[r].evaluate(policy, n_eval_episodes))
        return self._cat([o[0] for o in out]), self._cat([o[1] for o in out])

    def observation(self):
        return self._cat(self._map(lambda r: self.shards[r].observation()))

    def matrix_observation(self):
        return self._cat(self._map(lambda r: self.shards[r].matrix_observation()))

    def _view_rows(self, call, fetch, out=None):
        """One view of every shard — `call(r, **kw)` is shard r's method: the rows in env order, with `out` ([num_envs, dim],
        C-contiguous) every shard writing its own slice of it; fetch=False only queues."""
        if out is None or not fetch:
            parts = self._map(lambda r: call(r, fetch=fetch))
            return self._cat(parts) if fetch else None
        self._map(lambda r: call(r, out=out[self.bounds[r]:self.bounds[r + 1]]))
        return out

    def action_mask(self, layout="joint", fetch=True, given=None):
        """BatchedOpticalEnv.action_mask of every shard; `given` ([num_envs, 2], "core_slot") is cut by the shards' bounds."""
        if given is None:  # (shards may be any objects with the batch interface: the argument is passed only where it is used)
            return self._view_rows(lambda r, **kw: self.shards[r].action_mask(layout, **kw), fetch)
        given = np.asarray(given)
        if given.shape != (self.num_envs, 2):
            raise ValueError("given must be an int array of shape %r, got %r" % ((self.num_envs, 2), given.shape))
        return self._view_rows(lambda r, **kw: self.shards[r].action_mask(layout, given=self._cut(given, r), **kw), fetch)

    def complete_actions(self, given=None, n_given=None, fetch=True):
        """BatchedOpticalEnv.complete_actions of every shard; `given` ([num_envs, g] or [num_envs]) is cut by the shards' bounds."""
        from .envs import BatchedOpticalEnv

        g, n = BatchedOpticalEnv.completion_prefix(given, n_given, self.num_envs)
        out = self._map(lambda r: self.shards[r].complete_actions(given=self._cut(g, r), n_given=n, fetch=fetch))
        return self._cat(out) if fetch else None

    def assign_spectrum(self, rule="first", paths=None, n_given=None, fetch=True):
        """BatchedOpticalEnv.assign_spectrum of every shard; `paths` ([num_envs]) is cut by the shards' bounds."""
        from .envs import BatchedOpticalEnv

        p, n = BatchedOpticalEnv.assignment_paths(paths, n_given, self.num_envs)
        out = self._map(lambda r: self.shards[r].assign_spectrum(rule, paths=self._cut(p, r), n_given=n, fetch=fetch))
        return self._cat(out) if fetch else None

    def route_spectrum(self, rule="first", route="best", fetch=True, table=False):
        """BatchedOpticalEnv.route_spectrum of every shard; the shards' action rows (and table rows) concatenated."""
        out = self._map(lambda r: self.shards[r].route_spectrum(rule, route, fetch=fetch, table=table))
        if not fetch:
            return None
        return (self._cat([o[0] for o in out]), self._cat([o[1] for o in out])) if table else self._cat(out)

    def assign_table_shape(self):
        return self.shards[0].assign_table_shape()

    def route_cores(self, rule="first", route="best", paths=None, cores=None, n_given=None, modulation=None, fetch=True, table=False):
        """BatchedOpticalEnv.route_cores of every shard; `paths` and `cores` ([num_envs]) are cut by the shards' bounds, the shards'
        action rows (and table rows) concatenated."""
        from .envs import BatchedOpticalEnv

        g, n = BatchedOpticalEnv.core_prefix(paths, cores, n_given, self.num_envs)
        col = lambda r, i: None if g is None or g.shape[1] <= i else self._cut(np.ascontiguousarray(g[:, i]), r)
        out = self._map(lambda r: self.shards[r].route_cores(rule, route, paths=col(r, 0), cores=col(r, 1), n_given=n, modulation=modulation,
                                                             fetch=fetch, table=table))
        if not fetch:
            return None
        return (self._cat([o[0] for o in out]), self._cat([o[1] for o in out])) if table else self._cat(out)

    def core_table_shape(self):
        return self.shards[0].core_table_shape()

    def block_table_shape(self, j=1):
        return self.shards[0].block_table_shape(j)

    def block_table(self, j=1, modulation=None, fetch=True):
        """BatchedOpticalEnv.block_table of every shard; the shards' table rows and mask rows concatenated."""
        out = self._map(lambda r: self.shards[r].block_table(j, modulation, fetch=fetch))
        return (self._cat([o[0] for o in out]), self._cat([o[1] for o in out])) if fetch else None

    def select_blocks(self, blocks=None, j=1, modulation=None, placement="first", fetch=True):
        """BatchedOpticalEnv.select_blocks of every shard; `blocks` ([num_envs]) is cut by the shards' bounds."""
        from .envs import BatchedOpticalEnv

        a = BatchedOpticalEnv.block_indices(blocks, self.num_envs)
        out = self._map(lambda r: self.shards[r].select_blocks(self._cut(a, r), j, modulation, placement, fetch=fetch))
        return self._cat(out) if fetch else None

    def path_features_shape(self, j=1):
        return self.shards[0].path_features_shape(j)

    def path_features(self, j=1, modulation=None, fetch=True, out=None):
        """BatchedOpticalEnv.path_features of every shard, rows in env order; with `out` ([num_envs, dim] float32, C-contiguous)
        every shard writes its own rows."""
        return self._view_rows(lambda r, **kw: self.shards[r].path_features(j, modulation, **kw), fetch, out)

    def release_horizons_shape(self, layout="slots", j=1):
        return self.shards[0].release_horizons_shape(layout, j)

    def release_horizons(self, layout="slots", j=1, modulation=None, fetch=True, out=None):
        """BatchedOpticalEnv.release_horizons of every shard, rows in env order; with `out` ([num_envs, dim] float32, C-contiguous)
        every shard writes its own rows."""
        return self._view_rows(lambda r, **kw: self.shards[r].release_horizons(layout, j, modulation, **kw), fetch, out)

    def network_capacity_shape(self, layout="paths"):
        return self.shards[0].network_capacity_shape(layout)

    def network_capacity(self, layout="paths", fetch=True, out=None):
        """BatchedOpticalEnv.network_capacity of every shard, rows in env order; with `out` ([num_envs, dim] of the layout's type,
        C-contiguous) every shard writes its own rows."""
        return self._view_rows(lambda r, **kw: self.shards[r].network_capacity(layout, **kw), fetch, out)

    def capacity_after_shape(self, source="route", layout="total", j=1, n_candidates=0):
        return self.shards[0].capacity_after_shape(source, layout, j, n_candidates)

    def capacity_after(self, source="route", layout="total", j=1, placement="first", candidates=None, fetch=True, out=None):
        """BatchedOpticalEnv.capacity_after of every shard, rows in env order; `candidates` ([num_envs, Q, 3]) is split by env; with
        `out` (int32 [num_envs, dim], C-contiguous) every shard writes its own rows."""
        cand = None if candidates is None else np.asarray(candidates)
        if cand is not None and (cand.ndim != 3 or cand.shape[0] != self.num_envs):
            raise ValueError("candidates must be an int array of shape (%d, Q, 3), got %r" % (self.num_envs, cand.shape))
        return self._view_rows(lambda r, **kw: self.shards[r].capacity_after(
            source, layout, j, placement, None if cand is None else self._cut(cand, r), **kw), fetch, out)

    def link_features_shape(self):
        return self.shards[0].link_features_shape()

    def link_features(self, fetch=True, out=None):
        """BatchedOpticalEnv.link_features of every shard, rows in env order; with `out` ([num_envs, dim] float32, C-contiguous)
        every shard writes its own rows."""
        return self._view_rows(lambda r, **kw: self.shards[r].link_features(**kw), fetch, out)

    def matrix_paths_obs_shape(self):
        return self.shards[0].matrix_paths_obs_shape()

    def matrix_observation_with_paths(self, fetch=True, out=None):
        """The shards' rows in env order; with `out` ([num_envs, dim] uint8, C-contiguous) every shard writes its own rows."""
        return self._view_rows(lambda r, **kw: self.shards[r].matrix_observation_with_paths(**kw), fetch, out)

    def copy_envs(self, src, dst, keep_rng=False):
        """BatchedOpticalEnv.copy_envs with global env indices, inside this sharded batch.  The pairs are cut by the shards that own
        them: a pair inside one shard is an in-place copy of that shard, a pair between two shards on one device a copy between
        two batches.  Copies between GPUs are not supported: a pair whose shards sit on different devices raises ValueError
        naming it, and every pair is checked — range and devices — before any shard queues anything.  (The
        in-place rule of a single batch holds for the whole sharded batch: no env is a destination and the source of another pair.)"""
        d = np.asarray(dst)
        s = np.asarray(src)
        if d.ndim != 1:
            raise ValueError("copy_envs: dst must be 1-D, got shape %r" % (d.shape,))
        if s.ndim == 0:
            s = np.full(d.shape, s)
        if s.ndim != 1 or s.shape != d.shape:
            raise ValueError("copy_envs: src and dst must be 1-D and equally long, got shapes %r and %r" % (s.shape, d.shape))
        for name, a in (("src", s), ("dst", d)):
            if a.size and a.dtype.kind not in "iu":
                raise ValueError("copy_envs: %s must hold integers, got dtype %s" % (name, a.dtype))
        s, d = s.astype(np.int64), d.astype(np.int64)
        for name, a in (("source", s), ("destination", d)):
            bad = np.flatnonzero((a < 0) | (a >= self.num_envs))
            if bad.size:
                raise ValueError("copy_envs: pair %d: %s index %d outside [0, %d)" % (bad[0], name, a[bad[0]], self.num_envs))
        if len(np.unique(d)) != len(d):
            raise ValueError("copy_envs: a destination index occurs twice")
        moved = s != d  # (src == dst pairs are no-ops, as in a single batch)
        s, d = s[moved], d[moved]
        both = np.intersect1d(s, d)
        if both.size:  # (the rule of a single batch, for the whole sharded one: the shards' copies are not ordered with each other)
            raise ValueError("copy_envs: env %d is the destination of one pair and the source of another; go through a scratch batch"
                             % both[0])
        rs = np.searchsorted(self.bounds, s, side="right") - 1
        rd = np.searchsorted(self.bounds, d, side="right") - 1
        dev = [getattr(sh, "device_id", 0) for sh in self.shards]
        for p in range(len(d)):
            if dev[rs[p]] != dev[rd[p]]:
                raise ValueError("copy_envs: pair %d (%d -> %d) crosses devices (shard %d on device %d, shard %d on device %d): "
                                 "copies between GPUs are not supported" % (p, s[p], d[p], rs[p], dev[rs[p]], rd[p], dev[rd[p]]))
        for a in np.unique(rs):
            for b in np.unique(rd[rs == a]):
                sel = (rs == a) & (rd == b)
                self.shards[b].copy_envs(s[sel] - self.bounds[a], d[sel] - self.bounds[b],
                                         source=None if a == b else self.shards[a], keep_rng=keep_rng)

    def sync(self):
        self._map(lambda r: self.shards[r].sync())

    def check(self):
        self._map(lambda r: self.shards[r].check())

    def counters(self):
        return self._cat(self._map(lambda r: self.shards[r].counters()))

    def services(self):
        return self._cat(self._map(lambda r: self.shards[r].services()))

    def active(self):
        return self._cat(self._map(lambda r: self.shards[r].active()))

    def flags(self):
        return self._cat(self._map(lambda r: self.shards[r].flags()))

    def totals(self):
        t = self._map(lambda r: self.shards[r].totals())
        return sum(x[0] for x in t), sum(x[1] for x in t)

    def slots(self, env=0):
        s, i = self._owner(env)
        return s.slots(i)

    def link_stats(self, env=0):
        s, i = self._owner(env)
        return s.link_stats(i)

    def net_stats(self, env=0):
        s, i = self._owner(env)
        return s.net_stats(i)

    def n_active(self, env=0):
        s, i = self._owner(env)
        return s.n_active(i)

    def action_histograms_of(self, env=0):
        s, i = self._owner(env)
        return s.action_histograms_of(i)

    def pending(self, env=0):
        s, i = self._owner(env)
        return s.pending(i)

    def device_tensor(self, name):
        """Per-shard zero-copy device tensors (one per GPU), in env-index order."""
        return [s.device_tensor(name) for s in self.shards]

    def close(self):
        for s in self.shards:
            s.close()
        self._pool.shutdown(wait=False)
