/*
 * orl.h — C ABI of liborlgpu.so: batched optical-network RL environments on MI355X (gfx950).
 *
 * This is the drop-in boundary for ONE hot path of optical-rl-gym: the per-env
 * reset()/step()/observation()/heuristic loop of RWAEnv / RMSAEnv / DeepRMSAEnv / RMCSAEnv.
 * The reference is pure Python (no FFI of its own); each entry point below names the
 * reference interface it stands in for (file:line relative to the reference repo).  The
 * ctypes binding a maintainer would add is shown in INTEGRATION.md and implemented in
 * optical_rl_gym_amd/_lib.py.
 *
 * Conventions
 *   - every function returns 0 on success or a negative ORL_E_* code; orl_last_error() gives text
 *   - nothing throws across the ABI; no torch / HIP types appear in any signature
 *   - host buffers are caller-owned, C-contiguous, valid only for the duration of the call
 *   - device memory is owned by the handles; one batch lives on ONE GPU (multi-GPU = one process and
 *     one batch per GPU; envs are independent, there is no collective)
 *   - a handle is not thread-safe: one host thread drives it (the reference env is single-threaded too)
 *   - `n_envs` independent envs; env i behaves exactly like a reference env constructed with seed_i
 */
#ifndef ORL_H
#define ORL_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: orl_env_config starts with struct_size and carries the QoSConstrainedRA fields; ORL_E_INTERNAL; orl_multi_* (round 3).
 * A client compiled against another layout is refused by orl_batch_create (struct_size) and by the loader (version). */
#define ORL_ABI_VERSION 2

#define ORL_OK 0
#define ORL_E_INVALID (-1)   /* bad argument / unsupported configuration */
#define ORL_E_HIP (-2)       /* HIP runtime error (no GPU, out of memory, launch failure) */
#define ORL_E_ACTION (-3)    /* an action was out of the action space (reference: IndexError, rmsa_env.py:167) */
#define ORL_E_OVERFLOW (-4)  /* an env exceeded its pending-release capacity */
#define ORL_E_INTERNAL (-5)  /* a C++ exception (std::bad_alloc, ...) was stopped at the boundary: nothing throws across the ABI */

/* env families (optical_rl_gym/__init__.py:3-26 registry ids) */
#define ORL_ENV_RMSA 0      /* "RMSA-v0"      optical_rl_gym/envs/rmsa_env.py:18 */
#define ORL_ENV_DEEPRMSA 1  /* "DeepRMSA-v0"  optical_rl_gym/envs/deeprmsa_env.py:9 */
#define ORL_ENV_RWA 2       /* "RWA-v0"       optical_rl_gym/envs/rwa_env.py:15 */
#define ORL_ENV_RMCSA 3     /* "RMCSA-v0"     optical_rl_gym/envs/rmcsa_env.py:18 */
#define ORL_ENV_QOS 4       /* "QoSConstrainedRA-v0"  optical_rl_gym/envs/qos_constrained_ra.py:13 (its constructor raises
                             * upstream, :32-41; semantics as the class is written, see oracle/gen_golden_qos.py).  Actions: the
                             * path index (Discrete(k + reject)); policies SP_FF / SAP_FF / LLP_FF = shortest_path /
                             * shortest_available_path / least_loaded_path (:408-450); info: the two service blocking rates. */

/* on-device heuristics.  RMSA: rmsa_env.py:747-803; DeepRMSA: deeprmsa_env.py:135-155 (SP=0, SAP=1);
 * RWA: rwa_env.py:425-502; RMCSA: rmcsa_env.py:882-911 (id 1). */
#define ORL_POLICY_SP_FF 0
#define ORL_POLICY_SAP_FF 1 /* k-shortest-path first-fit (KSP-FF) */
#define ORL_POLICY_LLP_FF 2
#define ORL_POLICY_SAP_LF 3 /* RWA only */
/* PathOnlyFirstFitAction (rmsa_env.py:840-874, rwa_env.py:505-536): the agent chose the path (Discrete(k + reject)), the
 * device finds the first fitting slot on it.  The per-env path column is set with orl_batch_set_paths() or written into
 * the ORL_BUF_PATHS device array.  RMSA and RWA. */
#define ORL_POLICY_PATH_FF 4

/* Flattened topology: what the reference keeps in topology.graph["ksp"] / ["modulations"] and in the
 * networkx edge attributes (examples/create_topology.py:96-147).  All arrays are copied.
 * Accepted: 2..512 nodes, 1..128 links, k_paths 1..64, max_hops 1..30, 1..255 modulations, n_paths[i] <= k_paths, every link
 * index < n_links, edge_iter_order a permutation; anything else is ORL_E_INVALID.  (A connected topology has at most
 * n_links + 1 nodes, so the link limit is the one that binds: 129 nodes — a tree of 128 links — is the largest connected
 * network the library takes; more nodes only with node pairs that have no path.) */
typedef struct {
  int32_t n_nodes, n_links, k_paths, max_hops, n_modulations;
  const int32_t* n_paths;         /* [n_nodes*n_nodes]            paths available for (src,dst) */
  const int32_t* path_hops;       /* [n_nodes*n_nodes*k]          Path.hops */
  const int32_t* path_links;      /* [n_nodes*n_nodes*k*max_hops] edge "index" per hop, -1 padded */
  const double* path_length;      /* [n_nodes*n_nodes*k]          Path.length (km) */
  const int32_t* path_modulation; /* [n_nodes*n_nodes*k]          index of the modulation the heuristics use */
  const int32_t* edge_iter_order; /* [n_links]                    link index of the i-th edge of topology.edges() */
} orl_topology_desc;

/* Traffic + environment parameters: the reference constructors' kwargs after their own derivations
 * (optical_network_env.py:14-94, rmsa_env.py:29-161, deeprmsa_env.py:10-46, rwa_env.py:19-94,
 * rmcsa_env.py:29-207).  Float tables are computed on the host with the reference's own expressions. */
typedef struct {
  uint32_t struct_size;        /* sizeof(orl_env_config) as the caller compiled it; checked by orl_batch_create */
  int32_t env_type;            /* ORL_ENV_* */
  int32_t num_spectrum_resources;
  int32_t num_spatial_resources; /* cores; 1 unless RMCSA */
  int32_t episode_length;
  int32_t allow_rejection;
  int32_t j;                   /* DeepRMSA: blocks per path */
  int32_t bit_rate_mode;       /* 0 = continuous randint(lo, hi), 1 = discrete choices(bit_rates, probs) */
  int32_t bit_rate_lo, bit_rate_hi;
  int32_t n_bit_rates;         /* rows of the bit-rate tables: hi-lo+1 (continuous) or len(bit_rates) */
  int32_t event_capacity;      /* pending releases per env (0 = derive from load) */
  int32_t action_histograms;   /* != 0: keep actions_output / actions_taken per env: [2][k+1][S+1] (rmsa_env.py:126-137,
                                * rwa_env.py:52-58); RMCSA [2][k+1][M+1][C+1][S+1] (rmcsa_env.py:145-180; 863 KB per env at 7 x 320) */
  double lambda_arrival;       /* 1 / mean_service_inter_arrival_time  (rmsa_env.py:548-550) */
  double lambda_holding;       /* 1 / mean_service_holding_time        (rmsa_env.py:553) */
  const double* cum_src;       /* [n_nodes]          accumulate(node_request_probabilities) */
  const double* cum_dst;       /* [n_nodes*n_nodes]  per src: accumulate(probs with src zeroed, renormalised) */
  const int32_t* bit_rates;    /* [n_bit_rates]      bit rate of table row i */
  const double* cum_bit_rate;  /* [n_bit_rates]      discrete mode: accumulate(bit_rate_probabilities) */
  const uint8_t* n_slots;      /* [n_bit_rates*n_modulations] get_number_slots (rmsa_env.py:610-621) */
  const double* lmax_snr;      /* [n_modulations*n_bit_rates] RMCSA reach limit, eq.(1) (rmcsa_env.py:366-375); may be NULL */
  const double* lmax_xt;       /* [n_modulations]             RMCSA reach limit, eq.(2) (rmcsa_env.py:377-379); may be NULL */
  /* QoSConstrainedRA only (qos_constrained_ra.py:21-23); ignored (may be 0 / NULL) for the other families */
  int32_t n_service_classes;   /* num_service_classes */
  int32_t reserved;
  const double* cum_class;     /* [n_service_classes] accumulate(classes_arrival_probabilities) */
  const double* class_reward;  /* [n_service_classes] classes_reward */
} orl_env_config;

typedef struct orl_topology orl_topology;
typedef struct orl_batch orl_batch;

/* per-env integer counters, in this order (optical_network_env.py:29-34, rmsa_env.py:73-76) */
#define ORL_N_COUNTERS 8
/* current service record: arrival_time, holding_time, source_id, destination_id, bit_rate, service_id */
#define ORL_N_SERVICE 6

#define ORL_MAX_STEP_KERNELS 12
typedef struct {
  double ms_total;   /* wall time of the whole call on the device (HIP events) */
  double ms_policy;  /* time_kernels == 2: average duration of one stand-alone slot-scan (policy) launch */
  double ms_step;    /* time_kernels == 2: average duration of the launches of one step() */
  int64_t launches;  /* kernel launches issued */
  /* time_kernels == 0 with the persistent kernel: n_kernels = 1, kernel_name[0] = "k_persist", launches = number of its
   * launches (chunks of 128 steps), ms_kernel[0] = their average duration (ms_total / launches).
   * time_kernels == 1: the kernels one policy+step of the device loop launches, in launch order, each bracketed by HIP
   * events on the stream it runs on; average duration per launch */
  int32_t n_kernels;
  int32_t reserved;
  double ms_kernel[ORL_MAX_STEP_KERNELS];
  char kernel_name[ORL_MAX_STEP_KERNELS][32];
} orl_run_stats;

int orl_abi_version(void);
const char* orl_last_error(void);
int orl_device_count(void);

int orl_topology_create(const orl_topology_desc* desc, int device_id, orl_topology** out);
void orl_topology_destroy(orl_topology* t);

/* n_envs envs on device `device_id`.  mt_state: [n_envs][625] uint32 = random.Random(seed_i).getstate()[1]
 * (624 state words + index), i.e. optical_network_env.py:205-210 done by the caller.  Construction ends with
 * the reference's reset(only_episode_counters=False) (rmsa_env.py:160-161): every env holds its first service. */
int orl_batch_create(const orl_env_config* cfg, const orl_topology* topo, int64_t n_envs, const uint32_t* mt_state,
                     orl_batch** out);
/* Same, but the device runs random.Random(seed_i) itself (CPython random_seed -> init_by_array on abs(seed)). */
int orl_batch_create_seeded(const orl_env_config* cfg, const orl_topology* topo, int64_t n_envs, const int64_t* seeds,
                            orl_batch** out);
void orl_batch_destroy(orl_batch* b);
/* Per-env traffic load.  Env i has its own pair (lambda_arrival_i, lambda_holding_i) = (1 / mean_service_inter_arrival_time,
 * 1 / mean_service_holding_time), computed by the caller with the reference's expressions (optical_network_env.py:92-94,
 * rmsa_env.py:548-553); the two constructors above give every env the configuration's pair.  Rates are CONFIGURATION, not
 * simulation state: orl_batch_reset (soft or full), orl_batch_reseed and orl_batch_set_state leave them alone, and they are not
 * part of orl_batch_state_bytes / the snapshot format — a restored batch keeps the rates it has.
 * orl_batch_create_with_rates: orl_batch_create / orl_batch_create_seeded (exactly one of mt_state / seeds non-NULL) with
 * lambda_arrival / lambda_holding [n_envs] each, or NULL = the configuration's scalar for every env.  The rates are on the device
 * before the constructor's reset draws the first service.  With event_capacity == 0 the capacity is derived from the largest
 * lambda_arrival / lambda_holding of the batch. */
int orl_batch_create_with_rates(const orl_env_config* cfg, const orl_topology* topo, int64_t n_envs, const uint32_t* mt_state,
                                const int64_t* seeds, const double* lambda_arrival, const double* lambda_holding, orl_batch** out);
/* set_load(load, mean_service_holding_time) (optical_network_env.py:76-94) for the envs selected by env_mask (NULL = all, else
 * [n_envs] bytes): services drawn after the call use the new rates; the pending service, the clock, the pending releases, the
 * random stream, counters and statistics do not change.  Arrays [n_envs] (entries of unselected envs are ignored); either may be
 * NULL = keep.  Ordered on the batch's stream behind whatever is queued; returns synchronised.  Returns ORL_E_INVALID, with
 * nothing modified, for: a non-finite or non-positive rate of a selected env; a selected env whose load lambda_arrival /
 * lambda_holding needs more pending releases than the batch's event_capacity (by the formula that derives it at creation);
 * a batch whose last device-resident run did not complete (services it parked were drawn with the old rates: reset or restore
 * the batch first, as for orl_batch_get_state). */
int orl_batch_set_rates(orl_batch* b, const double* lambda_arrival, const double* lambda_holding, const uint8_t* env_mask);
/* The rates in force, read back from the device: [n_envs] each, either may be NULL. */
int orl_batch_get_rates(orl_batch* b, double* lambda_arrival_out, double* lambda_holding_out);
/* Pending releases per env the batch has room for: the configuration's event_capacity, or with 0 the value derived from the
 * (largest) load, (int)(load + 10 sqrt(load) + 64), either rounded up to a multiple of 64.  What orl_batch_set_rates compares
 * the same expression of a new load with. */
int orl_batch_event_capacity(const orl_batch* b);

int orl_batch_info_dim(const orl_batch* b); /* floats per env in the info row */
int orl_batch_obs_dim(const orl_batch* b);  /* DeepRMSA observation length, else 0 */

/* reset(only_episode_counters = !full) (rmsa_env.py:284-359, rwa_env.py:164-208, rmcsa_env.py:386-483).
 * env_mask: NULL = all envs, else [n_envs] bytes. */
int orl_batch_reset(orl_batch* b, int full, const uint8_t* env_mask);

/* seed(seed) (optical_network_env.py:205-210): env i (of the envs selected by env_mask, NULL = all) continues with the
 * random stream of random.Random(seeds[i]); nothing else of its state changes.  seeds: [n_envs] (entries of unselected
 * envs are ignored). */
int orl_batch_reseed(orl_batch* b, const int64_t* seeds, const uint8_t* env_mask);

/* evaluate_heuristic on the device (utils.py:103-141: reset, loop until done, sum the rewards, n episodes).  Arm a per-env
 * log of `capacity` episodes (0 = disarm); from then on every env that finishes an episode appends its
 * episode_services_accepted — the episode's reward sum for RMSA / RWA / RMCSA (reward 1 per accepted service), and
 * 2 * accepted - steps for DeepRMSA (reward +1 / -1) — before the auto (soft) reset.  Read it back with
 * orl_batch_get_episode_log: counts[n_envs], accepted[n_envs][capacity].
 *
 * A full log: counts[i] goes on counting every episode env i finishes, beyond `capacity`; row i holds the first `capacity`
 * episodes in the order they finished (entries behind min(counts[i], capacity) are 0); an episode that finishes after the row is
 * full is written nowhere — not over an earlier entry, not into another env's row.  So counts[i] > capacity says that
 * counts[i] - capacity episodes were dropped.  The same holds for the reward sums of orl_batch_get_episode_rewards.
 * Every route logs: device-resident runs (whatever the run plan) and host-driven steps through every step kernel.  A step without
 * auto reset logs the episode when it returns done, once: an env stepped on without a reset never reports done again.
 * Arming clears counts and rows, also when the log was armed before (with this or another capacity: the row stride is the
 * armed capacity); the episode in progress keeps the accepted services it has — the kernels log the env's own
 * episode_services_accepted — while the reward sums of QoSConstrainedRA start at 0.0 with the arming, so arm at an episode's start.
 * Disarmed (capacity 0) nothing is logged and orl_batch_get_episode_log is refused (ORL_E_INVALID). */
int orl_batch_episode_log(orl_batch* b, int32_t capacity);
int orl_batch_get_episode_log(orl_batch* b, int32_t* counts, int32_t* accepted);
/* QoSConstrainedRA (reward = the accepted service's class reward, qos_constrained_ra.py:131-136): the harness's episode_reward of
 * every logged episode — the float64 sum of the step rewards in step order, from 0.0 (utils.py:125-131) — [n_envs][capacity]. */
int orl_batch_get_episode_rewards(orl_batch* b, double* rewards);

/* ORL_POLICY_PATH_FF: the path index chosen for every env, [n_envs] int32 (>= k_paths = reject). */
int orl_batch_set_paths(orl_batch* b, const int32_t* paths);

/* Heuristic decision for the pending service of every env.  actions_out: [n_envs][4] int32 or NULL to keep the
 * result on the device for the next orl_batch_step(actions = NULL).
 * Columns: RMSA/RWA (path, slot, -, -); DeepRMSA (action, -, -, -); RMCSA (path, modulation, core, slot). */
int orl_batch_policy(orl_batch* b, int policy_id, int32_t* actions_out);

/* step() for every env (rmsa_env.py:163-282, deeprmsa_env.py:48-58, rwa_env.py:101-162, rmcsa_env.py:209-339).
 * actions: [n_envs][4] int32, or NULL = use the device-resident result of the last orl_batch_policy().
 * auto_reset != 0: an env that returns done is soft-reset right away (what SB3's VecEnv does).
 * Any output pointer may be NULL (result stays on the device).  reward_out/[n_envs] double, done_out/[n_envs] u8,
 * info_out/[n_envs][info_dim] double, obs_out/[n_envs][obs_dim] double (DeepRMSA).
 * Synchronous on return when any output pointer is given.
 * Errors, mirroring the reference's exceptions:
 *   ORL_E_ACTION    host-supplied `actions` hold an index outside the reference's actions_output array (IndexError at
 *                   rmsa_env.py:167, rwa_env.py:103, rmcsa_env.py:219): returned BEFORE anything is modified.  With
 *                   device-resident actions (actions = NULL) the kernel treats such an action as a rejection and the
 *                   error is reported by the next synchronous call (or orl_batch_check).
 *   ORL_E_OVERFLOW  an env needed more than event_capacity pending releases: that env's state is invalid from then on
 *                   (the reference's heap is unbounded); recreate the batch with a larger event_capacity. */
int orl_batch_step(orl_batch* b, const int32_t* actions, int auto_reset, double* obs_out, double* reward_out,
                   uint8_t* done_out, double* info_out);

/* step() in two halves, for a caller that has work of its own between issuing a step and needing its results (SB3's
 * VecEnv.step_async / step_wait, examples/stable_baselines3/DeepRMSA.ipynb:272-302 drives the env through them).
 * actions: [n_envs][action_width] (1..4 columns: the family's action, in the column order of orl_batch_step) of int32 or int64
 * (action_elem_bytes 4 / 8), C-contiguous — the array an agent hands to VecEnv.step as it is — or NULL for the device-resident
 * ones; checked and widened in one pass into the library's own page-locked staging rows.
 * orl_batch_step_async: the checks of orl_batch_step (ORL_E_ACTION before anything is modified), then everything is QUEUED on the
 * batch's stream — actions in, the step kernel, the requested results out — and the call returns.  The output buffers (any may
 * be NULL; obs_f32_out receives the observation cast to float32 on the device) must stay valid and untouched until
 * orl_batch_step_wait returns; give page-locked ones (orl_host_alloc) or the copies are staged synchronously.
 * orl_batch_step_wait: waits for that step and reports what orl_batch_step would have (ORL_E_OVERFLOW, flagged device-resident
 * actions).  One step may be pending per batch; any other call on the batch in between is ordered behind it by the stream. */
int orl_batch_step_async(orl_batch* b, const void* actions, int action_width, int action_elem_bytes, int auto_reset,
                         double* obs_out, float* obs_f32_out, double* reward_out, uint8_t* done_out, double* info_out);
int orl_batch_step_wait(orl_batch* b);

/* A heuristic's decision and the step on it in one call: what orl_batch_policy(b, policy_id, ...) followed by
 * orl_batch_step(b, NULL, auto_reset, ...) do — the heuristic of rmsa_env.py:747-803 / deeprmsa_env.py:135-155 / rwa_env.py:403-502 /
 * rmcsa_env.py:882-911, then step() — with the slot scan as the first phase of the step kernel where the 8-lanes-per-env step
 * kernel serves the batch (ONE launch per step instead of two; k_paths <= 8), else as the two launches.  For agents on the same
 * GPU that imitate, warm-start from or are compared with a heuristic.  actions_out: [n_envs][4] int32 or NULL (the actions also
 * stay in ORL_BUF_ACTIONS); the other outputs and the error behaviour as orl_batch_step with device-resident actions.  With no
 * output buffer the call only queues work on the batch's stream. */
int orl_batch_policy_step(orl_batch* b, int policy_id, int auto_reset, int32_t* actions_out, double* obs_out, double* reward_out,
                          uint8_t* done_out, double* info_out);

/* Which info entries the 8-lanes-per-env step kernel writes per step (RMSA / DeepRMSA; rmsa_env.py:228-264): 0 (default) = all of
 * them; 1 = the blocking rates only (service / episode_service / bit_rate / episode_bit_rate blocking and the per-rate entries of
 * the discrete mode) — network_compactness, network_compactness_difference, avg_link_compactness and avg_link_utilization, the
 * last two a read of every link record of every env per step, keep whatever an earlier step wrote.  For consumers that read the
 * rates only (SB3's Monitor with the reference's info_keywords, examples/stable_baselines3/DeepRMSA.ipynb:279-288).  The
 * one-wavefront-per-env kernel always writes everything. */
int orl_batch_set_info_mode(orl_batch* b, int mode);

/* DeepRMSAEnv.observation() for the pending service (deeprmsa_env.py:60-121). */
int orl_batch_observation(orl_batch* b, double* obs_out);
/* The observation array the last orl_batch_step / orl_batch_observation / orl_batch_reset left on the device (ORL_BUF_OBS), cast
 * to float32 ON THE DEVICE and copied out — half the PCIe bytes and no conversion pass on the host for agents that work in
 * float32 (SB3's default); the float64 values stay the parity-checked ones.  obs_out: [n_envs][obs_dim] float. */
int orl_batch_get_obs_f32(orl_batch* b, float* obs_out);
/* Rows env_index[0..n) of the info array the last orl_batch_step left on the device (ORL_BUF_INFO), gathered on the device and
 * copied out: info_out [n][info_dim] double.  What a VecEnv needs of info is the rows of the envs that just finished an episode
 * (SB3 reads `info["episode"]` there and nothing elsewhere, DeepRMSA.ipynb:272-302 with Monitor's info_keywords): a handful of
 * rows instead of the whole [n_envs][info_dim] array (4 MB per step at 65 536 RMSA envs) over PCIe.  Synchronous. */
int orl_batch_get_info_rows(orl_batch* b, const int64_t* env_index, int64_t n, double* info_out);

/* n_steps x { policy ; step(auto_reset) } entirely on the device (the loop of utils.evaluate_heuristic,
 * utils.py:113-128, with VecEnv-style auto reset).  time_kernels: 0 = production run (the persistent kernel where it
 * applies, else the per-env kernel with the slot scan inside), 1 = the separate-launch form with every kernel bracketed by
 * HIP events (stats->ms_kernel), 2 = stand-alone slot-scan kernel + per-env step launches (ms_policy, ms_step).
 * Returns ORL_E_OVERFLOW / ORL_E_ACTION like orl_batch_step. */
int orl_batch_run(orl_batch* b, int policy_id, int64_t n_steps, int time_kernels, orl_run_stats* stats);

int orl_batch_sync(orl_batch* b);
/* Synchronises and returns ORL_E_OVERFLOW / ORL_E_ACTION if any env flagged it since the last report (see orl_batch_step). */
int orl_batch_check(orl_batch* b);

/* Page-locked host memory for the buffers handed to orl_batch_step / orl_batch_policy: copies to and from it run at the
 * full PCIe rate (pageable numpy memory is staged through a bounce buffer by the runtime). */
int orl_host_alloc(size_t bytes, void** out);
int orl_host_free(void* p);

/* Zero-copy access for an agent that lives on the same GPU (the reference hands numpy arrays to SB3,
 * DeepRMSA.ipynb:272-302).  Device pointers of the batch's I/O arrays: write actions there, call
 * orl_batch_step(b, NULL, auto_reset, NULL, NULL, NULL, NULL) (no copies, no synchronisation: the launches are queued
 * on the batch's stream), orl_batch_sync(b), read reward / done / info / obs in place.  The pointers stay valid until
 * orl_batch_destroy.  `which`: */
#define ORL_BUF_ACTIONS 0  /* int32 [n_envs][4] */
#define ORL_BUF_REWARD 1   /* f64   [n_envs] */
#define ORL_BUF_DONE 2     /* u8    [n_envs] */
#define ORL_BUF_INFO 3     /* f64   [n_envs][info_dim] */
#define ORL_BUF_OBS 4      /* f64   [n_envs][obs_dim] (DeepRMSA) */
#define ORL_BUF_TERM_OBS 5 /* f64   [n_envs][obs_dim]: observation before an auto reset */
#define ORL_BUF_PATHS 6    /* int32 [n_envs]: path column of ORL_POLICY_PATH_FF */
#define ORL_BUF_ACTION_MASK 7 /* u8 [n_envs][pitch]: the rows of the last orl_batch_action_mask, in that call's layout (pitch of
                               * orl_batch_action_mask_shape); each layout has a buffer of its own, allocated by its first call, so a
                               * pointer taken after a JOINT call keeps showing JOINT rows; n_elements = 0 before any call */
#define ORL_BUF_MATRIX_PATHS_OBS 8 /* u8 [n_envs][pitch]: rows of the last orl_batch_matrix_paths_observation (pitch of
                                    * orl_batch_matrix_paths_obs_shape); allocated by the first call, n_elements = 0 before it */
#define ORL_BUF_PATH_FEATURES 9  /* f32 [n_envs][pitch]: rows of the last orl_batch_path_features (pitch, in floats, of
                                  * orl_batch_path_features_shape for that call's j); each j has a buffer of its own, allocated by
                                  * its first call; n_elements = 0 before any call */
#define ORL_BUF_LINK_FEATURES 10  /* f32 [n_envs][pitch]: rows of the last orl_batch_link_features (pitch, in floats, of
                                  * orl_batch_link_features_shape); allocated by the first call, n_elements = 0 before it */
#define ORL_BUF_ASSIGN_TABLE 11   /* int32 [n_envs][pitch]: the per-path table of the last orl_batch_route_spectrum, row p at columns
                                   * 4p .. 4p+3 (pitch of orl_batch_assign_table_shape); allocated by the first call, n_elements = 0
                                   * before it */
#define ORL_BUF_CORE_TABLE 12     /* int32 [n_envs][pitch]: RMCSA's (path, core) table of the last orl_batch_route_cores, row p C + c at
                                   * columns 4 (p C + c) .. + 3 (pitch of orl_batch_core_table_shape); allocated by the first call,
                                   * n_elements = 0 before it */
#define ORL_BUF_BLOCK_TABLE 13    /* int32 [n_envs][pitch]: the block table of the last orl_batch_block_table, row r at columns
                                   * (2 + 2j) r .. (pitch of orl_batch_block_table_shape for that call's j); each j has a buffer of its
                                   * own, allocated by its first call; n_elements = 0 before any call */
#define ORL_BUF_BLOCK_MASK 14     /* u8 [n_envs][pitch]: the mask of the block action space the same call left (mask pitch of
                                   * orl_batch_block_table_shape); one per j beside the table */
#define ORL_BUF_RELEASE_HORIZONS 15 /* f32 [n_envs][pitch]: rows of the last orl_batch_release_horizons (pitch, in floats, of
                                   * orl_batch_release_horizons_shape for that call's layout and j); allocated by the first call and
                                   * replaced by a larger one when a later call needs more; n_elements = 0 before any call */
#define ORL_BUF_PATH_CAPACITY 16   /* i32 [n_envs][pitch]: rows of the last orl_batch_network_capacity(ORL_CAPACITY_PATHS) */
#define ORL_BUF_SERVICEABLE 17     /* u8 [n_envs][pitch]: rows of the last orl_batch_network_capacity(ORL_CAPACITY_SERVICEABLE) */
#define ORL_BUF_CAPACITY_COUNTS 18 /* i32 [n_envs][pitch]: rows of the last orl_batch_network_capacity(ORL_CAPACITY_COUNTS); each of
                                    * the three is a buffer of its own at its layout's pitch (orl_batch_network_capacity_shape),
                                    * allocated by that layout's first call; n_elements = 0 before it */
#define ORL_BUF_CAPACITY_AFTER_CLASSES 19 /* i32 [n_envs][pitch]: rows of the last orl_batch_capacity_after(ORL_AFTER_CLASSES) */
#define ORL_BUF_CAPACITY_AFTER_TOTAL 20   /* i32 [n_envs][pitch]: rows of the last orl_batch_capacity_after(ORL_AFTER_TOTAL); each of the two
                                           * is a buffer of its own at the last call's pitch (orl_batch_capacity_after_shape), allocated
                                           * by that layout's first call and replaced by a larger one — of at least twice the size, at
                                           * most what ORL_AFTER_MAX_Q candidates need — when a later call has more candidates; the
                                           * one replaced lives on with the batch; n_elements = 0 before any call */
int orl_batch_device_buffer(orl_batch* b, int which, void** device_ptr, int64_t* n_elements);
/* The HIP stream (hipStream_t) the batch queues its launches on.  An agent on the same GPU that queues ITS kernels on this
 * stream too (torch: `torch.cuda.ExternalStream(ptr)`) needs no synchronisation between its network and orl_batch_step: the
 * step kernel runs after the kernels that wrote the actions, the network's next forward pass after the step kernel that wrote
 * the observation.  (orl_batch_run also uses a second stream internally and returns synchronised.) */
int orl_batch_stream(orl_batch* b, void** hip_stream_out);

/* state read-back (parity tests, Python attribute surface) */
int orl_batch_get_counters(orl_batch* b, int64_t* out /*[n_envs][ORL_N_COUNTERS]*/);
int orl_batch_get_services(orl_batch* b, double* out /*[n_envs][ORL_N_SERVICE]*/);
int orl_batch_get_slots(orl_batch* b, int64_t env, uint8_t* out /*[cores][links][slots] 0/1*/);
int orl_batch_get_link_stats(orl_batch* b, int64_t env, double* out /*[4][links]: utilization, external_fragmentation, compactness, last_update*/);
/* the same for every env at once: the slot maps as the device keeps them — bit s of 64-bit word s / 64 of a (core, link) row
 * set = slot s free, rows of orl_batch_row_words() words, orl_batch_map_words() words per env (cores * links * row words, padded
 * to an even number) — and [n_envs][4][links] link statistics, [n_envs][4] network statistics */
int orl_batch_row_words(const orl_batch* b);
int orl_batch_map_words(const orl_batch* b);
int orl_batch_get_slots_packed(orl_batch* b, uint64_t* out /*[n_envs][map_words]*/);
int orl_batch_get_link_stats_all(orl_batch* b, double* out /*[n_envs][4][links]*/);
int orl_batch_get_net_stats_all(orl_batch* b, double* out /*[n_envs][4]*/);
/* QoSConstrainedRA: topology.graph["available_spectrum"] of one env (free units per link, optical_network_env.py:189-193) */
int orl_batch_get_spectrum(orl_batch* b, int64_t env, int32_t* out /*[links]*/);
int orl_batch_get_net_stats(orl_batch* b, int64_t env, double* out /*[4]: throughput, compactness, last_update, current_time*/);
int orl_batch_get_active(orl_batch* b, int32_t* out /*[n_envs] pending releases*/);
int orl_batch_get_flags(orl_batch* b, int32_t* out /*[n_envs] bit0 event overflow, bit1 bad action*/);
/* actions_output and actions_taken of one env (batch created with action_histograms): int32 [2][k_paths+1][slots+1]
 * (rmsa_env.py:126-137, 167, 201, 211-212; rwa_env.py:52-58, 103, 125, 132-133 — RWA uses the top-left
 * [k+reject][slots+reject] corner); RMCSA: int32 [2][k_paths+1][modulations+1][cores+1][slots+1] (rmcsa_env.py:145-180,
 * 219, 273, 284-289) */
int orl_batch_get_action_histograms(orl_batch* b, int64_t env, int32_t* out);
/* The pending releases of one env (the reference's heap `_events`, optical_network_env.py:143-154, unordered): returns
 * their number; fills up to `capacity` entries of time_out[] (release time) and rec_out[][6] = (src*n_nodes+dst, path
 * index, initial slot, number of slots, core, bit rate) when both pointers are given. */
int orl_batch_get_pending(orl_batch* b, int64_t env, int32_t capacity, double* time_out, int32_t* rec_out);
/* summed over envs: services_processed, services_accepted (for throughput/blocking reports) */
int orl_batch_totals(orl_batch* b, int64_t* processed, int64_t* accepted);

/* SimpleMatrixObservation (rmsa_env.py:806-837, rmcsa_env.py:914-947) for every env:
 * uint8 [n_envs][2*n_nodes + cores*links*slots] = one-hot(min(src,dst)), one-hot(max(src,dst)), slot map. */
int orl_batch_matrix_obs_dim(const orl_batch* b);
int orl_batch_matrix_observation(orl_batch* b, uint8_t* out);

/* Several GPUs of one node from one process (the `n_devices, device_ids` of the batch constructor).  Envs are
 * independent, so the group is nothing but contiguous shards of the env index range — shard r holds envs
 * [first_env, first_env + n) on device_ids[r], seeds[first_env ...] — each an ordinary orl_batch bound to its device:
 * use orl_multi_shard() with every per-batch entry point above (scatter actions / gather results per shard).  No collective,
 * no peer access.  orl_multi_run drives the device-resident loop of all shards at once, one host thread per shard;
 * stats: [n_shards] or NULL; returns the first non-zero shard status.  The same device may be listed more than once. */
typedef struct orl_multi orl_multi;
int orl_multi_create(const orl_env_config* cfg, const orl_topology_desc* topo, int64_t n_envs, const int64_t* seeds,
                     int n_devices, const int* device_ids, orl_multi** out);
int orl_multi_n_shards(const orl_multi* m);
orl_batch* orl_multi_shard(orl_multi* m, int shard, int64_t* first_env /*nullable*/, int64_t* n_envs /*nullable*/);
int orl_multi_run(orl_multi* m, int policy_id, int64_t n_steps, orl_run_stats* stats);
void orl_multi_destroy(orl_multi* m);

/* Action masks of the pending service — what the next step() acts on, after any reset / step / policy_step / run / set_state,
 * auto resets included — for every env, computed on the device next to the slot maps (sb3-contrib's MaskablePPO reads them
 * through `action_masks()`; a torch agent fills the masked logits with -inf).  RMSA, DeepRMSA and RWA take ORL_MASK_JOINT /
 * ORL_MASK_PATH, RMCSA the two-stage pair ORL_MASK_PATH_MOD / ORL_MASK_CORE_SLOT; any other combination and QoSConstrainedRA
 * return ORL_E_INVALID.  Per env a row of `dim` bytes, 0 or 1; the last column is the reject action and equals allow_rejection.
 * Layouts: */
#define ORL_MASK_JOINT 0 /* RMSA / RWA: dim = k*S + 1, column i < dim-1 = action (i / S, i % S) (path, first slot / wavelength);
                          * DeepRMSA: dim = k*j + 1, column i = action i.  1 iff stepping that action provisions the service:
                          * rmsa_env.py:163-200 with is_path_free :623-636; deeprmsa_env.py:48-58 with get_available_blocks
                          * rmsa_env.py:667-697; rwa_env.py:101-135.  A path index >= n_paths[src, dst] is 0 (IndexError there). */
#define ORL_MASK_PATH 1  /* PathOnlyFirstFitAction (RMSA / RWA): dim = k + 1, column p = the wrapper's first fit finds a slot on
                          * path p — RMSA searches range(0, S - n) (rmsa_env.py:848-871), RWA every wavelength (rwa_env.py:518-533). */
/* RMCSA: an action is (path p, modulation m, core c, first slot s), and stepping it provisions — prov(p, m, c, s) — iff, with
 * n = n_slots[bit rate][m]: p < n_paths[src, dst], m < M, c < C, s + n <= S (s = S - n is valid), slots s .. s + n - 1 are free in
 * core c on every hop, and length(p) < lmax_xt[m] and length(p) < lmax_snr[m][bit rate] (rmcsa_env.py:209-289 with is_path_free
 * :767-794, get_number_slots :753-765, _crosstalk_is_acceptable :341-384).  A flat mask would have k*M*C*S columns; validity
 * factorises exactly into the two rows a two-head or autoregressive policy masks its logits with: sampling stage 1, then stage
 * 2 for the sampled pair, never yields a blocked action while a provisioning one exists. */
#define ORL_MASK_PATH_MOD 2  /* RMCSA, stage 1: dim = k*M + 1, column p*M + m = 1 iff some (c, s) has prov(p, m, c, s). */
#define ORL_MASK_CORE_SLOT 3 /* RMCSA, stage 2: dim = C*S + 1, column c*S + s = prov(p, m, c, s) for a pair (p, m) given per env:
                              * columns 0 and 1 of the env's row of ORL_BUF_ACTIONS (where an agent on the GPU writes its stage-1
                              * choice), or the `given` of orl_batch_action_mask_given.  A pair out of range (negative included)
                              * or beyond reach has no provisioning column.  The mask never touches env state or flags. */
/* Fallback: a row without a provisioning column gets, when allow_rejection == 0, every non-reject column set — every action of
 * the space then has the same effect (rejection) and a masked categorical never meets a row of -inf only.
 * orl_batch_action_mask_shape: *dim and the device pitch round_up(dim, 16) of ORL_BUF_ACTION_MASK's rows for `layout`.
 * orl_batch_action_mask: one launch on the batch's stream into ORL_BUF_ACTION_MASK (no synchronisation, graph-capturable: the
 * buffer is allocated by the first call, which should therefore come before a capture); with out != NULL ([n_envs][dim] bytes)
 * the rows are then copied out densely and the call synchronises.
 * orl_batch_action_mask_given: the same with the pairs of ORL_MASK_CORE_SLOT from the host — `given` [n_envs][2] int32 (path,
 * modulation) goes through a page-locked buffer of the batch into a device buffer of the batch, asynchronously on the batch's
 * stream (both allocated by the first such call); ORL_BUF_ACTIONS is not touched.  given == NULL: orl_batch_action_mask.  A `given`
 * with another layout is ORL_E_INVALID.  A configuration whose rows exceed the kernel's LDS budget (none with k <= 8) is refused
 * with ORL_E_INVALID before anything is queued. */
int orl_batch_action_mask_shape(const orl_batch* b, int layout, int32_t* dim, int32_t* pitch);
int orl_batch_action_mask(orl_batch* b, int layout, uint8_t* out);
int orl_batch_action_mask_given(orl_batch* b, int layout, const int32_t* given /* host [n_envs][2], or NULL = ORL_BUF_ACTIONS */, uint8_t* out);

/* MatrixObservationWithPaths (qos_constrained_ra.py:440-493) of the pending service of every env, built on the device from the
 * link counters: QoSConstrainedRA only (other families return ORL_E_INVALID).  Per env a row of dim = links * S * (k + 1) + 1
 * bytes: the reference's float64 [links, (k + 1) S] matrix flattened link-major, then the service class as a byte (it exceeds 1
 * for classes >= 2, as in the reference).  Block b of S columns of link l is a prefix run of ones of length
 *   b = 0: S - a_l (a_l = free units of l);  1 <= b <= k: min(S - a_l + 1, S) if l lies on allowed path b - 1, else 1 if b >= 2,
 *   l lies on allowed path b - 2 and a_l = 0 (the reference's slice runs one column into the next path's block, clipped at the
 *   end of the row), else 0.  Path p is allowed iff p < n_paths[src, dst] and (class != 0 or p == 0).
 * orl_batch_matrix_paths_obs_shape: *dim and the device pitch round_up(dim, 16) of ORL_BUF_MATRIX_PATHS_OBS's rows.
 * orl_batch_matrix_paths_observation: one launch on the batch's stream into ORL_BUF_MATRIX_PATHS_OBS (no synchronisation,
 * graph-capturable: the buffer is allocated by the first call, which should therefore come before a capture; a failed
 * allocation returns ORL_E_HIP and leaves the batch usable); with out != NULL ([n_envs][dim] bytes) the rows are then copied
 * out densely and the call synchronises. */
int orl_batch_matrix_paths_obs_shape(const orl_batch* b, int32_t* dim, int32_t* pitch);
int orl_batch_matrix_paths_observation(orl_batch* b, uint8_t* out);

/* Path features of the pending service of every env — the feature table of DeepRMSAEnv.observation (deeprmsa_env.py:60-121) as a
 * float32 device observation for every slot-map family: RMSA, DeepRMSA, RWA and RMCSA (QoSConstrainedRA, which has no slot maps,
 * returns ORL_E_INVALID).  `j` in [1, 8] is the number of free blocks listed per row, a parameter of the call (independent of a
 * DeepRMSA batch's own j).  Per env a row of dim = 1 + 2 n_nodes + R (2 j + 3) floats, R = k (RMCSA: R = k * cores, row p * cores
 * + c, path-major as rmcsa_env.py:889-906):
 *   column 0 = bit_rate / 100 (RWA: 0.0); column 1 + min(src, dst) = 1; column 1 + n_nodes + max(src, dst) = 1; other header
 *   columns 0; then per row r (path p, core c) a block of 2 j + 3 values, all -1.0 when p >= n_paths[src, dst], else with m = the
 *   slots free on every hop of p in core c and n = the slots the service needs (RMSA / DeepRMSA: get_number_slots under the path's
 *   best modulation; RWA: 1; RMCSA: under the path's best modulation — the one SAP_BM_FC_FF uses — for modulation == -1, under
 *   modulation m for every path for modulation == m in [0, M)):
 *     [2 b], [2 b + 1]  for b < min(j, maximal free runs of >= n slots), in slot order: 2 (start - 0.5 S) / S, (length - 8) / 8;
 *                       the block's other columns below 2 j stay -1.0
 *     [2 j] = (n - 5.5) / 3.5;  [2 j + 1] = 2 (popcount(m) - 0.5 S) / S;
 *     [2 j + 2] = (popcount(m) / runs(m) - 4) / 4 when m has a free run, else -1.0
 * Every value is the reference's float64 expression rounded to float32 once: on a DeepRMSA batch with its own j the row is the
 * float32 cast of its observation, bit for bit.  A modulation other than -1 outside RMCSA, a modulation outside [-1, M) and a j
 * outside [1, 8] return ORL_E_INVALID before anything is queued.
 * orl_batch_path_features_shape: *dim, *rows = R and the device pitch IN FLOATS, round_up(dim, 4), of ORL_BUF_PATH_FEATURES' rows.
 * orl_batch_path_features: one launch on the batch's stream into ORL_BUF_PATH_FEATURES (no synchronisation, graph-capturable:
 * the buffer of a j is allocated by the first call with that j, which should therefore come before a capture); with out != NULL
 * ([n_envs][dim] floats) the rows are then copied out densely and the call synchronises.  The pending service and the slot maps
 * are read as the last step or reset left them; nothing of the env is written. */
int orl_batch_path_features_shape(const orl_batch* b, int j, int32_t* dim, int32_t* rows, int32_t* pitch);
int orl_batch_path_features(orl_batch* b, int j, int modulation, float* out /* host [n_envs][dim], or NULL */);

/* Link features of the pending service of every env — the state per LINK, for agents that are graph networks over the topology,
 * where the path features above describe it per candidate path: RMSA, DeepRMSA, RWA and RMCSA (QoSConstrainedRA, which has no slot
 * maps, returns ORL_E_INVALID).  Per env a row of dim = 1 + 2 n_nodes + R F floats: the header of the path features (column 0 =
 * bit_rate / 100, RWA: 0.0; column 1 + min(src, dst) = 1; column 1 + n_nodes + max(src, dst) = 1; other header columns 0), then
 * R = cores * links blocks of F = 10 + k values, block r = c * links + l — the order of the slot maps, [cores][links] of
 * orl_batch_get_slots; cores = 1 outside RMCSA; l is the link index of the topology's path_links and of orl_batch_get_link_stats.
 * With a = the free-slot row of core c and link l, S its slots and f = the number of free slots:
 *   [0] f / S;  [1] maximal free runs / S;  [2] longest free run / S (0 when there is none);
 *   [3] first free slot / S;  [4] (last free slot + 1) / S;  both -1.0 when f == 0;
 *   [5] cur_external_fragmentation and [6] cur_link_compactness of the row as it stands (rmsa_env.py:492-528 = rmcsa_env.py:635-672):
 *       what _update_link_stats would feed into the link's running averages now — 0.0 for a row without a free slot; max_empty = 0
 *       for a single free run and for exactly two free runs at the two ends of the row; compactness 1.0 with fewer than two used
 *       runs.  RWA, whose reference keeps no such statistics, gets the same functions of the row;
 *   [7], [8], [9] the link's running utilization, external_fragmentation and compactness (orl_batch_get_link_stats columns 0 .. 2)
 *       cast to float32, the same three values for every core of a link (RWA: [8] and [9] are whatever the record holds);
 *   [10 + p] 1.0 when link l is on candidate path p of the pending (src, dst) and p < n_paths[src, dst], else 0.0; the same for
 *       every core.
 * Every value is computed in float64 and rounded to float32 once.
 * orl_batch_link_features_shape: *dim, *rows = R, *width = F and the device pitch IN FLOATS, round_up(dim, 4), of
 * ORL_BUF_LINK_FEATURES' rows; the pad columns are 0.
 * orl_batch_link_features: one launch on the batch's stream into ORL_BUF_LINK_FEATURES (no synchronisation, graph-capturable: the
 * buffer is allocated by the first call, which should therefore come before a capture); with out != NULL ([n_envs][dim] floats)
 * the rows are then copied out densely and the call synchronises.  The pending service, the slot maps and the link statistics are
 * read as the last step or reset left them; nothing of the env is written. */
int orl_batch_link_features_shape(const orl_batch* b, int32_t* dim, int32_t* rows, int32_t* width, int32_t* pitch);
int orl_batch_link_features(orl_batch* b, float* out /* host [n_envs][dim], or NULL = only queue the launch */);

/* First-fit completion of a partial RMCSA action: the agent fixes a prefix of (path p, modulation m, core c, first slot s) — nothing,
 * the path, the pair or the triple — and the device fills in the rest under prov(p, m, c, s), the predicate of ORL_MASK_PATH_MOD /
 * ORL_MASK_CORE_SLOT above, unchanged.  For an env whose first g = n_given action columns are given:
 *   g = 3 (p, m, c): the lowest s with prov(p, m, c, s);
 *   g = 2 (p, m):    the lowest column c * S + s of the env's ORL_MASK_CORE_SLOT row for that pair — cores in order, then slots;
 *   g = 1 (p):       m*(p), then as g = 2; m*(p) = the modulation that needs the fewest slots at the service's bit rate among those
 *                    within both reach limits for p (ties: the lowest index); none within reach: no completion.  "Enough free
 *                    slots exist" is monotone in n, so this completion provisions iff any column p * M + . of the env's
 *                    ORL_MASK_PATH_MOD row is set (without the fallback): that row is the mask of a one-head path-only agent too;
 *   g = 0:           the first path, in order, whose g = 1 completion exists — a reach-aware k-shortest-path first fit.
 * A given column out of range — negative, p >= n_paths[src, dst], m >= M, c >= C — or a pair beyond reach has no completion.  "No
 * completion" is the reject action (k, M, C, S), which RMCSA's heuristic (policy id 1, SAP_BM_FC_FF) returns too; it is inside actions_output under
 * either allow_rejection.  Two deliberate differences from SAP_BM_FC_FF and the reference's range(0, S - n)
 * (rmcsa_env.py:889-906): s = S - n is tried, and an action the reach check of step() would refuse is never returned (the
 * heuristic takes each path's best modulation by length alone).
 * The completion reads the pending service and the slot maps as the last step or reset left them and writes only the env's row of
 * ORL_BUF_ACTIONS, all four columns (a valid prefix comes back as given); env state, flags and snapshot bytes do not change.
 * orl_batch_complete_actions: one launch on the batch's stream.  given == NULL: the prefix is columns 0 .. n_given - 1 of
 * ORL_BUF_ACTIONS, where an agent on the GPU writes its choice; with actions_out == NULL as well the call does not synchronise,
 * allocates nothing and is graph-capturable.  A host `given` [n_envs][n_given] int32 goes through a page-locked buffer of the batch
 * into a device buffer of the batch (both allocated by the first such call, and not those of orl_batch_action_mask_given),
 * asynchronously on the batch's stream; ORL_BUF_ACTIONS is then written by the kernel only.  With actions_out != NULL the rows are
 * copied out and the call synchronises.  ORL_E_INVALID, before anything is queued: a family other than RMCSA (the single-core
 * families have ORL_POLICY_PATH_FF), n_given outside 0 .. 3, given != NULL with n_given == 0. */
int orl_batch_complete_actions(orl_batch* b, int n_given,
                               const int32_t* given /* host [n_envs][n_given], or NULL = columns 0..n_given-1 of ORL_BUF_ACTIONS */,
                               int32_t* actions_out /* host [n_envs][4], or NULL */);

/* Spectrum-assignment rules for RMSA and RWA actions: the agent gives nothing or the path p, and the device picks the first slot
 * (RWA: the wavelength) s* under a named rule — the single-core sibling of the completion above.  For the pending service of an env
 * and a path p < n_paths[src, dst]:
 *   n(p)    the slots the service needs on p: RMSA get_number_slots under the path's best modulation, RWA 1;
 *   m(p)    the AND over the hops of p of the free-slot rows, slots 0 .. S - 1;
 *   fits(p) = { s : s + n <= S and m(p)[s .. s + n - 1] all free }
 * — exactly the set columns p * S + s of the env's ORL_MASK_JOINT row without the fallback.  One deliberate difference from
 * ORL_POLICY_PATH_FF and the reference wrapper's range(0, S - n) (rmsa_env.py:848-871): s = S - n is tried, as by
 * orl_batch_complete_actions.  Each rule chooses s* from fits(p): */
#define ORL_ASSIGN_FIRST_FIT 0  /* min fits(p) */
#define ORL_ASSIGN_LAST_FIT 1   /* max fits(p) */
#define ORL_ASSIGN_BEST_FIT 2   /* among the maximal free runs of m(p) of length L >= n the one with the smallest L, ties to the
                                 * lowest start; s* = its start */
#define ORL_ASSIGN_EXACT_FIT 3  /* the lowest-start maximal free run with L == n if there is one, else ORL_ASSIGN_FIRST_FIT */
#define ORL_ASSIGN_MOST_USED 4  /* the s of fits(p) that maximises U(s), ties to the lowest s */
#define ORL_ASSIGN_LEAST_USED 5 /* the s of fits(p) that minimises U(s), ties to the lowest s */
/* U(s) = u[s] + .. + u[s + n - 1]; u[w] = the number of links of the env's whole slot map — all of them, not only those on the path
 * — on which slot w is occupied.  For RWA (n = 1) rules 4 and 5 are the textbook most-used and least-used wavelength rules, for RMSA
 * their window-sum generalisation.
 * n_given = 1: the path is given per env; a path that is negative or >= n_paths[src, dst] has no completion.  n_given = 0: the first
 * path in order with a non-empty fits(p), then the rule on that path (ORL_ASSIGN_FIRST_FIT: k-shortest-path first fit).  "No
 * completion" is the reject action (k, S), which every heuristic of the reference and ORL_POLICY_PATH_FF return too when nothing
 * fits.  The kernel writes the env's row of ORL_BUF_ACTIONS as (p, s*, 0, 0), where step(NULL) reads it; it reads only the pending
 * service and the slot maps as the last step or reset left them: env state, flags and snapshot bytes do not change.
 * orl_batch_assign_spectrum: one launch on the batch's stream.  given == NULL: the path is column 0 of ORL_BUF_ACTIONS, where an
 * agent on the GPU writes its choice; with actions_out == NULL as well the call does not synchronise, allocates nothing and is
 * graph-capturable.  A host `given` [n_envs] int32 goes through a page-locked buffer of the batch into a device buffer of the batch
 * (both allocated by the first such call, and not those of orl_batch_action_mask_given or orl_batch_complete_actions),
 * asynchronously on the batch's stream; ORL_BUF_ACTIONS is then written by the kernel only.  With actions_out != NULL the rows are
 * copied out and the call synchronises.  ORL_E_INVALID, before anything is queued: a family other than RMSA and RWA (a DeepRMSA
 * action is a block index and cannot express these rules; RMCSA has orl_batch_complete_actions), an unknown rule, n_given outside
 * 0 .. 1, given != NULL with n_given == 0. */
int orl_batch_assign_spectrum(orl_batch* b, int rule, int n_given,
                              const int32_t* given /* host [n_envs] paths, or NULL = column 0 of ORL_BUF_ACTIONS */,
                              int32_t* actions_out /* host [n_envs][4], or NULL */);

/* Routing rules and the per-path assignment table for RMSA and RWA actions: where orl_batch_assign_spectrum settles on the first path
 * that fits, this call computes the rule's winner on EVERY candidate path, hands the winners out as a table an agent on the GPU can
 * read (its action set, or features), and reduces them to one action under a routing order.  With n(p), m(p), fits(p), u[w] and U(s)
 * as defined above — for the pending service of an env and a path p < n_paths[src, dst]: n(p) the slots the service needs on p
 * (RMSA: under the path's best modulation, RWA: 1); m(p) the AND over the hops of p of the free-slot rows; fits(p) = { s : s + n <= S
 * and m(p)[s .. s + n - 1] all free }, s = S - n included; u[w] the links of the env's whole slot map with slot w occupied and U(s) =
 * u[s] + .. + u[s + n - 1] — and free(p) = popcount(m(p)):
 * The winner of a path with a non-empty fits(p) is (s*(p), c*(p)); c* is an integer cost, smaller is better.
 *   rule                    s*                                                c*
 *   ORL_ASSIGN_FIRST_FIT    min fits(p)                                       s*
 *   ORL_ASSIGN_LAST_FIT     max fits(p)                                       S - n - s*
 *   ORL_ASSIGN_BEST_FIT     as orl_batch_assign_spectrum                      L - n, L the length of the chosen maximal free run
 *   ORL_ASSIGN_EXACT_FIT    as orl_batch_assign_spectrum                      0 if a run with L == n exists, else 1 + s*
 *   ORL_ASSIGN_MOST_USED    as orl_batch_assign_spectrum                      n E - U(s*), E the links of the map
 *   ORL_ASSIGN_LEAST_USED   as orl_batch_assign_spectrum                      U(s*)
 *   ORL_ASSIGN_MIN_CUTS     the s of fits(p) with the fewest cuts, ties to    cuts(p, s*)
 *                           the lowest s
 * cuts(p, s) = the number of hops l of p with s >= 1, s + n <= S - 1, slot s - 1 free on link l and slot s + n free on link l: the
 * block then splits a free run of that link in two.  A start at slot 0 or a block ending at slot S - 1 cuts nothing on that side. */
#define ORL_ASSIGN_MIN_CUTS 6      /* accepted by orl_batch_route_spectrum only */
/* Routes, all over the paths with a non-empty fits(p): */
#define ORL_ROUTE_KSP 0            /* the lowest p: orl_batch_assign_spectrum with n_given = 0 */
#define ORL_ROUTE_BEST 1           /* the smallest c*(p), ties to the lowest p (with ORL_ASSIGN_FIRST_FIT: FF-KSP, the lowest slot over all paths) */
#define ORL_ROUTE_LEAST_LOADED 2   /* the largest free(p), ties to the lowest p (with ORL_ASSIGN_FIRST_FIT: the reference's
                                    * least_loaded_path_first_fit, except that s = S - n counts as a fit, as everywhere in these rules) */
#define ORL_ROUTE_NO_FIT 0x7fffffff
/* The action is (p, s*(p), 0, 0) in the env's row of ORL_BUF_ACTIONS, where step(NULL) reads it; the reject action (k, S, 0, 0) if no
 * path fits.  The table is int32 [n_envs][k][4] (ORL_BUF_ASSIGN_TABLE; the device pitch is 4 k): row p is (s*, c*, n(p), free(p));
 * (S, ORL_ROUTE_NO_FIT, n(p), free(p)) for a path on which nothing fits; (S, ORL_ROUTE_NO_FIT, 0, 0) for p >= n_paths[src, dst].  An
 * argmin over column 1 is ORL_ROUTE_BEST.
 * orl_batch_route_spectrum: one launch on the batch's stream; no atomics; with actions_out == NULL and table_out == NULL it does not
 * synchronise and, after the first call (which allocates the table), allocates nothing: graph-capturable.  With an output pointer the
 * rows are copied out ([n_envs][4], [n_envs][k][4]) and the call synchronises.  Env state, flags and snapshot bytes do not change.
 * ORL_E_INVALID, before anything is queued: a family other than RMSA and RWA, a rule outside 0 .. 6, a route outside 0 .. 2.
 * orl_batch_assign_table_shape: *rows = k, *width = 4 and the device pitch in int32 (4 k) of ORL_BUF_ASSIGN_TABLE's rows. */
int orl_batch_route_spectrum(orl_batch* b, int rule, int route, int32_t* actions_out /* host [n_envs][4], or NULL */,
                             int32_t* table_out /* host [n_envs][k][4], or NULL */);
int orl_batch_assign_table_shape(const orl_batch* b, int32_t* rows, int32_t* width, int32_t* pitch);

/* Core and spectrum rules with a (path, core) table for RMCSA actions: what orl_batch_route_spectrum is to the single-core families.
 * orl_batch_complete_actions is first fit in (path, core, slot) order; this call computes a rule's winner on EVERY (path, core) pair,
 * hands the winners out as a table an agent on the GPU can read, and reduces them to one action (path, modulation, core, first slot)
 * under a route — first-fit core, least-loaded core, best fit over the cores, the pair that fragments least.  For the pending service of
 * an env and every candidate pair (p, c), p < n_paths[src, dst] and c < C:
 *   m(p)       modulation = -1: m*(p) of orl_batch_complete_actions — among the modulations within both reach limits for p at this bit
 *              rate the one that needs the fewest slots, ties to the lowest index; modulation = m in [0, M): m for every path, usable
 *              on p only where it is within both reach limits (the convention of orl_batch_path_features).  A path without an m(p)
 *              cannot be used;
 *   n(p)       = nslots[br_idx][m(p)];
 *   row(p, c)  the AND over the hops of p of the free-slot rows of core c, slots 0 .. S - 1; free(p, c) = its popcount;
 *   fits(p, c) = { s : s + n <= S and row(p, c)[s .. s + n - 1] all free }, s = S - n included: the s at which stepping
 *              (p, m(p), c, s) provisions.
 * The winner (s*, c*) of a pair with a non-empty fits(p, c), c* an integer cost (smaller is better), is that of
 * orl_batch_route_spectrum's table above for ORL_ASSIGN_FIRST_FIT, ORL_ASSIGN_LAST_FIT, ORL_ASSIGN_BEST_FIT, ORL_ASSIGN_EXACT_FIT and
 * ORL_ASSIGN_MIN_CUTS with row(p, c) for m(p) and fits(p, c) for fits(p); the maximal free runs are those of row(p, c), and cuts(p, s)
 * counts the hops of p in core c.  ORL_ASSIGN_MOST_USED and ORL_ASSIGN_LEAST_USED are refused: an occupancy count over the C E rows
 * of all cores does not fit the byte counters those rules are built on.
 * Prefix: n_given = 0 — every pair is a candidate; 1 — the pairs of the env's given path; 2 — the env's given (path, core) pair alone.
 * A given column out of range (negative ones included) leaves no candidate.  The route picks among the candidate pairs with a
 * non-empty fits(p, c); ORL_ROUTE_KSP, ORL_ROUTE_BEST and ORL_ROUTE_LEAST_LOADED read over pairs in path-major order:
 *   ORL_ROUTE_KSP                    the lowest (p, c): the first path, then the first core, with a fit
 *   ORL_ROUTE_BEST                   the smallest c*, ties to the lowest (p, c)
 *   ORL_ROUTE_LEAST_LOADED           the largest free(p, c), ties to the lowest (p, c) */
#define ORL_ROUTE_KSP_BEST_CORE 3          /* the first path with any fit; among its cores the smallest c*, ties to the lowest core */
#define ORL_ROUTE_KSP_LEAST_LOADED_CORE 4  /* the first path with any fit; among its cores the largest free(p, c), ties to the lowest core */
/* (routes 3 and 4 are this call's only: orl_batch_route_spectrum refuses them.)  The action is (p, m(p), c, s*) in the env's row of
 * ORL_BUF_ACTIONS, where step(NULL) reads it; the reject action (k, M, C, S) if no candidate pair fits.  ORL_ASSIGN_FIRST_FIT with
 * ORL_ROUTE_KSP and modulation = -1 is orl_batch_complete_actions with the same n_given <= 1.
 * The table is int32 [n_envs][k C][4] (ORL_BUF_CORE_TABLE; the device pitch is 4 k C), row p C + c — the row order of
 * orl_batch_path_features — = (s*, c*, n(p), free(p, c)); (S, ORL_ROUTE_NO_FIT, n(p), free(p, c)) for a pair on which nothing fits;
 * (S, ORL_ROUTE_NO_FIT, 0, 0) for a path the service cannot use: p >= n_paths[src, dst], no modulation within reach, the fixed
 * modulation beyond reach.  The table is always complete, whatever the prefix.
 * orl_batch_route_cores: one launch on the batch's stream; no atomics.  given == NULL: the path is column 0 and the core column 2 of
 * ORL_BUF_ACTIONS — where they live in an action, so an agent on the GPU writes them there and the kernel fills in the modulation and
 * the slot; with actions_out == NULL and table_out == NULL as well the call does not synchronise and, after the first call (which
 * allocates the table), allocates nothing: graph-capturable.  A host `given` [n_envs][n_given] int32 — (path) or (path, core) — goes
 * through a page-locked buffer of the batch into a device buffer of the batch (both allocated by the first such call, this call's
 * own), asynchronously on the batch's stream; ORL_BUF_ACTIONS is then written by the kernel only.  With an output pointer the rows
 * are copied out ([n_envs][4], [n_envs][k C][4]) and the call synchronises.  Env state, flags and snapshot bytes do not change.
 * ORL_E_INVALID, before anything is queued or allocated: a family other than RMCSA, a rule outside 0 .. 3 and 6, a route outside
 * 0 .. 4, a modulation outside -1 .. M - 1, n_given outside 0 .. 2, given != NULL with n_given == 0.
 * orl_batch_core_table_shape: *rows = k C, *width = 4 and the device pitch in int32 (4 k C) of ORL_BUF_CORE_TABLE's rows. */
int orl_batch_route_cores(orl_batch* b, int rule, int route, int modulation /* -1: each path's best */, int n_given,
                          const int32_t* given /* host [n_envs][n_given], or NULL = columns 0 and 2 of ORL_BUF_ACTIONS */,
                          int32_t* actions_out /* host [n_envs][4], or NULL */, int32_t* table_out /* host [n_envs][k C][4], or NULL */);
int orl_batch_core_table_shape(const orl_batch* b, int32_t* rows, int32_t* width, int32_t* pitch);

/* Block actions: DeepRMSA's (path, free block) action space for every slot-map family.  The rules above hand the agent a rule's
 * single winner per row; the path features show it the first j free blocks that fit.  Here the agent ACTS in those terms: "row r,
 * block b" = take the b-th fitting block of that row, a Discrete(R j + 1) space in which every set column provisions and the agent
 * itself chooses where in the spectrum.  For the pending service of an env and every row r of orl_batch_path_features' row order —
 * R = k rows, r = p, for RMSA, DeepRMSA and RWA; R = k C rows, r = p C + c, for RMCSA:
 *   n(r), m(p), row(r), fits   those of orl_batch_route_spectrum (RMSA, DeepRMSA, RWA) and of orl_batch_route_cores (RMCSA:
 *              modulation = -1 is m*(p), the best within reach; modulation = m is m where it is within both reach limits).  A path
 *              without a usable modulation, or p >= n_paths[src, dst], makes its rows unusable;
 *   blocks(r)  the maximal free runs of row(r) of length L >= n(r), in slot order: block b = (start_b, L_b).  A run that ends at slot
 *              S - 1 counts, as everywhere in these rules.
 * The table is int32 [n_envs][R][2 + 2 j] (ORL_BUF_BLOCK_TABLE): row r = (n(r), free(r), start_0, L_0, ..., start_{j-1}, L_{j-1}),
 * columns (S, 0) for a block that does not exist, (0, 0, S, 0, ...) for an unusable row, which loads no link row.  The device pitch
 * is round_up(R (2 + 2 j), 4) int32, the pad columns 0.
 * The mask is uint8 [n_envs][R j + 1] (ORL_BUF_BLOCK_MASK) at a device pitch of round_up(R j + 1, 16): column r j + b = 1 iff block b
 * of row r exists; the last column is the reject action, = allow_rejection; a row without a set column and allow_rejection == 0 gets
 * every other column set (the fallback of orl_batch_action_mask).  On a DeepRMSA batch with its own j it is that batch's
 * ORL_MASK_JOINT mask.
 * Selection: a flat index a per env, r = a / j and b = a % j, and a placement of the service in the block: */
#define ORL_BLOCK_FIRST 0 /* s = start_b: the block's lower end, DeepRMSA's decode */
#define ORL_BLOCK_LAST 1  /* s = start_b + L_b - n: the block's upper end */
/* The action written to the env's row of ORL_BUF_ACTIONS, where step(NULL) reads it: (p, s, 0, 0) for RMSA and RWA, (p, m(p), c, s) for
 * RMCSA; the family's reject row — (k, S, 0, 0), (k, M, C, S) — for a < 0, a >= R j or a block that does not exist.  Stepping any
 * other result provisions.  Selection recomputes from the slot maps; it does not read a table an earlier call left.
 * orl_batch_block_table: one launch on the batch's stream into ORL_BUF_BLOCK_TABLE and ORL_BUF_BLOCK_MASK; no atomics.  Each j has a
 * pair of buffers of its own, allocated by its first call.  orl_batch_select_blocks: one launch.  given == NULL: the index is column 0
 * of ORL_BUF_ACTIONS, where an agent on the GPU writes it; a host `given` [n_envs] int32 goes through a page-locked buffer of the batch
 * into a device buffer of the batch (both allocated by the first such call, this call's own), asynchronously on the batch's stream.
 * With all output pointers NULL and after the first call for that j the calls neither synchronise nor allocate: graph-capturable.
 * With an output pointer the rows are copied out densely and the call synchronises.  Env state, flags and snapshot bytes do not
 * change.
 * Families: the table and mask exist for RMSA, DeepRMSA, RWA and RMCSA; selection for RMSA, RWA and RMCSA (DeepRMSA steps block
 * indices natively).  ORL_E_INVALID, before anything is queued or allocated: another family, j outside 1 .. 8, a modulation other than
 * -1 outside RMCSA or outside -1 .. M - 1, a placement outside 0 .. 1, more rows than the kernel's LDS holds mask words for (R > 1534).
 * orl_batch_block_table_shape: *rows = R, *width = 2 + 2 j, the table's device pitch in int32, the mask's dim R j + 1 and pitch. */
int orl_batch_block_table_shape(const orl_batch* b, int j, int32_t* rows, int32_t* width /* 2 + 2j */, int32_t* table_pitch,
                                int32_t* mask_dim, int32_t* mask_pitch);
int orl_batch_block_table(orl_batch* b, int j, int modulation /* -1: each path's best */, int32_t* table_out /* host [n_envs][R][2 + 2j], or NULL */,
                          uint8_t* mask_out /* host [n_envs][R j + 1], or NULL */);
int orl_batch_select_blocks(orl_batch* b, int j, int modulation, int placement,
                            const int32_t* given /* host [n_envs], or NULL = column 0 of ORL_BUF_ACTIONS */,
                            int32_t* actions_out /* host [n_envs][4], or NULL */);

/* Release horizons: for how long each slot stays taken.  The views above describe where the spectrum is free; this one reads the other
 * half of the state — the pending releases of the env (what orl_batch_get_pending reads back one env at a time) and the holding time
 * of the pending service — on the device.  For env e with clock now (the arrival time of the pending service, column 0 of
 * orl_batch_get_services), every row r of orl_batch_path_features' row order (r = p; RMCSA: r = p C + c) and slot s:
 *   H[r][s] = float32(max over the pending releases v that cover (r, s) of release_time(v) - now), the subtraction in float64 and one
 *             rounding; 0.0f when no pending release covers it; -1.0f throughout a row whose path does not exist (p >=
 *             n_paths[src, dst])
 * v covers (r, s) when its path shares at least one link with path p of the pending pair, its core is c (RMCSA only) and slot(v) <= s <
 * slot(v) + max(n(v), 1) (an RWA record has n = 0 for its one wavelength).  H[r][s] is the time until slot s is free on every link of
 * the path if nothing else is provisioned: > 0 exactly where the AND of the path's link rows has the slot taken. */
#define ORL_HORIZON_SLOTS 0  /* float32 [n_envs][R S + 1]: row r at columns r S .. r S + S - 1; the last column is the pending service's
                              * holding time as float32; j must be 1 and modulation -1 */
#define ORL_HORIZON_BLOCKS 1 /* float32 [n_envs][R 2 j + 1]: for block b < j of row r of orl_batch_block_table(j, modulation) columns
                              * r 2 j + 2 b and + 1 = (left, right) = (H[r][start_b - 1], H[r][start_b + L_b]); a neighbour beyond the
                              * spectrum's edge (start_b == 0, start_b + L_b == S) is +inf; (-1, -1) for a block that does not exist,
                              * -1 throughout a row the service cannot use; the last column is the holding time; j = 1 .. 8 */
/* The device pitch is round_up(dim, 4) floats, the pad columns 0 (ORL_BUF_RELEASE_HORIZONS).  One launch on the batch's stream, LDS
 * atomics only, no global atomics: with out == NULL and after a first call of at least that size the call neither synchronises nor
 * allocates — graph-capturable; with `out` the rows are copied out densely and the call synchronises.  Env state, flags and snapshot
 * bytes do not change.  ORL_E_INVALID, before anything is queued or allocated: QoSConstrainedRA (no slot maps), an unknown layout, j
 * outside 1 .. 8, ORL_HORIZON_SLOTS with j != 1 or a modulation, a modulation other than -1 outside RMCSA or outside -1 .. M - 1, rows
 * the kernel's LDS cannot hold.
 * orl_batch_release_horizons_shape: *rows = R, *width = S or 2 j, *dim = R width + 1, the device pitch in floats. */
int orl_batch_release_horizons_shape(const orl_batch* b, int layout, int j, int32_t* rows, int32_t* width, int64_t* dim, int64_t* pitch);
int orl_batch_release_horizons(orl_batch* b, int layout, int j, int modulation, float* out /* host [n_envs][dim], or NULL: stays on the device, no synchronisation */);

/* Network capacity: what the network of an env can still carry.  Every view above describes the pending service on the k candidate
 * paths of its own node pair; this one describes the env's whole slot map, for every ordered node pair and every bit-rate class.
 * RMSA, DeepRMSA, RWA and RMCSA.  For env e:
 *   pairs    an ordered pair (src, dst); its path p < n_paths[src, dst] has index pidx = (src N + dst) K + p, the index of the
 *            topology's path tables
 *   cores    C' = C for RMCSA, else 1
 *   m(pidx, c)  the AND of the path's link rows in core c, bits >= S clear; L(pidx, c) = its longest free run, F(pidx, c) = its
 *            number of free slots
 *   classes  RWA: n_cls = 1.  The others: n_cls = n_bit_rates, the rows of the batch's bit-rate table that br_idx of the pending
 *            service indexes (25 .. 100 Gb/s in the uniform mode, bit_rates in the discrete mode)
 *   need(pidx, r)  the slots a service of class r needs on the path: RWA 1; RMSA / DeepRMSA n_slots[r][the path's best modulation]
 *            (get_number_slots); RMCSA n_slots[r][m*], m* the modulation within both reach limits for the path's length and class
 *            r that needs the fewest slots, ties to the lowest index — the modulation orl_batch_complete_actions and
 *            orl_batch_route_cores use; no modulation within reach: the path cannot carry the class
 *   serviceable(pair, r)  some existing path p of the pair, in some core c, has need >= 1 and L(pidx, c) >= need(pidx, r) — the
 *            rule of the action masks (a start at S - n counts), not the off-by-one of the reference's first-fit loop */
#define ORL_CAPACITY_PATHS 0        /* int32 [n_envs][N N K C' 2]: row q = pidx C' + c (path-major within a pair, like every other
                                     * (path, core) table) at columns 2 q, 2 q + 1 = (L, F); (-1, -1) where the path does not exist
                                     * (p >= n_paths, the diagonal included) */
#define ORL_CAPACITY_SERVICEABLE 1  /* u8 0/1 [n_envs][N N n_cls]: column (src N + dst) n_cls + r = serviceable((src, dst), r); a pair
                                     * without paths has 0 in every class column */
#define ORL_CAPACITY_COUNTS 2       /* int32 [n_envs][n_cls + N N]: the first n_cls columns = per class the number of ordered pairs
                                     * with n_paths > 0 that are NOT serviceable; the next N N = per pair the number of serviceable
                                     * classes — the two marginals of the matrix above */
/* The device pitch is round_up(dim, 4) int32 or round_up(dim, 16) bytes, the pad columns 0.  Each layout has a device buffer of
 * its own (ORL_BUF_PATH_CAPACITY, ORL_BUF_SERVICEABLE, ORL_BUF_CAPACITY_COUNTS), allocated by its first call: a pointer taken after
 * one layout's call keeps showing that layout's rows.  One launch on the batch's stream (the first call of layout 1 or 2 also
 * builds the batch's static need table), one wavefront per env, no atomics: with out == NULL after a first call of that layout the
 * call neither allocates nor synchronises — graph-capturable; with `out` ([n_envs][dim] of the layout's type) the rows are copied
 * out densely and the call synchronises.  Env state, flags and snapshot bytes do not change.  ORL_E_INVALID, before anything is
 * queued or allocated: QoSConstrainedRA (no slot maps), an unknown layout, a topology whose N N K per-path array exceeds the
 * kernel's LDS.
 * orl_batch_network_capacity_shape: *rows, *width = (N N K C', 2), (N N, n_cls), (1, n_cls + N N); *dim = rows x width; the device
 * pitch in items. */
int orl_batch_network_capacity_shape(const orl_batch* b, int layout, int32_t* rows, int32_t* width, int64_t* dim, int64_t* pitch);
int orl_batch_network_capacity(orl_batch* b, int layout, void* out /* host [n_envs][dim] of the layout's type, or NULL */);

/* capacity_after: what each candidate placement of the PENDING service would leave the network — the class counts of
 * ORL_CAPACITY_COUNTS after the placement, for Q candidates per env in one launch, without a fork, a step or a second batch.  RMSA,
 * DeepRMSA, RWA and RMCSA; pidx, C', n_cls, need and serviceable are those of the network capacity above.  For env e with slot maps A:
 *   candidate  (row, s, n): row = p C' + c in the row order of orl_batch_path_features — path p of the pending service's pair, core c —
 *              and the window of slots [s, s + n).  PRESENT iff 0 <= row < k C', p < n_paths[pair], n >= 1, 0 <= s and s + n <= S
 *   A - cand   A with the slots s .. s + n - 1 taken on every link of path p in core c, whether they were free or not
 *   after(q)[r] = the ordered pairs with paths for which class r is NOT serviceable on A - cand_q
 *               = the first n_cls columns of ORL_CAPACITY_COUNTS evaluated on A - cand_q; -1 throughout for an absent candidate
 * Row Q, one past the last candidate, is the baseline on A itself: the first n_cls columns of ORL_CAPACITY_COUNTS of the same moment.
 * This is NOT "the counts of a forked env after its step": a step also runs the releases that fall due before the next arrival. */
#define ORL_AFTER_CLASSES 0 /* int32 [n_envs][(Q + 1) n_cls]: row q = after(q), row Q the baseline */
#define ORL_AFTER_TOTAL 1   /* int32 [n_envs][Q + 1]: the sum of row q over the classes; -1 for an absent candidate */
/* Candidate sources; whatever a table holds (a stale one is the caller's business) is validated on the device by the presence rule: */
#define ORL_AFTER_ROUTE 0   /* the table last written by orl_batch_route_spectrum (RMSA, RWA: ORL_BUF_ASSIGN_TABLE) or
                             * orl_batch_route_cores (RMCSA: ORL_BUF_CORE_TABLE): Q = k C', candidate q = (q, column 0, column 2) of
                             * row q; a row with column 0 >= S has no fit and is absent.  DeepRMSA has no such table: refused */
#define ORL_AFTER_BLOCKS 1  /* the table last written by orl_batch_block_table for this j (every family): Q = R j, candidate q = r j + b
                             * — the column order of the block mask, the index orl_batch_select_blocks decodes — with n = column 0
                             * of row r and s = start_b (placement ORL_BLOCK_FIRST) or start_b + L_b - n (ORL_BLOCK_LAST); a block
                             * with start_b >= S is absent */
#define ORL_AFTER_GIVEN 2   /* host candidates int32 [n_envs][Q][3] = (row, s, n), staged through a page-locked buffer of the batch
                             * like every other `given` (not graph-capturable) */
#define ORL_AFTER_MAX_Q 1024 /* the most candidates per env of one call; more (RMCSA with many cores and blocks) is refused */
/* The device pitch is round_up(dim, 4) int32, the pad columns 0.  Each layout has a device buffer of its own
 * (ORL_BUF_CAPACITY_AFTER_CLASSES, ORL_BUF_CAPACITY_AFTER_TOTAL).  One launch on the batch's stream (the first call also builds the
 * batch's static need table, if orl_batch_network_capacity has not), one wavefront per env, no global atomics, deterministic: with
 * out == NULL, after a first call of that (source, layout), the call neither allocates nor synchronises — graph-capturable for
 * ORL_AFTER_ROUTE and ORL_AFTER_BLOCKS; with `out` ([n_envs][dim] int32) the rows are copied out densely and the call synchronises.
 * Env state, flags, snapshot bytes and the tables read do not change.  j and placement are read for ORL_AFTER_BLOCKS only,
 * given / n_given_candidates for ORL_AFTER_GIVEN only (else NULL).  ORL_E_INVALID, before anything is queued or allocated:
 * QoSConstrainedRA, an unknown source, layout or placement, ORL_AFTER_ROUTE on DeepRMSA, a table that has never been written (the
 * message names the call to make first), j outside 1 .. 8, Q outside 1 .. ORL_AFTER_MAX_Q, a topology whose N N k per-path
 * array exceeds the kernel's LDS.
 * orl_batch_capacity_after_shape: *candidates = Q, *width = n_cls (ORL_AFTER_CLASSES) or 1; *dim = (Q + 1) x width; the device pitch
 * in int32. */
int orl_batch_capacity_after_shape(const orl_batch* b, int source, int j, int layout, int n_given_candidates, int32_t* candidates, int32_t* width,
                                   int64_t* dim, int64_t* pitch);
/* (*dim, *pitch) of the rows the last orl_batch_capacity_after of `layout` left in its device buffer — what ORL_BUF_CAPACITY_AFTER_*
 * hands out; (0, 0) before any call of that layout. */
int orl_batch_capacity_after_last(const orl_batch* b, int layout, int64_t* dim, int64_t* pitch);
int orl_batch_capacity_after(orl_batch* b, int source, int j, int placement, int layout, const int32_t* given /* host [n_envs][Q][3], or NULL */,
                             int n_given_candidates, int32_t* out /* host [n_envs][dim], or NULL: stays on the device, no synchronisation */);

/* Snapshot / restore of the complete simulation state of the batch (slot maps, pending releases, RNG, statistics,
 * counters).  The reference has no equivalent (no checkpointing); used for long PPO runs.  The per-env
 * rates (orl_batch_set_rates) are configuration and not part of it. */
int64_t orl_batch_state_bytes(orl_batch* b);
int orl_batch_get_state(orl_batch* b, void* out);
int orl_batch_set_state(orl_batch* b, const void* in);
/* The snapshot's format, so that a caller can address one env inside a get_state() buffer: returns the number of sections and,
 * for the first max_sections of them, row_bytes[s] = bytes per env of section s, in snapshot order (section s occupies
 * n_envs * row_bytes[s] bytes, env i at i * row_bytes[s]).  The sections: the scalar record, the pending service, the slot maps,
 * the pending releases (times, records), the random stream, the link statistics, the compactness sums, the soon list (times,
 * slots), then where the batch keeps them the bit-rate histograms, RWA's action marginals, the action histograms and the second
 * random stream of a reseeded batch. */
int orl_batch_state_layout(orl_batch* b, int64_t* row_bytes, int max_sections);

/* Fork env states on the device: for every p < n, env dst_idx[p] of `dst` becomes a copy of env src_idx[p] of `src` (NULL = dst
 * itself) — every per-env row a snapshot holds (orl_batch_state_layout), taken whole, so that right after the call the
 * destination's rows equal the source's byte for byte and the copy continues exactly as its source does under every step route,
 * given the same actions.  One source may feed many destinations.  The flag word of the env (ORL_E_OVERFLOW / bad action marks)
 * travels with the record, as with orl_batch_set_state.
 * flags & ORL_COPY_KEEP_RNG: the destination takes the source's network state, clock, counters, pending service and pending
 * releases but keeps its OWN random streams: its stream and, in a reseeded batch, its second stream, their positions and the
 * mark that the env was reseeded.  A lookahead child that shared its parent's stream would have seen the parent's future
 * arrivals.  The service id still comes from the source.
 * What does NOT travel: the traffic rates (configuration, as for orl_batch_set_state: orl_batch_get_rates of both batches is
 * unchanged; follow up with orl_batch_set_rates to fork across loads); the path column of ORL_POLICY_PATH_FF (ORL_BUF_PATHS) and
 * the actions / reward / done / info / terminal observation rows of the last step; the armed episode log; the info mode.
 * Afterwards the destination's observation (DeepRMSA) is rebuilt as by orl_batch_set_state.
 * Ordering: everything is queued on the destination's stream; between two batches that stream first waits for what is queued on
 * the source's, and the source's stream then waits for the copy, so later steps of the source cannot overtake the read.  The
 * call returns without waiting for the device (it waits only for its own previous upload of index arrays, which are host
 * arrays); it is not graph-capturable.
 * Refused with ORL_E_INVALID and a specific orl_last_error(), before anything is modified or queued: n < 0 (n == 0 is ORL_OK
 * and does nothing); a null index array with n > 0; an index outside its batch; a destination that occurs twice; inside one
 * batch, a destination that is also the source of another pair (pairs with src == dst are dropped as no-ops first: the kernel
 * is a single pass, a permutation goes through a scratch batch); batches on different devices; batches whose per-env layout
 * differs (family, topology sizes or path tables, spectrum, cores, j, event capacity, bit-rate table size and mode, histograms
 * on / off, QoS classes); one batch reseeded (it carries second streams) and the other not — orl_batch_reseed the other first,
 * an all-zero mask allocates the streams without reseeding an env; either batch's last device-resident run abandoned. */
#define ORL_COPY_KEEP_RNG 1
int orl_batch_copy_envs(orl_batch* dst, orl_batch* src /* NULL = dst */, int64_t n, const int64_t* src_idx, const int64_t* dst_idx,
                        uint32_t flags);
/* The index rules of orl_batch_copy_envs without a device (tests/test_copy_plan.py): the number of pairs that remain after
 * dropping the no-ops, or ORL_E_INVALID with the refusal in orl_last_error(). */
int orl_debug_copy_pairs_check(int64_t B_src, int64_t B_dst, int same_batch, int64_t n, const int64_t* src_idx, const int64_t* dst_idx);

/* Profiling aid: reads the whole slot-map array once with 8-B (width16 = 0) or 16-B (1) loads per lane and returns the
 * number of bytes read, so that rocprofv3's FETCH_SIZE can be calibrated on a known byte count. */
int64_t orl_batch_debug_stream_read(orl_batch* b, int width16);
/* Measurement aid (bench.py, roofline.peak_measured): what the HBM of GPU `device` delivers to plain streaming kernels of this
 * library, measured now with HIP events, best of `reps` launches over `bytes` bytes (>= 1 MiB): *read_gbs — 16 bytes per lane,
 * read only (the kernel of orl_batch_debug_stream_read); *copy_gbs — 16 bytes per lane, copied (read + write bytes counted). */
int orl_debug_stream_peak(int device, int64_t bytes, int reps, double* read_gbs, double* copy_gbs);
/* Specialisation: the persistent kernel with ONE configuration's sizes (topology, spectrum, traffic model, kernel form) as
 * compile-time constants — same source, same results, 5-12 % faster.  It is a small shared library of its own, built on first
 * use from csrc/orl_kernels.hip with the -D flags orl_batch_spec_flags() writes (hipcc --offload-arch=gfx950 -O3 -std=c++17
 * -ffp-contract=off -fPIC <flags> -shared; optical_rl_gym_amd/_build.py build_spec caches it under build/spec/ keyed by the
 * flags and the source hash) and attached with orl_batch_load_spec(), which compares every field with the batch and refuses
 * a mismatch.  orl_spec_flags_for() gives the same flags without a device (pre-building) for a large batch,
 * orl_spec_flags_for_batch() for a batch of n_envs: the kernel form is part of the flags, and batches of at most 12 288 envs of the
 * single-core families take the two-wavefront form (a control and a row wavefront per 8 envs).  All return the
 * string length, 0 when the configuration does not run the persistent kernel.  ORL_PERSIST_SPEC=0 in the environment keeps the
 * generic kernel. */
int orl_batch_spec_flags(orl_batch* b, char* buf, int capacity);
int orl_spec_flags_for(const orl_env_config* cfg, const orl_topology_desc* topo, char* buf, int capacity);
int orl_spec_flags_for_batch(const orl_env_config* cfg, const orl_topology_desc* topo, int64_t n_envs, char* buf, int capacity);
int orl_batch_load_spec(orl_batch* b, const char* so_path);
/* Whether the last orl_batch_run used the attached specialisation — 1: one wavefront per 8 envs, 2: its two-wavefront form (a control
 * and a row wavefront per 8 envs: batches of at most 12 288 envs) — or the generic persistent kernel (0); -1 = another step form. */
int orl_batch_debug_persist_spec(orl_batch* b);
/* The form of the persistent kernel the last orl_batch_run launched (what lives in its LDS window / how the row statistics are
 * done): 0-6 the forms with the row phase in the loop, 7 / 8 the rows-deferred forms (round 6: the loop logs events,
 * k_rowstats replays the link statistics after the launch); -1 = no device-resident run through the persistent kernel yet. */
int orl_batch_debug_persist_form(orl_batch* b);
/* The whole choice the launcher of the persistent kernel makes for a batch of n_envs envs of this configuration, without a
 * device (tests/test_persist_choice.py): out[0..8] = form number, the kernel's LDS template argument, waves per SIMD, the
 * two-wavefront form, row-cache level, release times in LDS, bytes of the LDS window, bytes of LDS the launch asks for, workgroups
 * per CU.  `tuned`: the choice made when a specialisation library is attached.  The ORL_PERSIST_* overrides are read from the
 * environment as at a launch.  Returns 9, or 0 when the configuration does not run the persistent kernel. */
int orl_debug_persist_choice(const orl_env_config* cfg, const orl_topology_desc* topo, int64_t n_envs, int tuned, int32_t* out);
/* The host-side decisions for a batch of n_envs envs of this configuration, without a device (tests/test_run_plan.py).  The step
 * route taken at creation: out[0..4] = device-resident runs through the persistent kernel, the two-kernel form (ORL_ALT_IMPLS
 * builds), host-driven steps through k_agent, DevParams::item_masks, DevParams::rel_limit.  The plan of a device-resident run of
 * n_steps steps on a GPU of n_cu CUs, for a batch whose statistics log holds log_cap_have steps, whose workgroups stand at step
 * run_base and whose last run did not complete (wg_dirty): out[5..10] = steps per launch, parts (1, or 2: two halves on two
 * streams), envs of the first half, steps the statistics log must hold, events per env the event log must hold (0 unless the
 * chosen form is rows-deferred), step counters cleared first; zeros where the persistent kernel does not serve the batch.
 * `tuned` as for orl_debug_persist_choice.  Every override is read from the environment as at creation / at a run.  Returns 11,
 * or 0 for an invalid configuration. */
int orl_debug_run_plan(const orl_env_config* cfg, const orl_topology_desc* topo, int64_t n_envs, int64_t n_steps, int tuned, int n_cu,
                       int log_cap_have, int64_t run_base, int wg_dirty, int32_t* out);
/* The shape of a per-step view's rows and the geometry of its launch (csrc/orl_view_plan.h) without a device or a configuration
 * (tests/test_view_plan.py), from raw sizes: the env family, the row width W in 64-bit words (1, 2, 5 or 8), the batch B and the
 * sizes N, E, K, C, S, J, M of a batch, all >= 1.  view: 0 action mask, 1 RMCSA mask, 2 action completion, 3 spectrum assignment,
 * 4 path features, 5 link features, 6 MatrixObservationWithPaths, 7 routing rules, 8 core and spectrum rules (RMCSA only); arg: the mask layout (ORL_MASK_*), the rule (ORL_ASSIGN_*), the
 * path features' j.  out[0..4] = row length (0: the family has no such layout), blocks per row, values per block, device pitch in
 * elements, bytes per element; out[5..12] = accepted (0: the call refuses the shape, the rest 0), wavefronts and threads per
 * workgroup, grid, dynamic LDS bytes, path features staged in LDS, link features' slot rows per round (0: whole rows), assignment
 * with occupancy counts.  Returns 13, or 0 for arguments outside every batch. */
int orl_debug_view_plan(int env_type, int W, int64_t B, int N, int E, int K, int C, int S, int J, int M, int view, int arg, int32_t* out);
/* The same for the release horizons (csrc/orl_view_plan.h, horizon_plan; tests/test_release_horizons.py), which take a layout
 * (ORL_HORIZON_*) and a j: out[0..3] = row length (0: no such rows), rows, values per row, device pitch in floats; out[4..9] = accepted
 * (0: the call refuses the shape, the rest 0), wavefronts and threads per workgroup, grid, dynamic LDS bytes, rows of H per round.
 * Returns 10, or 0 for arguments outside every batch. */
int orl_debug_horizon_plan(int env_type, int W, int64_t B, int N, int E, int K, int C, int S, int M, int layout, int j, int32_t* out);
/* The same for the network capacity (csrc/orl_view_plan.h, capacity_plan; tests/test_network_capacity.py): out[0..3] = row length
 * (0: no such rows), rows, width, device pitch in items; out[4..10] = accepted (0: the call refuses the shape), wavefronts and threads
 * per workgroup, grid, dynamic LDS bytes of a workgroup, slot maps staged in LDS, LDS bytes of one wavefront (= one env).  Returns
 * 11, or 0 for arguments outside every batch. */
int orl_debug_capacity_plan(int env_type, int W, int64_t B, int N, int E, int K, int C, int S, int M, int n_br, int layout, int32_t* out);
/* The same for capacity_after (csrc/orl_view_plan.h, capacity_after_plan; tests/test_capacity_after.py) with Q candidates: the same
 * eleven values; out[1] = Q + 1 rows.  Returns 11, or 0 for arguments outside every batch. */
int orl_debug_capacity_after_plan(int env_type, int W, int64_t B, int N, int E, int K, int C, int S, int M, int n_br, int layout, int Q, int32_t* out);
/* Test aid: rows of H per round for the release horizons of this batch (0: what the plan says; more than the plan's: the plan's), so
 * that a small shape runs in several rounds. */
int orl_debug_set_horizon_rows(orl_batch* b, int rows);
/* Which kernel orl_batch_step launches for this batch: 2 = k_agent (8 lanes per env, the persistent kernel's phases for one
 * step; QoSConstrainedRA: k_agent_qos, from 20 480 envs), 0 = k_step (one wavefront per env). */
int orl_batch_debug_step_kernel(orl_batch* b);
/* Statistics: env-steps whose releases took the serial tail (more than 8 of one step meeting on one link). */
int64_t orl_batch_debug_serial_count(orl_batch* b);
/* Diagnostic builds with -DORL_TIMING only (zeros otherwise): shader-clock cycles per phase of the persistent kernel, 48
 * slots summed over wavefronts (0-15 control phase, 16-31 release detection, 32-47 row phase). */
int orl_batch_debug_prof(orl_batch* b, uint64_t* out48, int reset);
/* 1 when the library was built with -DORL_ALT_IMPLS (the two-kernel form of the persistent kernel's phases, used by
 * the cross-implementation tests), else 0. */
int orl_build_has_alt(void);

#ifdef __cplusplus
}
#endif
#endif /* ORL_H */
