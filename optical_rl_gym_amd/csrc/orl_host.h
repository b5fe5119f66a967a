// orl_host.h — host-side structures shared by the translation units of liborlgpu.so.
//
// The library is built from one W-independent unit (orl_api.hip: the C ABI of include/orl.h, batch construction, the small
// utility kernels) and one unit per row width W in {1, 2, 5, 8} 64-bit words (orl_kernels.hip compiled with -DORL_W=W: the
// env kernels, which keep a whole link row in registers and are therefore templates over W).  The units compile in
// parallel (optical_rl_gym_amd/_build.py); the API unit reaches the kernels through the launchers declared below.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/orl.h"
#include "orl_device.h"

// Deferred statistics of the persistent kernel (orl_device_split.h ctrl_phase<..., DS>, orl_kernels.hip k_stats): the per-env
// bookkeeping of a launch is logged and replayed lane-per-env afterwards (RMSA, DeepRMSA, RWA, RMCSA).  -DORL_PERSIST_DS=0 keeps
// it in the loop.
#ifndef ORL_PERSIST_DS
#define ORL_PERSIST_DS 1
#endif
#ifndef ORL_PERSIST_SVC
#define ORL_PERSIST_SVC 1
#endif
static inline bool orl_persist_deferred(int env_type) {
  return ORL_PERSIST_DS != 0 && ORL_PERSIST_SVC != 0 &&
         (env_type == orl::ENV_RMSA || env_type == orl::ENV_DEEPRMSA || env_type == orl::ENV_RWA || env_type == orl::ENV_RMCSA);
}

struct PersistChoice;  // orl_persist_form.h

struct orl_topology {
  int device;
  int N, E, K, H, M;
  std::vector<int32_t> h_hops, h_links, h_mod;  // host copies (per-batch derived tables are built from them)
  int* n_paths;
  double* path_length;
  int* edge_iter_order;
  int* link_pos;
};

// per-kernel timing (orl_batch_run, time_kernels == 1): an event after every launch
struct TkRec { std::vector<hipEvent_t> ev; std::vector<const char*> name; };

// A host `given` on its way to the device (stage_given, orl_api.hip): the device buffer a kernel reads it from, the page-locked
// buffer it is copied through, and the event behind the last upload out of that one — the next call waits for it before it refills
// the buffer.  All three allocated on first use.
struct GivenStage { int32_t* dev = nullptr; int32_t* host = nullptr; hipEvent_t up = nullptr; };

struct orl_batch {
  orl::DevParams P;
  TkRec* tk = nullptr;
  int parity = 0;        // two-kernel form (ORL_ALT_IMPLS): which deferred-env buffer the next step writes
  int persist = 0;       // device-resident runs go through the persistent kernel (k_persist)
  int agent_step = 0;    // host- / agent-driven steps with auto reset go through k_agent (the phases of k_persist) instead of k_step
  int two_kernel = 0;    // ORL_ALT_IMPLS builds, ORL_STEP_IMPL=2 ORL_PERSIST=0: the phases of k_persist as separate launches
  int64_t persist_launches = 0;
  int persist_spec = 0;            // 1: the last launch of k_persist used the instantiation built for this configuration
  int persist_form_last = -1;      // the form (index into kPersistForms, orl_persist_form.h) of the last launch of k_persist
  // a specialisation library attached by orl_batch_load_spec: k_persist with this batch's sizes as compile-time constants
  void* spec_handle = nullptr;
  void (*spec_launch)(const orl::DevParams*, unsigned, size_t, hipStream_t, int, int, int*, unsigned int*, unsigned int*) = nullptr;
  void (*spec_agent_launch)(const orl::DevParams*, unsigned, size_t, hipStream_t, int, int) = nullptr;  // k_agent of the same library
  int spec_lds = -1, spec_waves = -1, spec_rw = -1;  // the form it was built for: k_persist's LDS argument, waves per SIMD, two-wavefront form
  int* d_wg_step = nullptr;        // [ceil(B/8)] steps each workgroup of the persistent kernel has completed since run_base was 0
  int64_t run_base = 0;            // ... all of them, between runs (no per-run clearing of d_wg_step)
  bool wg_dirty = true;            // a run did not complete (or none has run yet): clear d_wg_step and run_base first
  bool run_abandoned = false;      // a device-resident run returned early (HIP error): services may be parked, envs at different steps
  int un_slot[2] = {0, 0};         // per half of the batch: the slot of d_unfinished its next launch counts into
  // per half p and slot s, at 8 p + 4 s: [0] straggler workgroups of a persistent launch, [1] OR of the env flag words
  // (k_finish2); a launch counts into one slot and clears the other for the launch after it (no memset between launches);
  // [16..17]: the same pair for report_flags
  unsigned int* d_unfinished = nullptr;
  int device = 0, wt = 0;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;   // second half of the batch in device-resident runs (see orl_batch_run)
  hipEvent_t ev_half = nullptr;
  int n_cu = 256;
  std::vector<void*> allocs;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  unsigned long long* d_totals = nullptr;
  int32_t* h_actions = nullptr;    // page-locked [B][4]: where orl_batch_step_async expands the caller's compact action rows
  int step_pending = 0;            // orl_batch_step_async queued a step that orl_batch_step_wait has not collected yet
  unsigned int* h_tail = nullptr;  // page-locked: where the straggler count / flag words of a run land (a pageable target is staged)
  int cache_epoch = 1;             // bumped by every call that may change slot maps outside the persistent kernel (DevParams::row_cache_key)
  long long* gather_idx = nullptr;  // orl_batch_get_info_rows: row indices and gathered rows on the device, grown on demand
  double* gather_out = nullptr;
  int64_t gather_cap = 0;
  float* obs_f32 = nullptr;        // device copy of the observation array in float32 (orl_batch_get_obs_f32), allocated on first use
  int* ep_buf = nullptr;           // episode log buffer (orl_batch_episode_log): [B][ep_alloc] ints, armed with stride P.ep_cap <= ep_alloc
  int ep_alloc = 0;
  double* ep_rew_buf = nullptr;    // QoSConstrainedRA: the float64 reward sums beside it, same shape
  unsigned char* mask_buf[4] = {nullptr, nullptr, nullptr, nullptr};  // action masks per layout (ORL_MASK_*): [B][pitch] bytes, allocated
                                   // by the first orl_batch_action_mask of that layout (a view of one stays that layout's)
  // host `given`s: [0] ORL_MASK_CORE_SLOT's (path, modulation) pairs [B][2], [1] orl_batch_complete_actions' prefixes [B][n_given <= 3]
  // (capacity [B][3]), [2] orl_batch_assign_spectrum's paths [B], [3] orl_batch_route_cores' (path, core) prefixes [B][n_given <= 2]
  // (capacity [B][2]).  One stage per call on purpose: each may refill its staging buffer without waiting for another's upload.
  // [4] orl_batch_select_blocks' block indices [B].
  enum { GIVEN_MASK, GIVEN_COMPLETE, GIVEN_ASSIGN, GIVEN_ROUTE_CORES, GIVEN_BLOCKS, GIVEN_STAGES };
  GivenStage given[GIVEN_STAGES];
  int mask_last = -1;              // layout of the last launch: what ORL_BUF_ACTION_MASK hands out (-1: none yet)
  float* pf_buf[9] = {};           // path features per block count j (1 .. 8): [B][pitch] floats, allocated by the first
                                   // orl_batch_path_features of that j (a view of one stays that j's)
  int pf_last = 0;                 // j of the last launch: what ORL_BUF_PATH_FEATURES hands out (0: none yet)
  float* lf_buf = nullptr;         // link features: [B][pitch] floats, allocated by the first orl_batch_link_features; what
                                   // ORL_BUF_LINK_FEATURES hands out
  unsigned char* qobs_buf = nullptr;  // MatrixObservationWithPaths (QoSConstrainedRA): [B][pitch] bytes, allocated by the first
                                    // orl_batch_matrix_paths_observation; what ORL_BUF_MATRIX_PATHS_OBS hands out
  int32_t* route_table = nullptr;  // the per-path assignment table: [B][4 K] int32, allocated by the first orl_batch_route_spectrum; what
                                   // ORL_BUF_ASSIGN_TABLE hands out
  int32_t* core_table = nullptr;   // RMCSA's (path, core) table: [B][4 K C] int32, allocated by the first orl_batch_route_cores; what
                                   // ORL_BUF_CORE_TABLE hands out
  int32_t* bt_buf[9] = {};         // block tables per block count j (1 .. 8): [B][pitch] int32, and their masks [B][pitch] bytes, both allocated
  unsigned char* bk_buf[9] = {};   // by the first orl_batch_block_table of that j (a view of one stays that j's)
  int bt_last = 0;                 // j of the last launch: what ORL_BUF_BLOCK_TABLE and ORL_BUF_BLOCK_MASK hand out (0: none yet)
  float* rh_buf = nullptr;         // release horizons: [B][pitch] floats of the last orl_batch_release_horizons, rh_cap bytes; allocated by
  size_t rh_cap = 0;               // the first call, replaced by a larger one when a call needs more; what ORL_BUF_RELEASE_HORIZONS
  int64_t rh_pitch = 0;            // hands out, at the last call's pitch (0: none yet)
  int rh_rows = 0;                 // orl_debug_set_horizon_rows: rows of H per round (0: the plan's)
  void* cap_buf[3] = {};           // network capacity: [B][pitch] rows per layout (ORL_CAPACITY_*), each allocated by that layout's first call
  unsigned char* cap_need = nullptr;  // need(pidx, r), static per batch: [N N][n_cls][round_up(K, 8)] bytes, built by the first call that reads it
  int32_t* ca_buf[2] = {};         // capacity_after: [B][pitch] int32 rows per layout (ORL_AFTER_*), ca_cap bytes; allocated by the layout's first
  size_t ca_cap[2] = {};           // call, replaced by a larger one when a call has more candidates; what ORL_BUF_CAPACITY_AFTER_* hand out,
  int64_t ca_pitch[2] = {};        // at the last call's pitch (0: none yet); ca_dim: that call's row length, (Q + 1) x width
  int64_t ca_dim[2] = {};
  GivenStage ca_given;             // its host candidates [B][Q][3]: as `given`, but of ca_given_cap bytes, replaced when a call needs more
  size_t ca_given_cap = 0;
  // orl_batch_copy_envs (as the destination): the pair indices [2][n] on the device and in page-locked memory, grown on demand
  long long* copy_idx = nullptr;
  long long* h_copy_idx = nullptr;
  int64_t copy_cap = 0;
  hipEvent_t ev_copy_up = nullptr;  // behind the last upload out of h_copy_idx: the next call waits for it before it refills the buffer
  hipEvent_t ev_copy = nullptr;     // cross-batch copies: orders this batch's stream with the other's (as source: behind what it queued;
                                    // as destination: behind the copy)
  uint64_t topo_hash = 0;           // FNV-1a of the topology's sizes and path tables (hops, links, modulations): copy_envs compares it
};

// Anything but the row-cache-keeping forms of the persistent kernel is about to write slot maps: the row caches the persistent
// kernel left with the state (DevParams::row_cache) no longer describe them.  The key of the next persistent launch differs from
// every stored stamp.
static inline void slot_maps_change(orl_batch* b, hipStream_t st) {
  if (++b->cache_epoch >= (1 << 22)) {  // (the key keeps 22 bits of it: start over with no stamp left standing)
    if (b->P.row_cache_stamp) hipMemsetAsync(b->P.row_cache_stamp, 0, (size_t)((b->P.B + 7) / 8) * sizeof(int), st);
    b->cache_epoch = 1;
  }
}

#define ORL_TK(B_, NAME)                                                                 \
  do {                                                                                   \
    if ((B_)->tk) {                                                                      \
      hipEvent_t e_;                                                                     \
      hipEventCreate(&e_);                                                               \
      hipEventRecord(e_, (B_)->stream);                                                  \
      (B_)->tk->ev.push_back(e_);                                                        \
      (B_)->tk->name.push_back(NAME);                                                    \
    }                                                                                    \
  } while (0)

// ---- launchers, one explicit instantiation per W (orl_kernels.hip) ----------------------------------------------------
namespace orl_launch {
template <int W> void reset(orl_batch* b, int full, const unsigned char* dmask);
template <int W> void policy(orl_batch* b, int pol);                       // stand-alone slot scan -> P.actions
template <int W> void step64(orl_batch* b, int auto_reset, int want_info, int fused_policy);  // one wavefront per env
template <int W> void obs(orl_batch* b, int with_terminal);                // DeepRMSA observation
// The views of the pending service: each launches what view_plan (orl_view_plan.h) says, into rows of view_shape's pitch.  A plan
// that is not ok is the caller's to refuse before it allocates or queues anything.
template <int W> void action_mask(orl_batch* b, int layout, unsigned char* out);  // k_action_mask -> out [B][pitch]
// k_rmcsa_mask -> out [B][pitch]; given: device (path, modulation) of env e at given[e * gstride + 0 / 1]
template <int W> void rmcsa_mask(orl_batch* b, int layout, unsigned char* out, const int* given, int gstride);
// k_rmcsa_complete: the first n_given action columns of env e at given[e * gstride ...] (device) completed first-fit into P.actions
template <int W> void rmcsa_complete(orl_batch* b, int n_given, const int* given, int gstride);
// k_assign_spectrum: the path of env e at given[e * gstride] (device; n_given == 0: all paths) and its first slot under `rule` into P.actions
template <int W> void assign_spectrum(orl_batch* b, int rule, int n_given, const int* given, int gstride);
// k_route_spectrum: every path's winner under `rule` -> table [B][K][4] (device), the action under `route` into P.actions
template <int W> void route_spectrum(orl_batch* b, int rule, int route, int32_t* table);
// k_route_cores: every (path, core) pair's winner under `rule` -> table [B][K C][4] (device), the action under `route` over the pairs
// the prefix admits (path at given[e * gstride], core at given[e * gstride + gcore]) into P.actions
template <int W> void route_cores(orl_batch* b, int rule, int route, int modulation, int n_given, const int* given, int gstride, int gcore, int32_t* table);
template <int W> void path_features(orl_batch* b, float* out, int j, int mod);  // k_path_features -> out [B][pitch] floats
// k_block_table -> table [B][pitch] int32 and mask [B][pitch] bytes (device); k_select_blocks: the index of env e at given[e * gstride]
// (device) -> its row of P.actions
template <int W> void block_table(orl_batch* b, int32_t* table, unsigned char* mask, int j, int mod);
template <int W> void select_blocks(orl_batch* b, int j, int mod, int placement, const int* given, int gstride);
template <int W> void link_features(orl_batch* b, float* out);             // k_link_features -> out [B][pitch] floats
// k_release_horizons -> out [B][pitch] floats in `layout` (ORL_HORIZON_*), in rounds of min(rows, the plan's) rows (0: the plan's)
template <int W> void release_horizons(orl_batch* b, float* out, int layout, int j, int mod, int rows);
// k_network_capacity -> out [B][pitch] of the layout's type (ORL_CAPACITY_*); need: the batch's need table (null for ORL_CAPACITY_PATHS)
template <int W> void network_capacity(orl_batch* b, void* out, const unsigned char* need, int layout);
template <int W> void capacity_need(orl_batch* b, unsigned char* need);  // k_capacity_need -> need [N N][n_cls][round_up(K, 8)]
// k_capacity_after -> out [B][pitch] int32 in `layout` (ORL_AFTER_*) for the Q candidates per env of `tab` (tstride int32 per env) of `source`
template <int W> void capacity_after(orl_batch* b, int* out, const unsigned char* need, const int* tab, int tstride, int source, int j, int placement, int Q,
                                     int layout);
// k_persist in the form `ch` (the run's choice for the whole batch; use_spec: made for the attached specialisation library) over the
// env range of view VP up to step `target` of this run, then k_rel_tail, on stream st
template <int W> void persist(orl_batch* b, const orl::DevParams& VP, const PersistChoice& ch, bool use_spec, hipStream_t st, int pol, int target,
                              int* wg_step, unsigned int* unfinished, unsigned int* clear_next, int finish);  // finish: this launch ends the run (DevParams::persist_finish)
template <int W> int prof_read(unsigned long long* out48, int reset);      // -DORL_TIMING builds: per-phase cycle sums
template <int W> void step2(orl_batch* b, int pol);                        // ORL_ALT_IMPLS: k_step_a2 ; k_rows2 ; k_rel_tail
template <int W> void agent_step(orl_batch* b, int auto_reset, int pol);   // k_agent: one step, actions in P.actions, info / obs written
}  // namespace orl_launch

#define ORL_DISPATCH_W(B_, CALL)      \
  switch ((B_)->wt) {                 \
    case 1: CALL(1); break;           \
    case 2: CALL(2); break;           \
    case 5: CALL(5); break;           \
    default: CALL(8); break;          \
  }
