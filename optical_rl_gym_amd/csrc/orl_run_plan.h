// orl_run_plan.h — the host-side decisions around the kernels: which kernels serve a batch's steps (the step route, taken once at
// creation) and how a device-resident run through the persistent kernel is cut into launches (the run plan, made once per run).
//
// Like the form choice (orl_persist_form.h) both are pure functions of the batch's sizes and of their overrides, which ONE reader
// each takes from the environment (step_overrides_from_env, run_overrides_from_env): tests/test_run_plan.py pins them case by
// case without a device (orl_debug_run_plan).  No HIP call in here.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <optional>

#include "orl_persist_form.h"

// ---- the step route ----------------------------------------------------------------------------------------------------
// Cross-checks and test knobs: one field per environment variable, empty where it is not set (or set outside its range).
struct StepOverrides {
  std::optional<int> step_impl;   // ORL_STEP_IMPL: 64 = the per-env kernel; 2 (with ORL_PERSIST=0, ORL_ALT_IMPLS builds) = the two-kernel form
  std::optional<int> persist;     // ORL_PERSIST: 0 = no persistent kernel
  std::optional<int> agent_step;  // ORL_AGENT_STEP: 1 = k_agent at any batch size (parity tests), 0 = never
  std::optional<int> item_masks;  // ORL_ITEM_MASKS, 1..ORL_IMASKS: a smaller limit sends far more env-steps through the serial tail
                                  // (and, RMCSA, the tally pass)
};
// Read once, when a batch is created.
static inline StepOverrides step_overrides_from_env() {
  StepOverrides o;
  if (const char* e = getenv("ORL_STEP_IMPL")) o.step_impl = atoi(e);
  if (const char* e = getenv("ORL_PERSIST")) o.persist = atoi(e);
  if (const char* e = getenv("ORL_AGENT_STEP")) o.agent_step = atoi(e);
  if (const char* e = getenv("ORL_ITEM_MASKS")) { const int v = atoi(e); if (v >= 1 && v <= ORL_IMASKS) o.item_masks = v; }
  return o;
}
struct StepRoute {
  int persist;     // device-resident runs go through the persistent kernel (k_persist)
  int two_kernel;  // ORL_ALT_IMPLS builds: the phases of k_persist as separate launches
  int agent_step;  // host- / agent-driven steps go through k_agent (QoSConstrainedRA: k_agent_qos) instead of k_step
  int item_masks;  // DevParams::item_masks
  int rel_limit;   // DevParams::rel_limit
};
// `pipeline_ok`: the persistent kernel's 8-lanes-per-env slot scan applies to the configuration (pipeline_applies, orl_api.hip).
// P.B is the batch.
static inline StepRoute step_route(const orl::DevParams& P, bool pipeline_ok, const StepOverrides& ov) {
  const bool qos = P.env_type == orl::ENV_QOS;
  const bool per_env = ov.step_impl && *ov.step_impl == 64;
  StepRoute r;
  // The persistent kernel (k_persist) serves the device-resident loop wherever its 8-lanes-per-env slot scan applies
  // (k <= 8 paths, release slots indexed with 8 + 3 bits): cfg2 64 envs 2.6e6 vs 2.1e6 env-steps/s for the per-env kernel;
  // 4 096: 1.6e8 vs 7.6e7; 32 768: 6.3e8 vs 4.0e8; RWA 4 096: 2.4e8 vs 8.3e7.  ORL_STEP_IMPL=64 forces the per-env kernel
  // (cross-checks); ORL_STEP_IMPL=2 with ORL_PERSIST=0 selects the two-kernel form in ORL_ALT_IMPLS builds.
  r.persist = pipeline_ok && !per_env;
  r.two_kernel = 0;
  if (ov.persist && *ov.persist == 0 && r.persist) {
    r.persist = 0;
    r.two_kernel = (kPersistAltBuild && ov.step_impl && *ov.step_impl == 2) ? 1 : 0;
  }
  // Host- / agent-driven steps with auto reset (what SB3's VecEnv issues) through the phases of the persistent kernel
  // (k_agent) wherever they apply and the batch is large enough to fill the GPU with 8 envs per wavefront: cfg2 65 536 envs
  // 305 us per step in k_step (one wavefront per env), ~90 us in k_agent.  ORL_AGENT_STEP=1 forces it for any batch size
  // (parity tests), 0 disables it.
  // (QoSConstrainedRA, which no persistent kernel serves, has its own 8-lanes-per-env step kernel, k_agent_qos: its releases
  // are found by 8 lanes scanning the env's release times where k_step has 64, a longer chain per step that pays once the
  // batch fills the GPU — 65 536 envs 120 against 225 us per step, 32 768: 77 / 109, 16 384: 65 / 66, 4 096: 47 / 33)
  const bool fits = (r.persist && P.E <= 128) || (qos && P.K <= 8 && !per_env);
  r.agent_step = fits && P.B >= (qos ? 20480 : 2048);
  if (ov.agent_step) r.agent_step = fits && *ov.agent_step != 0;
  r.item_masks = ov.item_masks.value_or(ORL_IMASKS);
  r.rel_limit = ov.item_masks.value_or(31);
  return r;
}

// ---- the run plan ------------------------------------------------------------------------------------------------------
// A/B measurements and test knobs; a value outside its range is ignored.
struct RunOverrides {
  std::optional<int> chunk;               // ORL_PERSIST_CHUNK, >= 1: steps per launch
  std::optional<int> parts;               // ORL_PERSIST_PARTS, 1 | 2: the batch as one launch per chunk, or as two halves on two streams
  std::optional<int> log_cap;             // ORL_LOG_CAP, 2..256: steps the statistics log of a launch holds per wavefront (tests)
  std::optional<int> elog_cap;            // ORL_ELOG_CAP, 34..4096: events per env the event log of a launch holds (tests: wavefronts
                                          // stop for a full event log)
  std::optional<int64_t> run_base_limit;  // ORL_RUN_BASE_LIMIT, >= 1: where the step counters start over (tests)
};
// Read once per device-resident run.
static inline RunOverrides run_overrides_from_env() {
  RunOverrides o;
  if (const char* e = getenv("ORL_PERSIST_CHUNK")) { const int v = atoi(e); if (v >= 1) o.chunk = v; }
  if (const char* e = getenv("ORL_PERSIST_PARTS")) { const int v = atoi(e); if (v == 1 || v == 2) o.parts = v; }
  if (const char* e = getenv("ORL_LOG_CAP")) { const int v = atoi(e); if (v >= 2 && v <= 256) o.log_cap = v; }
  if (const char* e = getenv("ORL_ELOG_CAP")) { const int v = atoi(e); if (v >= 34 && v <= 4096) o.elog_cap = v; }
  if (const char* e = getenv("ORL_RUN_BASE_LIMIT")) { const long long v = atoll(e); if (v >= 1) o.run_base_limit = v; }
  return o;
}
struct RunPlan {
  int chunk;            // steps per launch
  int parts;            // 1: one launch per chunk; 2: the batch as two halves on two streams
  int64_t half;         // envs of the first half (a multiple of 8: wavefronts own 8 consecutive envs); the batch where parts == 1
  int log_cap;          // steps per wavefront the statistics log must hold (DevParams::slog); `log_cap_have` where that is enough
  int elog_cap;         // events per env the event log must hold (DevParams::elog); 0 unless the chosen form is rows-deferred
  bool clear_counters;  // the per-workgroup step counters and run_base start over in front of this run
};
// The logs of a launch of the persistent kernel (deferred statistics: 24 bytes per env-step, DevParams::slog; rows-deferred forms:
// 16 bytes per provision / release, DevParams::elog) are sized for the launches the run makes — `chunk` steps each, a wavefront
// that left a launch early catching up over at most two chunks — instead of the 256 steps' worth every batch used to get at
// creation (404 MB per 65 536-env batch whether it ever ran a device loop or not).  Each log stays below 1 GiB: larger batches
// run shorter launches.  A later run with longer launches replaces them (ensure_logs, orl_api.hip).
// `ch`: the form chosen for the whole batch P.B; `log_cap_have`, `run_base`, `wg_dirty`: the batch's state in front of the run.
static inline RunPlan run_plan(const orl::DevParams& P, const PersistChoice& ch, int n_cu, int64_t n_steps, int log_cap_have, int64_t run_base,
                               bool wg_dirty, const RunOverrides& ov) {
  RunPlan r;
  const int64_t n_wg = (P.B + 7) / 8;
  // d_wg_step counts steps since run_base was 0: between runs every workgroup stands at run_base, so a run needs no clearing
  // (a fill kernel in front of every run: ~1 % of a 20-step run) until the counters, which are ints, would run over
  r.clear_counters = wg_dirty || run_base + n_steps > ov.run_base_limit.value_or((int64_t)1 << 30);
  // (launches of 128 steps: every launch boundary costs a wavefront its window fill / write-back and a cold first step —
  // cfg2 1.265e9 with 64-step launches, 1.295e9 with 128; with the bit-word sink a wavefront practically never has to
  // leave its loop early, so longer launches leave no stragglers behind)
  r.chunk = ov.chunk.value_or(128);
  r.log_cap = log_cap_have;
  r.elog_cap = 0;
  if (orl_persist_deferred(P.env_type)) {
    const size_t B = (size_t)P.B;
    size_t want = (n_steps <= r.chunk) ? (size_t)(n_steps > 0 ? n_steps : 1) : (size_t)2 * r.chunk;
    const size_t per_step = (size_t)ORL_SLOG_ROW_WORDS * 8 * B;
    size_t most = ((size_t)1 << 30) / per_step;
    most = most > 256 ? 256 : (most < 2 ? 2 : most);
    if (want > most) want = most;
    if (want < 2) want = 2;
    if (ov.log_cap) want = (size_t)*ov.log_cap;
    if ((size_t)log_cap_have < want) r.log_cap = (int)want;
    // (a launch logs at most log_cap steps per wavefront, a straggler up to two chunks)
    if (n_steps > r.log_cap && r.chunk > r.log_cap / 2) r.chunk = r.log_cap / 2 > 0 ? r.log_cap / 2 : 1;
    // events: a step logs its provision and its releases, two per step on average; a wavefront whose envs' logs cannot take
    // another step stops early like one that used up the statistics log
    if (kPersistForms[ch.form].rd) {
      size_t ecap = 3 * (size_t)r.log_cap + 40, emost = ((size_t)1 << 30) / (32 * B);
      if (emost < 80) emost = 80;
      if (ecap > emost) ecap = emost;
      if (ov.elog_cap) ecap = (size_t)*ov.elog_cap;
      r.elog_cap = (int)ecap;
    }
  }
  // A launch occupies the GPU in rounds of `resident` wavefronts, and a last round that is not full leaves CUs idle until
  // the launch ends (cfg2: 8 192 wavefronts over 3 072 resident = 2.67 rounds, 11 % of the machine-time lost).  When the
  // rounds do not come out even, the batch runs as two halves on two streams: the tail of one half's launch overlaps the
  // other half's next one.  (ORL_PERSIST_PARTS=1|2 forces either.)
  const int resident = ch.wgs_per_cu * n_cu;  // wavefronts the GPU holds at once (LDS window and register budget)
  const double rounds = (double)n_wg / (double)(resident > 0 ? resident : 1);
  // (a run of a single chunk has no next launch to overlap with: one part)
  r.parts = (n_steps > r.chunk && n_wg >= 2048 && rounds > 1.0) ? 2 : 1;
  if (ov.parts && (*ov.parts == 1 || n_wg >= 2)) r.parts = *ov.parts;
  r.half = r.parts == 2 ? (n_wg + 1) / 2 * 8 : P.B;
  return r;
}
