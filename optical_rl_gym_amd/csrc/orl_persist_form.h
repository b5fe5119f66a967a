// orl_persist_form.h — the forms of the persistent kernel (k_persist, orl_kernels.hip) and the choice among them.
//
// One table describes every form; the kernel (the decode of its LDS template argument), the launcher (orl_launch::persist),
// the specialisation flags and the debug queries (orl_api.hip) all read it.  The choice is a pure function of the batch's
// sizes, of whether a specialisation library runs, and of the ORL_PERSIST_* overrides, which ONE function reads from the
// environment (persist_overrides_from_env): tests/test_persist_choice.py pins it case by case without a device.
#pragma once
#include <assert.h>
#include <stdlib.h>
#include <optional>

#include "orl_host.h"

// ---- the LDS window ----------------------------------------------------------------------------------------------------
struct PersistLds {  // byte offsets into the workgroup's dynamic LDS window (all multiples of 16)
  int tab, mtab, tally, tw, list, clk, misc, bm, ls, cs, csw, sc, ic, mini, total;  // (ic: inner-run cache, then the occ / fb cache)
};
// state: 0 = only the per-step tables, 1 = + slot maps, per-core sums and env records, 2 = + link statistics, 3 = slot maps and
// per-core sums but the env records stay in global memory (the window of the 4-wave forms: cfg2 8 832 B, 16 per CU);
// compact: the bit-word sink of the single-core families (4 bytes per link and env + a mask table per env);
// inner: 0 = no row caches, 1 = the per-word longest-run cache of every row, 2 = + every row's contribution to the compactness
// sums, (occ << 16) | free blocks (4 bytes per row each)
// mini: the eight record words the deferred-statistics control phase works on, for the forms whose records stay in global memory
// rd: the rows-deferred form (round 6) — no row phase in the loop, hence no sink table, mask table, item list, clock pairs, row
// caches or per-core sums: the window is the slot maps, the record words the control phase works on, and 16 bytes
__host__ __device__ inline PersistLds persist_lds_layout(int E, int H, int bm_words, int C, int state, bool compact, int inner, bool mini = false,
                                                         bool rd = false) {
  PersistLds L;
  int o = 0;
  L.tab = o; if (!rd) o += (8 * E * (int)(compact ? sizeof(orl::sp::SinkEntryC) : sizeof(orl::sp::SinkEntry)) + 15) & ~15;
  L.mtab = o; if (compact && !rd) o += 8 * ORL_MTAB * 2;
  L.tw = compact ? 0 : (E + 3) >> 2;
  L.tally = o; o += 8 * L.tw * 4;
  // one entry per touched link and env, a second one where the step's provision meets a release (at most its hops)
  L.list = o; if (!rd) o += ((8 * (E + (H < E ? H : E)) * 2) + 15) & ~15;
  // {provision clock, step clock} of the 8 envs for the row phase (the deferred-statistics control phase never writes SC_NOWA,
  // which the replay owns, so the forms with the records in LDS have the pair too; the full-LDS test form reads the records)
  L.clk = o; if (state != 2 && !rd) o += 8 * 2 * 8;
  L.misc = o; o += 16;
  L.bm = o; if (state >= 1) o += 8 * bm_words * 8;
  L.csw = (4 * C + 3) & ~3;  // sums + their release part, ints per env
  L.cs = o; if ((state >= 1 || mini) && !rd) o += 8 * L.csw * 4;  // (the global-state form of the deferred-statistics kernel keeps them in LDS too)
  L.sc = o; if (state == 1 || state == 2) o += 8 * ORL_SCAL_LDS_WORDS * 8;
  L.ic = o; if (state >= 1 && inner && !rd) o += inner * ((8 * E * 4 + 15) & ~15);
  L.ls = o; if (state == 2) o += 8 * E * 32;
  L.mini = o; if (mini && (state == 0 || state == 3)) o += (8 * ORL_MINI_STRIDE * 8 + 15) & ~15;
  L.total = o;
  return L;
}
template <int ENV> struct PersistCompact { static constexpr bool value = ENV != orl::ENV_RMCSA; };
static inline bool persist_compact(int env_type) { return env_type != orl::ENV_RMCSA; }
// (rows of one or two words: searching both costs less than the bookkeeping — cfg3 measured 1.20e9 without, 1.01e9 with)
template <int ENV, int W, int LDS> struct PersistInner { static constexpr bool value = LDS >= 1 && W >= 3 && W <= 5 && (ENV == orl::ENV_RMSA || ENV == orl::ENV_DEEPRMSA); };
static inline bool persist_inner(int env_type, int W, int state) { return state >= 1 && W >= 3 && W <= 5 && (env_type == orl::ENV_RMSA || env_type == orl::ENV_DEEPRMSA); }
// the two-wavefront form (k_persist<..., RW>): the pair's counters and channels, then the two staging areas, behind the window
// (orl_kernels.hip, persist_row_wave)
#define ORL_RW_SYNC_WORDS 12
#define ORL_RW_STAGE_BYTES (2 * 64 * 24)  // two batches: the one asked for a step ahead, and one asked for on the spot
#define ORL_RW_EXTRA_BYTES (ORL_RW_SYNC_WORDS * 4 + ORL_RW_STAGE_BYTES)

// ---- the forms ---------------------------------------------------------------------------------------------------------
// A form is what lives in the LDS window and how many waves per SIMD the registers are budgeted for.  The LDS window decides
// how many wavefronts a CU holds.  The hardware allocates LDS in pieces of 1 280 bytes (tools/probe/lds_resident.hip,
// measured on MI355X: 12 workgroups share a CU's 160 KiB up to 12 800 B each, 11 up to 14 080, 16 up to 10 240 —
// hipOccupancyMaxActiveBlocksPerMultiprocessor says 12 up to 13 648).
// k_persist's LDS template argument: 0-3 the state in the window (persist_lds_layout); 4 / 5 = state 3 / 1 with the rows deferred
// (round 6: the window without the row phase's tables)
constexpr int persist_state_of(int lds_arg) { return lds_arg == 4 ? 3 : (lds_arg == 5 ? 1 : lds_arg); }
constexpr bool persist_rd_of(int lds_arg) { return lds_arg == 4 || lds_arg == 5; }
struct PersistForm {
  int lds_arg;    // k_persist's LDS template argument
  int state;      // what is in the window (persist_lds_layout)
  bool rd;        // rows deferred: the loop logs events, k_rowstats replays the link statistics after the launch
  int waves;      // waves per SIMD the registers are budgeted for
  bool alt_only;  // built into the -DORL_ALT_IMPLS library only
};
constexpr PersistForm persist_form_entry(int lds_arg, int waves, bool alt_only = false) {
  return {lds_arg, persist_state_of(lds_arg), persist_rd_of(lds_arg), waves, alt_only};
}
// indexed by the form number (ORL_PERSIST_VARIANT, orl_batch_debug_persist_form).  Forms 2 and 3 (link statistics and sums in LDS
// too) measured slower everywhere: one more independent form for the cross-implementation tests
constexpr PersistForm kPersistForms[] = {persist_form_entry(0, 4), persist_form_entry(0, 3), persist_form_entry(2, 2, true),
                                         persist_form_entry(2, 3, true), persist_form_entry(1, 3), persist_form_entry(1, 4),
                                         persist_form_entry(3, 4), persist_form_entry(4, 4), persist_form_entry(5, 4)};
constexpr int kPersistFormCount = (int)(sizeof(kPersistForms) / sizeof(kPersistForms[0]));
#ifdef ORL_ALT_IMPLS
constexpr bool kPersistAltBuild = true;
#else
constexpr bool kPersistAltBuild = false;
#endif
// a form number of the table that this library carries for some family ...
constexpr bool persist_form_in_build(int form) {
  return form >= 0 && form < kPersistFormCount && (kPersistAltBuild || !kPersistForms[form].alt_only);
}
// ... and for this one.  RMCSA (24-byte sink entries, a core per mask, the general row loop) does not fit the 128-VGPR budget of the
// 4-wave forms — 25-32 spilled VGPRs, measured slower than its 3-wave forms wherever both fit — and is not built in them.
constexpr bool persist_form_built(int env_type, int form) {
  return persist_form_in_build(form) && !(env_type == orl::ENV_RMCSA && kPersistForms[form].waves == 4);
}
// forms of at most this many waves per SIMD keep the soon list in registers and request early
#ifndef ORL_PF_WAVES
#define ORL_PF_WAVES 3
#endif
constexpr bool persist_soon_in_registers(int waves) { return waves <= ORL_PF_WAVES; }

// ---- the overrides -----------------------------------------------------------------------------------------------------
// A/B measurements and cross-checks: one field per environment variable, empty where it is not set.
struct PersistOverrides {
  std::optional<int> variant;         // ORL_PERSIST_VARIANT: the form number
  std::optional<int> inner;           // ORL_PERSIST_INNER: 0 = no row caches, 1 = inner runs, 2 = + occ / free blocks
  std::optional<int> rw;              // ORL_PERSIST_RW: the two-wavefront form at any batch size (0 / 1)
  std::optional<int> evl;             // ORL_PERSIST_EVL: the pair's pending release times in LDS (0 / 1)
  std::optional<int> spec;            // ORL_PERSIST_SPEC: 0 = the generic kernels although a specialisation library is attached
  std::optional<int> fair;            // ORL_PERSIST_FAIR: DevParams::persist_fair, 0-30 (0 = the arbiter's oldest-first)
  std::optional<int> wgs_per_cu;      // ORL_PERSIST_WGS_PER_CU: lowers the residency by padding the LDS request (experiments)
  std::optional<int> row_cache_keep;  // ORL_ROW_CACHE_KEEP: 0 = rebuild the row caches at every launch
};
// Read where a choice is made — once per device-resident run, and at every flags query — so that a script may change a variable
// between two runs of one batch (not between two launches of one run: every launch of a run gets the run's one choice).
static inline PersistOverrides persist_overrides_from_env() {
  PersistOverrides o;
  if (const char* e = getenv("ORL_PERSIST_VARIANT")) o.variant = atoi(e);
  if (const char* e = getenv("ORL_PERSIST_INNER")) o.inner = atoi(e);
  if (const char* e = getenv("ORL_PERSIST_RW")) o.rw = atoi(e);
  if (const char* e = getenv("ORL_PERSIST_EVL")) o.evl = atoi(e);
  if (const char* e = getenv("ORL_PERSIST_SPEC")) o.spec = atoi(e);
  if (const char* e = getenv("ORL_PERSIST_FAIR")) { const int f = atoi(e); if (f >= 0 && f <= 30) o.fair = f; }
  if (const char* e = getenv("ORL_PERSIST_WGS_PER_CU")) o.wgs_per_cu = atoi(e);
  if (const char* e = getenv("ORL_ROW_CACHE_KEEP")) o.row_cache_keep = atoi(e);
  return o;
}
// whether the launchers take the kernels of the attached specialisation library
static inline bool persist_use_spec(bool attached, const PersistOverrides& ov) { return attached && ov.spec.value_or(1) != 0; }

// ---- the choice --------------------------------------------------------------------------------------------------------
static inline int lds_wgs_per_cu(size_t lds) {
  if (lds == 0) return 1 << 20;
  const size_t alloc = (lds + 1279) / 1280 * 1280;
  return (int)((size_t)(160 * 1024) / alloc);
}
static inline size_t persist_window(const orl::DevParams& VP, int lds_arg, int inner) {
  const bool rd = persist_rd_of(lds_arg);
  return (size_t)persist_lds_layout(VP.E, VP.H, VP.bm_words, VP.C, persist_state_of(lds_arg), persist_compact(VP.env_type), rd ? 0 : inner,
                                    orl_persist_deferred(VP.env_type), rd).total;
}
// the rows-deferred forms: single-core families with the statistics deferred, a bit per link in a 64-bit event word, services of
// at most 63 slots in a 9-bit first slot (the compact sink's own limits).  (The event log they write to: the plan of a run asks for
// one whenever the chosen form is one of them, run_plan / ensure_logs.)
static inline bool persist_rd_possible(const orl::DevParams& VP) {
  return orl_persist_deferred(VP.env_type) && VP.env_type != orl::ENV_RMCSA && VP.E <= 64 && VP.S <= 512;
}
struct PersistChoice {
  int form;             // index into kPersistForms; persist_form_built() for the batch's family
  size_t lds;           // bytes of the LDS window (with the pair's areas and release times, where taken)
  int inner;            // row-cache level (DevParams::persist_ic)
  int rw;               // 1: the two-wavefront form (specialisation libraries only)
  int evl;              // 1: the pair's pending release times in LDS (DevParams::persist_evl)
  size_t launch_lds;    // bytes of LDS the launch asks for: `lds`, padded where ORL_PERSIST_WGS_PER_CU lowers the residency
  int wgs_per_cu;       // workgroups per CU the form allows (window `lds`, register budget): what decides one stream or two
  int fair;             // DevParams::persist_fair
  bool row_cache_keep;  // the row caches of the last launch may be taken over (DevParams::row_cache_key != 0)
};
// `tuned`: the choice for a specialisation library (built without machine-level LICM and with the soon list in registers in the
// 4-wave forms, _build.py SPEC_TUNING) — for the flags such a library is built with, and at launch when one is attached.
// VP.B is the WHOLE batch (its wavefront count decides between the 3- and the 4-wave form, and a specialisation library is built
// for that choice).
static inline PersistChoice persist_choose(const orl::DevParams& VP, bool tuned, const PersistOverrides& ov) {
  using orl::ENV_RMCSA;
  using orl::i64;
  // Measured on MI355X, env-steps/s: cfg2 65 536 envs: form 0 (global state, 4 waves) 8.3e8, form 4 (LDS
  // state, 3 waves) 1.02e9 at 11 wavefronts per CU with the inner-run cache, 1.05e9 at 12 without it — 69 MB of HBM traffic
  // and 0.85 M L2<->fabric requests per batched step against 206 MB / 2.63 M; cfg1 65 536: form 4 1.13e9, form 5 (LDS state,
  // 4 waves) 1.18e9; cfg3: 1.25e9 / 1.27e9.  A wavefront more per CU is worth 3-5 %: the 4-wave form is taken if its
  // window keeps 16 on a CU, the 3-wave form down to 10, and the inner-run cache (+2.5 %) only where it costs no wavefront.
  const bool can_inner = persist_inner(VP.env_type, VP.W, 1);
  // the row caches (level 1: inner free runs, +2.5 %; level 2: + each row's occ / free-block contribution, +2 %) are taken at the
  // highest level that costs no wavefront per CU
  auto level = [&](int lds_arg, int cap) {
    if (!can_inner) return 0;
    const int r_none = lds_wgs_per_cu(persist_window(VP, lds_arg, 0));
    for (int lv = 2; lv >= 1; lv--) {
      const int r = lds_wgs_per_cu(persist_window(VP, lds_arg, lv));
      if ((r < cap ? r : cap) == (r_none < cap ? r_none : cap)) return lv;
    }
    return 0;
  };
  const size_t l0 = persist_window(VP, 1, 0), g0 = persist_window(VP, 3, 0);  // (g: records in global memory)
  const int r0 = lds_wgs_per_cu(l0);
  PersistChoice c;
  // (round 3, cfg2 with the 4-byte sink entries: form 4 with the cache 1.23e9; form 6 — 4 waves per SIMD, 16 per CU, but the
  // records in global memory, the soon list in memory and 9 spilled VGPRs — 1.14e9: what a wavefront keeps next to itself is
  // worth more than a fourth wavefront per SIMD.  Form 6 is taken only where the 3-wave window does not fit at all.)
  if (r0 >= 16) { c.form = 5; c.inner = level(1, 16); }
  // (round 4: a tuned instantiation of form 6 needs 128 VGPRs with the soon list in registers and no spills, and 16 wavefronts
  // per CU are 4 096 resident = exactly two generations of a 65 536-env batch: cfg2 20-step launches 1.135e9 -> 1.190e9, 300-step
  // runs 1.467e9 -> 1.474e9 against form 4)
  // ... for batches of more wavefronts than form 4 keeps resident (12 per CU x 256 CUs); below that no generation is cut short, and
  // the records in LDS are a dependent round trip per step less: 4 096 envs +1.7 %, 8 192 +2.1 %, 16 384 +4.1 % for form 4
  else if (tuned && VP.env_type != ENV_RMCSA && r0 >= 10 && lds_wgs_per_cu(g0) >= 16 && (VP.B + 7) / 8 > 12 * 256) { c.form = 6; c.inner = level(3, 16); }
  else if (r0 >= 10) { c.form = 4; c.inner = level(1, 12); }
  else if (lds_wgs_per_cu(g0) >= 16) { c.form = 6; c.inner = level(3, 16); }
  // (global state: the 4-wave form except for RMCSA — round 3, with the 4-byte sink entries: cfg5 Germany50 32 768 envs 5.6e8 at 4
  // waves per SIMD, 5.2e8 at 3; cfg4 RMCSA 5.0e8 / 5.3e8)
  else { c.form = (VP.env_type == ENV_RMCSA) ? 1 : 0; c.inner = 0; }
  // Small batches (round 5): at most 1 536 workgroups — 6 pairs per CU, all resident at 3 waves per SIMD — need the window to fit
  // at most six times — form 4
  // (everything in LDS, 3 waves per SIMD: soon list in registers) for every single-core configuration whose window fits a
  // workgroup's 64 KiB, in its two-wavefront form (below).  4 096 envs, form 4 as a pair against the form chosen above alone:
  // cfg2 +16 %, cfg3 +7 %, cfg1 +2 %, cfg5 (Germany50, global state above) +19 %.
  const i64 n_wg = (VP.B + 7) / 8;
  bool small_pair = false;
  if (tuned && VP.env_type != ENV_RMCSA && n_wg <= 1536) {
    const size_t w = persist_window(VP, 1, can_inner ? 2 : 0) + ORL_RW_EXTRA_BYTES;
    if (w <= 64 * 1024 && lds_wgs_per_cu(w) >= (int)((n_wg + 255) / 256)) { c.form = 4; small_pair = true; }
  }
  if (ov.variant) {  // A/B measurements and cross-checks
    const int f = *ov.variant;
    bool built = persist_form_in_build(f);
    if (built && kPersistForms[f].rd) built = persist_rd_possible(VP);
    if (built && persist_window(VP, kPersistForms[f].lds_arg, 0) <= 64 * 1024 && f != c.form) {
      c.form = f;
      const PersistForm& F = kPersistForms[f];
      c.inner = (!F.rd && persist_inner(VP.env_type, VP.W, F.state)) ? level(F.lds_arg, 4 * F.waves) : 0;
    }
  }
  // RMCSA is not built in the 4-wave forms (persist_form_built): routed to the 3-wave form with the same state (global: 1; maps +
  // records in LDS: 4, where that window fits a workgroup; else global)
  if (!persist_form_built(VP.env_type, c.form)) {
    const bool lds_ok = kPersistForms[c.form].lds_arg != 0 && persist_window(VP, 1, 0) <= 64 * 1024 && lds_wgs_per_cu(persist_window(VP, 1, 0)) >= 4;
    c.form = lds_ok ? 4 : 1;
    c.inner = 0;
  }
  if (ov.inner) {  // A/B and cross-checks
    const int v = *ov.inner;
    c.inner = (v >= 0 && v <= 2 && !kPersistForms[c.form].rd && persist_inner(VP.env_type, VP.W, kPersistForms[c.form].state)) ? v : 0;
  }
  // The two-wavefront form (k_persist<..., RW>, specialisation libraries only): batches whose pairs are all resident at once
  // (measured: +20 % at 10 240 and 12 288 envs of cfg2, -20 % at 14 336, where a second generation starts).  LDS is no constraint
  // there: both row caches, and ORL_RW_EXTRA_BYTES for the pair's counters and the staged batch of services.  ORL_PERSIST_RW=0/1: A/B measurements and cross-checks at
  // any batch size.
  c.rw = 0;
  if (tuned && VP.env_type != ENV_RMCSA && kPersistForms[c.form].lds_arg == 1) {
    c.rw = small_pair ? 1 : 0;
    if (ov.rw) c.rw = *ov.rw != 0 ? 1 : 0;
  }
  if (c.rw && !ov.inner) c.inner = can_inner ? 2 : 0;
  c.lds = persist_window(VP, kPersistForms[c.form].lds_arg, c.inner) + (c.rw ? ORL_RW_EXTRA_BYTES : 0);
  // ... and, where it still fits a workgroup's 64 KiB and the batch's workgroups a CU, the 8 envs' pending release times (cfg2:
  // 36 KiB: two workgroups per CU, batches of at most 4 096 envs)
  c.evl = 0;
  if (c.rw) {
    const size_t w = c.lds + (size_t)8 * VP.ev_cap * 8;
    if (w <= 64 * 1024 && lds_wgs_per_cu(w) >= (int)(((VP.B + 7) / 8 + 255) / 256)) c.evl = 1;
    if (ov.evl) c.evl = (*ov.evl != 0 && w <= 64 * 1024) ? 1 : 0;
    if (c.evl) c.lds = w;
  }
  // Workgroups per CU the form allows (LDS window, register budget).  ORL_PERSIST_WGS_PER_CU=r lowers the residency of the launch
  // by padding the LDS request to the largest window that still fits r times (experiments).
  c.wgs_per_cu = 4 * kPersistForms[c.form].waves;
  if (lds_wgs_per_cu(c.lds) < c.wgs_per_cu) c.wgs_per_cu = lds_wgs_per_cu(c.lds);
  if (c.wgs_per_cu < 1) c.wgs_per_cu = 1;
  c.launch_lds = c.lds;
  if (ov.wgs_per_cu && *ov.wgs_per_cu >= 1 && *ov.wgs_per_cu < c.wgs_per_cu) {
    const size_t want = ((size_t)(160 * 1024) / (size_t)*ov.wgs_per_cu) / 1280 * 1280;
    if (want > c.lds) c.launch_lds = want;
  }
  c.fair = ov.fair.value_or(11);  // (20 us per priority level: about one step)
  c.row_cache_keep = ov.row_cache_keep.value_or(1) != 0;
  assert(persist_form_built(VP.env_type, c.form));
  return c;
}
