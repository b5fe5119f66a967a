// orl_view_plan.h — the host-side decisions of the per-step device views of the pending service: the shape of a view's rows
// (view_shape) and the geometry of its launch (view_plan).
//
// Like the form choice (orl_persist_form.h) and the run plan (orl_run_plan.h) both are pure functions of the batch's sizes, pinned
// without a device by tests/test_view_plan.py (orl_debug_view_plan).  No HIP call in here.  Included behind the views' headers
// (orl_mask.h, orl_rmcsa_mask.h, orl_assign.h, orl_route.h, orl_route_cores.h, orl_blocks.h, orl_horizon.h, orl_capacity.h, orl_link_obs.h, orl_qos_obs.h), which keep the LDS sizes of one env or wavefront
// next to the kernels that lay them out; orl_kernels.hip and orl_api.hip both see all of them, their kernels only where they are
// launched.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef ORL_PATH_OBS_STAGE
#define ORL_PATH_OBS_STAGE 1  // 0: the path features' direct form for every shape (A/B builds)
#endif

enum ViewKind {
  VIEW_ACTION_MASK = 0,    // k_action_mask (RMSA, DeepRMSA, RWA); arg: the layout
  VIEW_RMCSA_MASK,         // k_rmcsa_mask; arg: the layout
  VIEW_COMPLETE,           // k_rmcsa_complete
  VIEW_ASSIGN,             // k_assign_spectrum; arg: the rule
  VIEW_PATH_FEATURES,      // k_path_features; arg: j
  VIEW_LINK_FEATURES,      // k_link_features
  VIEW_MATRIX_PATHS_OBS,   // k_qos_matrix_obs
  VIEW_ROUTE,              // k_route_spectrum; arg: the rule
  VIEW_ROUTE_CORES,        // k_route_cores (RMCSA); arg: the rule
  VIEW_BLOCKS,             // k_block_table, k_select_blocks; arg: j
  VIEW_COUNT
};

// LDS of one workgroup: what a kernel gets without asking for more (every view but the last stays within it), and the most a
// workgroup can ask for
constexpr size_t kViewLdsDefault = 48 * 1024;
constexpr size_t kViewLdsMax = 64 * 1024;

// wavefronts per workgroup of a view whose wavefront keeps `bytes_per_wavefront` of LDS: the most of 4, 2, 1 that fit
// kViewLdsDefault; 0: not even one does
inline int view_waves(size_t bytes_per_wavefront) {
  for (int w = 4; w >= 1; w >>= 1)
    if (w * bytes_per_wavefront <= kViewLdsDefault) return w;
  return 0;
}

// A view's rows: per env `dim` elements of `elem_bytes` at a device pitch of `pitch` elements (rows are written as 16-byte
// stores); the feature rows are a header and `rows` blocks of `width` values.  dim == 0: this family has no such layout.
struct ViewShape { int64_t dim; int rows, width; int64_t pitch; int elem_bytes; };
// arg: the mask layout (ORL_MASK_*), the path features' j
inline ViewShape view_shape(const orl::DevParams& P, int view, int arg) {
  const bool rmcsa = P.env_type == orl::ENV_RMCSA;
  ViewShape s = {0, 0, 0, 0, 1};
  switch (view) {
    case VIEW_ACTION_MASK:
    case VIEW_RMCSA_MASK:  // (orl_mask.h, orl_rmcsa_mask.h: the family decides which layouts exist)
      if (rmcsa) s.dim = arg == ORL_MASK_PATH_MOD ? P.K * P.M + 1 : (arg == ORL_MASK_CORE_SLOT ? P.C * P.S + 1 : 0);
      else if (P.env_type != orl::ENV_RMSA && P.env_type != orl::ENV_DEEPRMSA && P.env_type != orl::ENV_RWA) s.dim = 0;
      else if (arg == ORL_MASK_JOINT) s.dim = P.K * (P.env_type == orl::ENV_DEEPRMSA ? P.J : P.S) + 1;
      else if (arg == ORL_MASK_PATH && P.env_type != orl::ENV_DEEPRMSA) s.dim = P.K + 1;
      break;
    case VIEW_COMPLETE:
    case VIEW_ASSIGN:  // the env's row of ORL_BUF_ACTIONS
      s.dim = 4; s.elem_bytes = 4;
      break;
    case VIEW_PATH_FEATURES:  // (orl_path_obs.h) the header, then a block of 2 j + 3 values per path (RMCSA: per path and core)
      s.rows = rmcsa ? P.K * P.C : P.K; s.width = 2 * arg + 3; s.elem_bytes = 4;
      s.dim = 1 + 2 * P.N + s.rows * s.width;
      break;
    case VIEW_LINK_FEATURES:  // (orl_link_obs.h) the header, then a block of 10 + k values per slot row
      s.rows = (rmcsa ? P.C : 1) * P.E; s.width = 10 + P.K; s.elem_bytes = 4;
      s.dim = 1 + 2 * P.N + s.rows * s.width;
      break;
    case VIEW_MATRIX_PATHS_OBS:  // (orl_qos_obs.h)
      s.dim = (int64_t)P.E * P.S * (P.K + 1) + 1;
      break;
    case VIEW_ROUTE:  // (orl_route.h) the per-path table: a row of (s*, c*, n, free) per path
      s.rows = P.K; s.width = 4; s.elem_bytes = 4;
      s.dim = 4 * P.K;
      break;
    case VIEW_ROUTE_CORES:  // (orl_route_cores.h) the (path, core) table: a row of (s*, c*, n, free) per pair, in the path features' row order
      if (rmcsa) { s.rows = P.K * P.C; s.width = 4; s.dim = 4 * s.rows; }
      s.elem_bytes = 4;
      break;
    case VIEW_BLOCKS:  // (orl_blocks.h) the block table: a row of (n, free, j (start, length) pairs) per row of the path features; its mask: view_blocks_mask
      s.rows = rmcsa ? P.K * P.C : P.K; s.width = 2 + 2 * arg; s.elem_bytes = 4;
      s.dim = (int64_t)s.rows * s.width;
      break;
  }
  const int64_t per16 = 16 / s.elem_bytes;
  s.pitch = (s.dim + per16 - 1) / per16 * per16;
  return s;
}

// the mask that goes with the block table of j blocks per row: one column per (row, block) and the reject column, bytes at a pitch of
// round_up(dim, 16)
inline ViewShape view_blocks_mask(const orl::DevParams& P, int j) {
  ViewShape s = {0, P.env_type == orl::ENV_RMCSA ? P.K * P.C : P.K, j, 0, 1};
  s.dim = (int64_t)s.rows * j + 1;
  s.pitch = (s.dim + 15) / 16 * 16;
  return s;
}

// A view's launch.  ok == 0: refused (the rows of the least workgroup the kernel runs in exceed the LDS limit, or a path's
// modulations its 32-bit word) — everything else is 0 then.  Every view but MatrixObservationWithPaths (one env per wavefront)
// puts 8 envs on a wavefront.
struct ViewPlan {
  bool ok;
  int waves, block;   // wavefronts and threads per workgroup
  unsigned grid;
  size_t lds_bytes;   // dynamic LDS of a workgroup
  bool staged;        // path features, block table: the wavefront's rows are assembled in LDS (else every lane stores its own blocks)
  int chunk;          // link features: slot rows per env and round through LDS (a multiple of 8); 0: the rows whole
  bool counted;       // spectrum assignment: the instantiation with the per-slot occupancy counts
};
// W: the batch's row width in 64-bit words; arg: the mask layout, the assignment rule (ORL_ASSIGN_*; VIEW_ROUTE too), the path features' j
inline ViewPlan view_plan(const orl::DevParams& P, int W, int view, int arg) {
  ViewPlan r = {};
  int per_wave = 8;  // envs of a wavefront
  size_t wave = 0;   // LDS bytes of a wavefront
  switch (view) {
    case VIEW_ACTION_MASK:  // 4 wavefronts per workgroup, or refused
      wave = (size_t)8 * mask_env_words(arg, P.env_type, W, P.K) * sizeof(uint32_t);
      r.waves = view_waves(wave) < 4 ? 0 : 4;
      break;
    case VIEW_RMCSA_MASK:
      wave = (size_t)8 * rmcsa_mask_env_words(arg, W, P.K, P.C) * sizeof(uint32_t);
      r.waves = P.M > 32 ? 0 : view_waves(wave);
      break;
    case VIEW_COMPLETE:
    case VIEW_ROUTE_CORES:  // (orl_route_cores.h: no LDS; ORL_ASSIGN_MIN_CUTS keeps its planes in registers)
      r.waves = 4;
      break;
    case VIEW_ASSIGN:  // (the counts of 4 wavefronts fit for every W: orl_assign.h)
    case VIEW_ROUTE:   // (orl_route.h: the same counts for the same rules; ORL_ASSIGN_MIN_CUTS keeps its planes in registers)
      r.counted = assign_rule_counted(arg);
      wave = r.counted ? (size_t)8 * assign_env_dwords(W) * sizeof(uint32_t) : 0;
      r.waves = r.counted ? view_waves(wave) : 4;
      break;
    case VIEW_PATH_FEATURES: {  // staged where a wavefront's 8 rows fit
      wave = (size_t)8 * view_shape(P, view, arg).pitch * sizeof(float);
      const int fit = ORL_PATH_OBS_STAGE ? view_waves(wave) : 0;
      r.staged = fit != 0;
      r.waves = fit ? fit : 4;
      if (!fit) wave = 0;
    } break;
    // (orl_blocks.h) as the path features, with the mask's bit rows beside the table rows in both forms; k_select_blocks takes the
    // same geometry and no LDS of its own (the launcher passes 0)
    case VIEW_BLOCKS: {
      const size_t bits = (size_t)8 * blocks_mask_env_words(view_shape(P, view, arg).rows) * sizeof(uint32_t);
      wave = bits + (size_t)8 * view_shape(P, view, arg).pitch * sizeof(int32_t);
      r.staged = view_waves(wave) != 0;
      if (!r.staged) wave = bits;
      r.waves = view_waves(wave);
    } break;
    // the rows whole where 8 of them fit beside the 8 envs' link sets; else in rounds of `chunk` slot rows per env, the most (a
    // multiple of 8) that 4, 2 or 1 wavefronts' staging fits
    case VIEW_LINK_FEATURES: {
      const ViewShape s = view_shape(P, view, 0);
      r.waves = view_waves(link_obs_wave_lds(P.K, (int)s.pitch));
      if (!r.waves) {
        r.waves = view_waves(link_obs_wave_lds(P.K, 8 * s.width));  // (k = 64: 8 blocks of 74 floats for 8 envs + their link sets = 27 kB, one wavefront)
        if (r.waves) r.chunk = (int)((kViewLdsDefault / r.waves - link_obs_wave_lds(P.K, 0)) / (8 * s.width * sizeof(float))) / 8 * 8;
      }
      wave = link_obs_wave_lds(P.K, r.chunk ? r.chunk * s.width : (int)s.pitch);
    } break;
    case VIEW_MATRIX_PATHS_OBS:
      per_wave = 1;
      wave = (size_t)qos_obs_wave_lds(P.E, P.K);
      r.waves = ORL_QOBS_WAVES * wave > kViewLdsMax ? 0 : ORL_QOBS_WAVES;
      break;
  }
  if (!r.waves) return ViewPlan{};
  r.ok = true;
  r.block = 64 * r.waves;
  r.grid = (unsigned)((P.B + per_wave * r.waves - 1) / (per_wave * r.waves));
  r.lds_bytes = r.waves * wave;
  return r;
}

// The release horizons (orl_horizon.h) are planned apart from view_plan: the view takes two arguments (layout, j), and one wavefront
// serves one env.  dim = rows x (S | 2 j) + 1 float32 (the last column: the pending service's holding time).  dim == 0: no such rows
// (QoSConstrainedRA; a layout or j out of range; ORL_HORIZON_SLOTS with j != 1).
inline ViewShape horizon_shape(const orl::DevParams& P, int layout, int j) {
  ViewShape s = {0, 0, 0, 0, 4};
  if (P.env_type == orl::ENV_QOS || j < 1 || j > 8 || (layout != ORL_HORIZON_SLOTS && layout != ORL_HORIZON_BLOCKS)) return s;
  if (layout == ORL_HORIZON_SLOTS && j != 1) return s;
  s.rows = P.env_type == orl::ENV_RMCSA ? P.K * P.C : P.K;
  s.width = layout == ORL_HORIZON_SLOTS ? P.S : 2 * j;
  s.dim = (int64_t)s.rows * s.width + 1;
  s.pitch = (s.dim + 3) / 4 * 4;
  return s;
}

// The launch of k_release_horizons: the most wavefronts per workgroup of 4, 2, 1 whose LDS shares hold all R rows of H beside the link
// table and (BLOCKS) the output row — one round; where not even one wavefront's 48 KiB do, one wavefront and rounds of the most rows
// that fit (every round re-reads the env's release table, so fewer rounds come before more wavefronts).  ok == 0: refused — no such
// rows, or not one row fits beside the rest.
struct HorizonPlan {
  bool ok;
  int waves, block;
  unsigned grid;
  size_t lds_bytes;  // dynamic LDS of a workgroup
  int rows;          // rows of H per round
  int wave_bytes;    // LDS of one wavefront
};
inline HorizonPlan horizon_plan(const orl::DevParams& P, int W, int layout, int j) {
  (void)W;  // (the kernel is compiled per row width for the block walk; its LDS does not depend on it)
  HorizonPlan r = {};
  const ViewShape sh = horizon_shape(P, layout, j);
  if (!sh.dim) return r;
  const int64_t stage = layout == ORL_HORIZON_BLOCKS ? sh.pitch : 0;
  if (stage > (int64_t)(kViewLdsDefault / sizeof(float))) return r;
  r.waves = view_waves(horizon_wave_lds(P.E, P.S, sh.rows, (int)stage));
  r.rows = sh.rows;
  if (!r.waves) {
    const int64_t left = (int64_t)kViewLdsDefault - (int64_t)horizon_wave_lds(P.E, P.S, 0, (int)stage);
    r.rows = left < 0 ? 0 : (int)(left / ((int64_t)sizeof(float) * P.S));
    while (r.rows > 0 && horizon_wave_lds(P.E, P.S, r.rows, (int)stage) > kViewLdsDefault) r.rows--;
    if (r.rows < 1) return HorizonPlan{};
    r.waves = 1;
  }
  r.ok = true;
  r.block = 64 * r.waves;
  r.grid = (unsigned)((P.B + r.waves - 1) / r.waves);
  r.wave_bytes = (int)horizon_wave_lds(P.E, P.S, r.rows, (int)stage);
  r.lds_bytes = (size_t)r.waves * r.wave_bytes;
  return r;
}

// The network capacity view (orl_capacity.h) is planned apart as well: one wavefront serves one env and walks the path tables of
// every pair.  n_cls: the classes of the family (RWA: one; else the rows of the bit-rate table).  dim == 0: no such rows
// (QoSConstrainedRA, which has no slot maps; an unknown layout).
inline int capacity_classes(const orl::DevParams& P) { return P.env_type == orl::ENV_RWA ? 1 : P.n_br; }
inline ViewShape capacity_shape(const orl::DevParams& P, int layout) {
  ViewShape s = {0, 0, 0, 0, 4};
  if (P.env_type == orl::ENV_QOS) return s;
  const int64_t NN = (int64_t)P.N * P.N, cores = P.env_type == orl::ENV_RMCSA ? P.C : 1, n_cls = capacity_classes(P);
  switch (layout) {
    case ORL_CAPACITY_PATHS: s.rows = (int)(NN * P.K * cores); s.width = 2; s.dim = 2 * NN * P.K * cores; break;
    case ORL_CAPACITY_SERVICEABLE: s.rows = (int)NN; s.width = (int)n_cls; s.dim = NN * n_cls; s.elem_bytes = 1; break;
    case ORL_CAPACITY_COUNTS: s.rows = 1; s.width = (int)(n_cls + NN); s.dim = n_cls + NN; break;
    default: return s;
  }
  const int64_t per16 = 16 / s.elem_bytes;
  s.pitch = (s.dim + per16 - 1) / per16 * per16;
  return s;
}

// The launch of k_network_capacity.  A wavefront keeps in LDS the per-path longest runs (SERVICEABLE, COUNTS), its output row (COUNTS) and,
// where they fit beside them, the env's slot maps (staged): the most wavefronts per workgroup of 4, 2, 1 whose shares hold all of it
// within kViewLdsDefault; else one wavefront with all of it within kViewLdsMax; else the maps stay in global memory and the same two
// rules go for the rest.  ok == 0: refused — no such rows, or one env's per-path array and bit matrix exceed kViewLdsMax.
struct CapacityPlan {
  bool ok;
  int waves, block;
  unsigned grid;
  size_t lds_bytes;  // dynamic LDS of a workgroup
  bool staged;       // the env's slot maps are copied into LDS
  int wave_bytes;    // LDS of one wavefront
};
inline CapacityPlan capacity_plan(const orl::DevParams& P, int W, int layout) {
  CapacityPlan r = {};
  const ViewShape sh = capacity_shape(P, layout);
  if (!sh.dim) return r;
  const size_t fixed = layout == ORL_CAPACITY_PATHS ? 0 : capacity_path_bytes(P.N, P.K) + (layout == ORL_CAPACITY_COUNTS ? (size_t)sh.pitch * 4 : 0);
  if (fixed > kViewLdsMax) return r;
  const size_t maps = capacity_map_bytes(W, P.env_type == orl::ENV_RMCSA ? P.C : 1, P.E);
  r.waves = view_waves(fixed + maps);
  r.staged = r.waves != 0;
  if (!r.waves && fixed + maps <= kViewLdsMax) { r.waves = 1; r.staged = true; }
  if (!r.waves) r.waves = view_waves(fixed);
  if (!r.waves) r.waves = 1;
  r.ok = true;
  r.block = 64 * r.waves;
  r.grid = (unsigned)((P.B + r.waves - 1) / r.waves);
  r.wave_bytes = (int)(fixed + (r.staged ? maps : 0));
  r.lds_bytes = (size_t)r.waves * r.wave_bytes;
  return r;
}

// capacity_after (orl_capacity_after.h): what each of Q candidate placements of the pending service leaves of the COUNTS class row.
// Q: the candidates of the call — the rows of the route / core table, the rows of the block table times j, or the given count —
// 1 .. ORL_AFTER_MAX_Q; the rows are Q + 1, the last one the baseline.  dim == 0: no such rows (QoSConstrainedRA, an unknown layout,
// Q out of range).
inline ViewShape capacity_after_shape(const orl::DevParams& P, int layout, int Q) {
  ViewShape s = {0, 0, 0, 0, 4};
  if (P.env_type == orl::ENV_QOS || Q < 1 || Q > ORL_AFTER_MAX_Q) return s;
  const int64_t n_cls = capacity_classes(P);
  switch (layout) {
    case ORL_AFTER_CLASSES: s.rows = Q + 1; s.width = (int)n_cls; break;
    case ORL_AFTER_TOTAL: s.rows = Q + 1; s.width = 1; break;
    default: return s;
  }
  s.dim = (int64_t)s.rows * s.width;
  s.pitch = (s.dim + 3) / 4 * 4;
  return s;
}
// The launch of k_capacity_after: capacity_plan's rules — the most wavefronts per workgroup of 4, 2, 1 whose shares hold the fixed
// terms and the maps within kViewLdsDefault; else one wavefront with all of it within kViewLdsMax; else the maps stay in global
// memory and the same two rules go for the rest — with this kernel's fixed terms: the longest runs, 64 lanes' scratch of k8 bytes, the
// class row twice, and for TOTAL the Q + 1 sums (capacity_after_fixed_bytes).  ok == 0: refused.
inline CapacityPlan capacity_after_plan(const orl::DevParams& P, int W, int layout, int Q) {
  CapacityPlan r = {};
  const ViewShape sh = capacity_after_shape(P, layout, Q);
  if (!sh.dim) return r;
  const size_t fixed = capacity_after_fixed_bytes(P.N, P.K, capacity_classes(P), Q, layout == ORL_AFTER_TOTAL);
  if (fixed > kViewLdsMax) return r;
  const size_t maps = capacity_map_bytes(W, P.env_type == orl::ENV_RMCSA ? P.C : 1, P.E);
  r.waves = view_waves(fixed + maps);
  r.staged = r.waves != 0;
  if (!r.waves && fixed + maps <= kViewLdsMax) { r.waves = 1; r.staged = true; }
  if (!r.waves) r.waves = view_waves(fixed);
  if (!r.waves) r.waves = 1;
  r.ok = true;
  r.block = 64 * r.waves;
  r.grid = (unsigned)((P.B + r.waves - 1) / r.waves);
  r.wave_bytes = (int)(fixed + (r.staged ? maps : 0));
  r.lds_bytes = (size_t)r.waves * r.wave_bytes;
  return r;
}
