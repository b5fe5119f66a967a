// orl_route_cores.h — core and spectrum rules with a (path, core) table for RMCSA actions (include/orl.h, orl_batch_route_cores);
// included by orl_kernels.hip behind orl_route.h (the rules' winners and costs: route_plain_winner, route_cuts_winner,
// route_and_cuts, and through it orl_assign.h's keys) and orl_rmcsa_complete.h (m*(p): rmcsa_best_in_reach; rmcsa_reach of
// orl_rmcsa_mask.h).
//
// For EVERY pair (p, c) of a candidate path and a core of the env's pending service the kernel computes the winner (s*, c*) of the
// launch's rule on the path's AND-row in that core, for the n(p) of the path's modulation m(p) — m*(p) of orl_rmcsa_complete.h, or
// the launch's fixed modulation where it is within reach on p — and writes row p C + c of the env's table as one 16-byte store
// (s*, c*, n(p), free(p, c)); (S, ORL_ROUTE_NO_FIT, n(p), free(p, c)) where nothing fits, (S, ORL_ROUTE_NO_FIT, 0, 0) for a path
// the service cannot use (p >= n_paths, no modulation within reach), which loads no link row.  The pairs the prefix admits —
// all, those of the given path, the given pair — and that fit are reduced to one action (p, m(p), c, s*) in ORL_BUF_ACTIONS under
// the launch's route; none: the reject action (K, M, C, S).  A given column out of range matches no pair.
//
// Layout of the work: as k_rmcsa_complete — 8 lanes per env, one (path, core) pair per lane, path-major chunks of 8 — but with no
// early exit: the table needs every pair.  The route's running best stays in a register across the chunks as ONE packed key
// reduced with g8_min (key_cores).  Two instantiations, chosen by the launcher from the rule (route_mode_of): ROUTE_PLAIN for rules
// 0 - 3, ROUTE_CUTS for ORL_ASSIGN_MIN_CUTS with the 5 W plane words of route_and_cuts.  No LDS, no atomics, no host
// synchronisation: graph-capturable.  Env state and flags are only read.
// `given`: the path of env e at given[e * gstride] and its core at given[e * gstride + gcore] — the actions buffer itself with
// gstride 4 and gcore 2 (every lane of the group has both in registers before lane 0 stores the row: the store's value depends on
// those loads), or the batch's upload buffer (gstride n_given, gcore 1).
#pragma once

// the two routes that settle on the first path with a fit before they look at the cores
__host__ __device__ inline bool route_cores_path_first(int route) { return route == ORL_ROUTE_KSP_BEST_CORE || route == ORL_ROUTE_KSP_LEAST_LOADED_CORE; }

#ifdef ORL_W  // (the kernel: the per-W units, orl_kernels.hip)
// (primary, p, c, s*) of a pair that fits: the smallest key = the route's choice.  primary = 0 (KSP), c* (BEST, KSP_BEST_CORE) or
// S - free(p, c) (LEAST_LOADED, KSP_LEAST_LOADED_CORE), at most S under rules 0 - 3 and MIN_CUTS; the two KSP_*_CORE routes put the
// path above it.  Every key lies below ORL_ROUTE_NO_FIT, the key of "no fit"
enum { KEY_CORE_BITS = 5, KEY_CORE_MAX = (1 << KEY_CORE_BITS) - 1, KEY_PRIMARY_BITS = 10 };
static_assert(ORL_MAX_CORES <= KEY_CORE_MAX + 1, "a core does not fit the key's core field");
static_assert(ORL_MAX_SLOTS < (1 << KEY_PRIMARY_BITS) && ORL_MAX_HOPS <= ORL_MAX_SLOTS, "a cost or S - free(p, c) <= S does not fit the key's primary field");
static_assert(((((long long)ORL_MAX_SLOTS << KEY_PATH_BITS | KEY_PATH_MAX) << KEY_CORE_BITS | KEY_CORE_MAX) << KEY_SLOT_BITS | KEY_SLOT_MAX) < ORL_ROUTE_NO_FIT,
              "a (primary, path, core, slot) key reaches ORL_ROUTE_NO_FIT");
static_assert(((((long long)(ORL_MAX_PATHS - 1) << KEY_PRIMARY_BITS | ORL_MAX_SLOTS) << KEY_CORE_BITS | KEY_CORE_MAX) << KEY_SLOT_BITS | KEY_SLOT_MAX) < ORL_ROUTE_NO_FIT,
              "a (path, primary, core, slot) key reaches ORL_ROUTE_NO_FIT");
__device__ __forceinline__ int key_cores(bool path_first, int primary, int p, int c, int s) {
  const int hi = path_first ? ((p << KEY_PRIMARY_BITS) | primary) : ((primary << KEY_PATH_BITS) | p);
  return (((hi << KEY_CORE_BITS) | c) << KEY_SLOT_BITS) | s;
}
__device__ __forceinline__ int key_cores_path(bool path_first, int key) {
  const int hi = key >> (KEY_CORE_BITS + KEY_SLOT_BITS);
  return path_first ? (hi >> KEY_PRIMARY_BITS) : (hi & KEY_PATH_MAX);
}
__device__ __forceinline__ int key_cores_core(int key) { return (key >> KEY_SLOT_BITS) & KEY_CORE_MAX; }

template <int W, int MODE>
__global__ void __launch_bounds__(256) k_route_cores(DevParams P, int rule, int route, int modulation, int n_given, const int* given, int gstride, int gcore,
                                                     int4* table) {
  static_assert(MODE == ROUTE_PLAIN || MODE == ROUTE_CUTS, "the counted rules have no (path, core) form");
  const ViewLanes v = view_lanes();
  if (v.env >= P.B) return;  // (whole groups: the exchanges below stay within a group)
  const int gl = v.gl;
  const int K = P.K, S = P.S, E = P.E, M = P.M, C = P.C;
  const PendingSvc sv = view_pending(P, v.env);
  const int br_idx = sv.br_idx, pb = sv.pb;
  const int np = sv.np < K ? sv.np : K;
  const unsigned char* nsl = P.nslots + br_idx * M;
  const int* gv = given + v.env * gstride;
  const int gp = n_given >= 1 ? gv[0] : 0, gc = n_given >= 2 ? gv[gcore] : 0;
  const bool path_first = route_cores_path_first(route);
  const bool by_cost = route == ORL_ROUTE_BEST || route == ORL_ROUTE_KSP_BEST_CORE;
  const int total = K * C;
  int best = ORL_ROUTE_NO_FIT;
  for (int base = 0; base < total; base += 8) {
    const int q = base + gl;
    const int pth = q / C, core = q - pth * C;
    int n = 0, nfree = 0, slot = S, cost = ORL_ROUTE_NO_FIT;
    if (pth < np) {
      const double len = P.path_length[pb + pth];
      int mod;
      if (modulation >= 0) mod = rmcsa_reach(P, len, modulation, br_idx) ? modulation : -1;
      else mod = rmcsa_best_in_reach(P, nsl, len, br_idx);
      if (mod >= 0) {
        n = (int)nsl[mod];
        Row<W> m;
        Row<W> pl[MODE == ROUTE_CUTS ? ROUTE_CUT_PLANES : 1];
        if constexpr (MODE == ROUTE_CUTS) m = route_and_cuts<W>(path_rec_load(P, pb + pth), sv.bm + (size_t)core * E * W, S, n, pl);
        else m = view_path_row<W>(P, sv.bm, pb + pth, core);
        nfree = row_popc<W>(m);
        // bit s: s .. s + n - 1 free on every hop (bits >= S of the AND-row are 0, so s + n <= S)
        const Row<W> r = row_runs_ge<W>(m, n);
        if (row_any<W>(r)) {
          if constexpr (MODE == ROUTE_CUTS) route_cuts_winner<W>(r, pl, slot, cost);
          else route_plain_winner<W>(rule, r, S, n, slot, cost);
        }
      }
    }
    if (q < total) table[v.env * total + q] = make_int4(slot, cost, n, nfree);
    int key = ORL_ROUTE_NO_FIT;
    if (cost != ORL_ROUTE_NO_FIT && (n_given < 1 || pth == gp) && (n_given < 2 || core == gc))
      key = key_cores(path_first, route == ORL_ROUTE_KSP ? 0 : (by_cost ? cost : S - nfree), pth, core, slot);
    key = g8_min(key);
    best = key < best ? key : best;
  }
  if (gl == 0) {
    const bool found = best != ORL_ROUTE_NO_FIT;
    const int bp = found ? key_cores_path(path_first, best) : 0;
    // m(p) of the chosen path once more, by this lane alone (the pairs' lanes had it; this spares an exchange per chunk)
    const int bmod = modulation >= 0 ? modulation : rmcsa_best_in_reach(P, nsl, P.path_length[pb + bp], br_idx);
    view_store_action<true>(P, v.env, found, make_int4(bp, bmod, key_cores_core(best), key_route_slot(best)));
  }
}
#endif
