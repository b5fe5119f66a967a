// orl_rmcsa_complete.h — first-fit completion of a partial RMCSA action (include/orl.h, orl_batch_complete_actions); included by
// orl_kernels.hip behind orl_view.h (the kernel's opening and the decode of the pending service are shared with the other views)
// and orl_rmcsa_mask.h (rmcsa_reach).
//
// The env's first g action columns — nothing, (p), (p, m) or (p, m, c) — are given; the kernel fills in the rest first-fit under
// prov(p, m, c, s) of orl_rmcsa_mask.h and writes all four columns of the env's row of ORL_BUF_ACTIONS:
//   g = 3  the lowest s with prov(p, m, c, s)
//   g = 2  the lowest column c S + s of the env's ORL_MASK_CORE_SLOT row for (p, m): cores in order, then slots
//   g = 1  m*(p) — the modulation within both reach limits for p that needs the fewest slots at this bit rate, ties to the lowest
//          index — then as g = 2.  "A run of >= n free slots exists" is monotone in n, so this provisions iff any column p M + . of
//          the ORL_MASK_PATH_MOD row is set
//   g = 0  the first path whose g = 1 completion exists
// No completion — a given column out of range (negative ones included), a pair beyond reach, no free run — is the reject action
// (K, M, C, S).  Nothing of the env is read but its scalar record and slot maps, nothing written but the row of actions.
//
// Layout of the work: 8 lanes per env, 8 envs per wavefront, 4 wavefronts per workgroup.  The candidate (path, core) pairs — one
// path or np of them, one core or C — are walked path-major in chunks of 8, as the RMCSA branch of policy_g does: per pair
// row_runs_ge of the path's AND-row in that core for the n of the pair's modulation, and its row_ctz.  A ballot over the group picks
// the lowest fitting pair; the group leaves at the first chunk that has one.  A path with no modulation within reach loads no link
// row.  Lane 0 of the group stores the row as 16 bytes.  No LDS, no atomics, no host synchronisation: graph-capturable.
// `given`: the prefix of env e at given[e * gstride + 0 .. g - 1] — the actions buffer itself with gstride 4 (every lane of the group
// has the prefix in registers before lane 0 stores the row: the store's value depends on those loads), or the batch's upload buffer.
#pragma once

// m*(p) for a path of length len: the modulation within reach with the fewest slots (lowest index among equals), -1 if none
__device__ __forceinline__ int rmcsa_best_in_reach(const DevParams& P, const unsigned char* nsl, double len, int br_idx) {
  int best = -1, nb = 0x7fffffff;
  for (int m = 0; m < P.M; m++) {
    const int n = (int)nsl[m];
    if (n < nb && rmcsa_reach(P, len, m, br_idx)) { best = m; nb = n; }
  }
  return best;
}

template <int W>
__global__ void __launch_bounds__(256) k_rmcsa_complete(DevParams P, int n_given, const int* given, int gstride) {
  const ViewLanes v = view_lanes();
  if (v.env >= P.B) return;  // (whole groups: the ballot and the exchanges below stay within a group)
  const int lane = v.lane, gl = v.gl;
  const int M = P.M, C = P.C;
  const PendingSvc sv = view_pending(P, v.env);
  const int br_idx = sv.br_idx, np = sv.np, pb = sv.pb;
  const unsigned char* nsl = P.nslots + br_idx * M;
  const int* gv = given + v.env * gstride;
  const int gp = n_given >= 1 ? gv[0] : 0, gm = n_given >= 2 ? gv[1] : 0, gc = n_given >= 3 ? gv[2] : 0;
  // the candidate paths [p0, p0 + n_p) and cores [c0, c0 + n_c); a given column out of range: none
  bool ok = true;
  int p0 = 0, n_p = np, c0 = 0, n_c = C;
  if (n_given >= 1) { ok = gp >= 0 && gp < np; p0 = gp; n_p = 1; }
  if (n_given >= 2) ok = ok && gm >= 0 && gm < M;
  if (n_given >= 3) { ok = ok && gc >= 0 && gc < C; c0 = gc; n_c = 1; }
  const int total = ok ? n_p * n_c : 0;
  int best = -1, bslot = 0, bmod = 0;
  for (int base = 0; base < total && best < 0; base += 8) {
    const int q = base + gl;
    int slot = -1, mod = -1;
    if (q < total) {
      const int pth = p0 + q / n_c, core = c0 + (q - (q / n_c) * n_c);
      const double len = P.path_length[pb + pth];
      if (n_given >= 2) mod = rmcsa_reach(P, len, gm, br_idx) ? gm : -1;
      else mod = rmcsa_best_in_reach(P, nsl, len, br_idx);
      if (mod >= 0) {
        // bit s: s .. s + n - 1 free on every hop (bits >= S of the AND-row are 0, so s + n <= S)
        const Row<W> r = row_runs_ge<W>(view_path_row<W>(P, sv.bm, pb + pth, core), (int)nsl[mod]);
        if (row_any<W>(r)) slot = row_ctz<W>(r);
      }
    }
    const u32 fit = g8::gballot(slot >= 0, lane);
    if (fit) {
      const int l = (int)__builtin_ctz(fit);
      best = base + l;
      bslot = g8::gget(slot, l, lane);
      bmod = g8::gget(mod, l, lane);
    }
  }
  if (gl == 0) view_store_action<true>(P, v.env, best >= 0, make_int4(p0 + best / n_c, bmod, c0 + (best - (best / n_c) * n_c), bslot));
}
