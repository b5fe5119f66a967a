// orl_blocks.h — block actions: DeepRMSA's (row, free block) action space for every slot-map family (include/orl.h,
// orl_batch_block_table, orl_batch_select_blocks); included by orl_kernels.hip behind orl_view.h (the kernels' opening, the decode of
// the pending service, the rows' way from LDS to memory) and orl_rmcsa_complete.h (m*(p): rmcsa_best_in_reach; rmcsa_reach of
// orl_rmcsa_mask.h).
//
// For the pending service of an env and every row r of the path features' row order — r = p for RMSA, DeepRMSA and RWA, r = p C + c
// for RMCSA — with n(r) and row(r) of orl_batch_route_spectrum / orl_batch_route_cores, the blocks of r are the maximal free runs of
// row(r) of >= n(r) slots in slot order, block b = (start_b, L_b).
//   k_block_table   the first j blocks of every row as int32 (n, free, start_0, L_0, ..., start_{j-1}, L_{j-1}), (S, 0) for a block
//                   that does not exist, (0, 0, S, 0, ...) for a row the service cannot use (p >= n_paths, no modulation within
//                   reach), which loads no link row; per env R (2 + 2 j) int32 at a pitch of round_up(., 4), pad 0.  And the mask
//                   of the action space Discrete(R j + 1): column r j + b = block b of row r exists; the reject column and the
//                   fallback are those of orl_mask.h.
//   k_select_blocks a flat index a per env -> (r, b) = (a / j, a % j) -> the env's row of ORL_BUF_ACTIONS: first slot start_b
//                   (ORL_BLOCK_FIRST) or start_b + L_b - n (ORL_BLOCK_LAST); the family's reject row for an index out of range or a
//                   block that does not exist.  It recomputes from the slot maps and reads no table.
//
// Layout of the work, k_block_table: as k_path_features — 8 lanes per env, 8 envs per wavefront, the rows r = gl, gl + 8, ...
// striped over the env's lanes, each of which ANDs its row straight from global memory.  Where the table rows go:
//   staged  the wavefront's 8 env rows (8 pitch int32, contiguous in the output too) are assembled in LDS and streamed as 16-byte
//           stores; 1 / 2 / 4 wavefronts per workgroup, what 48 KiB of LDS allow beside the mask's bit rows (view_waves)
//   direct  every lane stores its own rows, 8 bytes per store — the shapes whose 8 rows do not fit (RMCSA with 31 cores and j = 8:
//           11 kB per env)
// The mask leaves as one u32 of j bits per row in LDS and view_store_rows in both forms.  k_select_blocks: one row per env, the
// group's 8 lanes all walk it (whole groups stay alive, as in the siblings) and lane 0 stores.  No atomics, no host
// synchronisation: graph-capturable.  Env state and flags are only read.
#pragma once

// u32 words of LDS one env's mask takes: one word of j <= 8 bits per row, a pad word (read past the last row's end, masked off)
// and the env's "has a provisioning column" flag — the image view_store_rows reads
__host__ __device__ inline int blocks_mask_env_words(int R) { return R + 2; }

#ifdef ORL_W  // (the kernels: the per-W units, orl_kernels.hip; the API unit takes the size above for its view_plan)
// The next fitting run: r = row_runs_ge(m, n) less the runs already taken, zeros = the occupied slots of m below S.  false: none is
// left; else [st, end) is the lowest maximal free run of >= n slots, and it is taken out of r (the steps of path_obs_block)
template <int W>
__device__ __forceinline__ bool block_next_run(Row<W>& r, const Row<W>& zeros, int S, int& st, int& end) {
  if (!row_any<W>(r)) return false;
  st = row_ctz<W>(r);
  const Row<W> z = row_andn<W>(zeros, row_mask_lo<W>(st));
  end = row_any<W>(z) ? row_ctz<W>(z) : S;
  r = row_andn<W>(r, row_mask_lo<W>(end));
  return true;
}

// n(r) of row r's path p (< np is the caller's to check) and, RMCSA, its modulation m(p) into `mod`; 0: the service cannot use p
__device__ __forceinline__ int block_need(const DevParams& P, const PendingSvc& sv, int p, int modulation, bool rwa, bool rmcsa, int& mod) {
  mod = 0;
  if (!rmcsa) return view_need(P, sv, sv.pb + p, rwa);
  const unsigned char* nsl = P.nslots + sv.br_idx * P.M;
  const double len = P.path_length[sv.pb + p];
  if (modulation >= 0) mod = rmcsa_reach(P, len, modulation, sv.br_idx) ? modulation : -1;
  else mod = rmcsa_best_in_reach(P, nsl, len, sv.br_idx);
  return mod >= 0 ? (int)nsl[mod] : 0;
}

// the env's table row into o (LDS or global, 8-byte aligned) and its mask words into mw, by the group's lanes; returns whether one of
// this lane's rows has a block
template <int W>
__device__ __forceinline__ int block_table_env(const DevParams& P, i64 env, int gl, int J, int modulation, int dim, int pitch, int* o, u32* mw) {
  const PendingSvc sv = view_pending(P, env);
  const int K = P.K, S = P.S, WD = 2 + 2 * J;
  const bool rwa = P.env_type == ENV_RWA, rmcsa = P.env_type == ENV_RMCSA;
  const int C = rmcsa ? P.C : 1, R = K * C;
  const int np = sv.np < K ? sv.np : K;
  for (int i = dim + gl; i < pitch; i += 8) o[i] = 0;
  int any = 0;
  for (int r = gl; r < R; r += 8) {
    const int p = r / C, core = r - p * C;
    int2* row = (int2*)(o + r * WD);
    int mod, n = 0, nfree = 0, nb = 0;
    if (p < np) n = block_need(P, sv, p, modulation, rwa, rmcsa, mod);
    if (n > 0) {
      const Row<W> m = view_path_row<W>(P, sv.bm, sv.pb + p, core);
      nfree = row_popc<W>(m);
      Row<W> f = row_runs_ge<W>(m, n);  // bit s: slots s .. s + n - 1 free
      const Row<W> zeros = row_andn<W>(row_mask_lo<W>(S), m);
      int st, end;
      while (nb < J && block_next_run<W>(f, zeros, S, st, end)) row[1 + nb++] = make_int2(st, end - st);
    }
    row[0] = make_int2(n, nfree);
    for (int b = nb; b < J; b++) row[1 + b] = make_int2(S, 0);
    mw[r] = (1u << nb) - 1u;
    any |= nb;
  }
  return any != 0;
}

template <int W>
__global__ void __launch_bounds__(256) k_block_table(DevParams P, int* table, unsigned char* mask, int J, int modulation, int dim, int pitch, int mpitch,
                                                     int staged) {
  const ViewLanes v = view_lanes();
  const int lane = v.lane, gl = v.gl;
  const int R = (P.env_type == ENV_RMCSA ? P.C : 1) * P.K, ew = blocks_mask_env_words(R);
  // LDS of the workgroup: the wavefronts' table rows (staged), behind them their mask images
  int* tl = (int*)orl_lds_raw + (size_t)v.wv * 8 * pitch;
  u32* ml = (u32*)orl_lds_raw + (staged ? (size_t)v.waves * 8 * pitch : 0) + (size_t)v.wv * 8 * ew;
  u32* mine = ml + (lane >> 3) * ew;
  int any = 0;
  if (v.env < P.B) any = block_table_env<W>(P, v.env, gl, J, modulation, dim, pitch, staged ? tl + (lane >> 3) * pitch : table + v.env * pitch, mine);
  any = g8_max(any);
  if (gl == 0) { mine[R] = 0u; mine[R + 1] = (u32)any; }
  wave_fence();
  if (staged) {  // the wavefront's table rows are one contiguous range of the output: 4 int32 per lane and store
    const i64 left = P.B - v.env0;
    const int nch = (int)(left < 8 ? (left < 0 ? 0 : left) : 8) * (pitch >> 2);
    uint4* dst4 = (uint4*)(table + v.env0 * pitch);
    const uint4* src4 = (const uint4*)tl;
    for (int g = lane; g < nch; g += 64) dst4[g] = src4[g];
  }
  view_store_rows(ml, R, 1, J, ew, R, P.allow_rejection, v.env0, P.B, mask, mpitch);
}

// `given`: the index of env e at given[e * gstride] — the actions buffer itself with gstride 4 (every lane of the group has it in a
// register before lane 0 stores the row: the store's value depends on that load), or the batch's upload buffer (gstride 1)
template <int W>
__global__ void __launch_bounds__(256) k_select_blocks(DevParams P, int J, int modulation, int placement, const int* given, int gstride) {
  const ViewLanes v = view_lanes();
  if (v.env >= P.B) return;  // (whole groups)
  const int K = P.K, S = P.S;
  const bool rwa = P.env_type == ENV_RWA, rmcsa = P.env_type == ENV_RMCSA;
  const int C = rmcsa ? P.C : 1, R = K * C;
  const int a = given[v.env * gstride];
  const PendingSvc sv = view_pending(P, v.env);
  const int np = sv.np < K ? sv.np : K;
  const bool in_range = a >= 0 && a < R * J;
  const int r = in_range ? a / J : 0, b = a - r * J;
  const int p = r / C, core = r - p * C;
  int mod = 0, n = 0, slot = S;
  bool found = false;
  if (in_range && p < np) n = block_need(P, sv, p, modulation, rwa, rmcsa, mod);
  if (n > 0) {
    const Row<W> m = view_path_row<W>(P, sv.bm, sv.pb + p, core);
    Row<W> f = row_runs_ge<W>(m, n);
    const Row<W> zeros = row_andn<W>(row_mask_lo<W>(S), m);
    int st = 0, end = 0, i = 0;
    found = true;
    for (; i <= b && found; i++) found = block_next_run<W>(f, zeros, S, st, end);
    slot = placement == ORL_BLOCK_LAST ? end - n : st;
  }
  if (v.gl == 0) {
    if (rmcsa) view_store_action<true>(P, v.env, found, make_int4(p, mod, core, slot));
    else view_store_action<false>(P, v.env, found, make_int4(p, slot, 0, 0));
  }
}
#endif
