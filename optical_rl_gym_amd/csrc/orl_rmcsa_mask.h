// orl_rmcsa_mask.h — the two-stage action masks of RMCSA's pending service (include/orl.h, ORL_MASK_PATH_MOD / ORL_MASK_CORE_SLOT);
// included by orl_kernels.hip behind orl_view.h (the kernel's opening, the decode of the pending service and the rows' way from
// LDS to memory are shared with the other views and live there; the LDS budget rule: orl_view_plan.h).
//
// An RMCSA action is (path p, modulation m, core c, first slot s).  With n = nslots[br_idx][m], stepping it provisions iff
// (rmcsa_env.py:209-289 with is_path_free :767-794, get_number_slots :753-765, _crosstalk_is_acceptable :341-384)
//   p < n_paths[src, dst], m < M, c < C, s + n <= S, slots s .. s + n - 1 free in core c on every hop of p, and
//   length(p) < lmax_xt[m] and length(p) < lmax_snr[m][br_idx]
// — `prov(p, m, c, s)`.  The test factorises, and so do the masks.  Rows as orl_mask.h: `dim` bytes of 0/1 at a pitch of
// round_up(dim, 16), the last column (reject) = allow_rejection, and the same fallback rule.
//   ORL_MASK_PATH_MOD   dim = k M + 1: column p M + m = some (c, s) has prov(p, m, c, s)
//   ORL_MASK_CORE_SLOT  dim = C S + 1: column c S + s = prov(p, m, c, s) for the env's given (p, m) = given[env * stride + 0 / 1];
//                       a pair out of range (negative ones included) or beyond reach has no provisioning column
// Nothing of the env is written.
//
// Layout of the work, as k_action_mask: 8 lanes per env, 8 envs per wavefront, 1 / 2 / 4 wavefronts per workgroup (what the LDS
// rows allow: view_waves).
//   PATH_MOD   "a run of >= n free slots exists" is monotone in n, so one number per (path, core) serves every modulation: the
//              longest free run of the AND of the path's link rows in that core.  Lanes walk the (path, core) pairs path-major as
//              the RMCSA branch of policy_g and leave the runs in LDS; pairs of a path that no modulation reaches at this bit rate
//              load nothing.  Then lane = path: the largest run over the cores against nslots of each modulation within reach, M
//              bits into the path's word.
//   CORE_SLOT  lane = core: row_runs_ge of the given path's AND-row in that core, for the given modulation's n.
// Then the wavefront streams its 8 envs' rows as 16-byte stores (view_store_rows of orl_view.h: a 16-column chunk is a 16-bit
// field of the env's bit rows, expanded to bytes in registers).  No atomics, no host synchronisation: graph-capturable.
#pragma once

// u32 words of LDS per env: `rows` bit rows of `rw` words, a pad word, the "has a provisioning column" flag; PATH_MOD: the k C
// longest runs before them
__host__ __device__ inline int rmcsa_mask_rows(int layout, int K, int C) { return layout == ORL_MASK_PATH_MOD ? K : C; }
__host__ __device__ inline int rmcsa_mask_row_words(int layout, int W) { return layout == ORL_MASK_PATH_MOD ? 1 : 2 * W; }
__host__ __device__ inline int rmcsa_mask_env_words(int layout, int W, int K, int C) {
  return rmcsa_mask_rows(layout, K, C) * rmcsa_mask_row_words(layout, W) + 2 + (layout == ORL_MASK_PATH_MOD ? K * C : 0);
}
#ifdef ORL_W  // (the kernel: the per-W units, orl_kernels.hip; the API unit takes the size above for its view_plan)
// is modulation m within both reach limits for a path of length len at bit-rate index br_idx?
__device__ __forceinline__ bool rmcsa_reach(const DevParams& P, double len, int m, int br_idx) {
  return len < P.lmax_xt[m] && len < P.lmax_snr[m * P.n_br + br_idx];
}

template <int W>
__global__ void __launch_bounds__(256) k_rmcsa_mask(DevParams P, unsigned char* out, int layout, int pitch, const int* given, int gstride) {
  const ViewLanes v = view_lanes();
  const int lane = v.lane, gl = v.gl;
  const int K = P.K, S = P.S, M = P.M, C = P.C;
  const bool pm = layout == ORL_MASK_PATH_MOD;
  const int nrows = rmcsa_mask_rows(layout, K, C), rw = rmcsa_mask_row_words(layout, W), ew = rmcsa_mask_env_words(layout, W, K, C);
  const int cpp = pm ? M : S;  // columns per bit row
  u32* lds = (u32*)orl_lds_raw + (size_t)v.wv * 8 * ew;
  u32* mine = lds + (lane >> 3) * ew;
  int any = 0;
  if (v.env < P.B) {
    const PendingSvc sv = view_pending(P, v.env);
    const int br_idx = sv.br_idx, np = sv.np, pb = sv.pb;
    const u64* bm = sv.bm;
    const unsigned char* nsl = P.nslots + br_idx * M;
    if (pm) {
      u32* runs = mine + nrows * rw + 2;  // [np][C] longest free runs
      for (int q = gl; q < np * C; q += 8) {
        const int pth = q / C, core = q - pth * C;
        const double len = P.path_length[pb + pth];
        bool reach = false;
        for (int m = 0; m < M; m++) reach = reach || rmcsa_reach(P, len, m, br_idx);
        int run = 0;
        if (reach) run = row_longest_run<W>(view_path_row<W>(P, bm, pb + pth, core));
        runs[q] = (u32)run;
      }
      wave_fence();
      for (int p = gl; p < K; p += 8) {
        u32 bits = 0u;
        if (p < np) {
          int run = 0;
          for (int c = 0; c < C; c++) run = max(run, (int)runs[p * C + c]);
          const double len = P.path_length[pb + p];
          for (int m = 0; m < M; m++)
            if ((int)nsl[m] <= run && rmcsa_reach(P, len, m, br_idx)) bits |= 1u << m;
        }
        any |= bits ? 1 : 0;
        mine[p] = bits;
      }
    } else {
      const int p = given[v.env * gstride], m = given[v.env * gstride + 1];
      const bool ok = p >= 0 && p < np && m >= 0 && m < M && rmcsa_reach(P, P.path_length[pb + p], m, br_idx);
      const PathRec prec = path_rec_load(P, pb + (ok ? p : 0));
      const int n = ok ? (int)nsl[m] : 1;
      for (int c = gl; c < C; c += 8) {
        Row<W> r = row_mask_lo<W>(0);
        if (ok) r = row_runs_ge<W>(path_and_rec<W>(prec, bm, P.E, S, c), n);  // bit s: s .. s + n - 1 free on every hop (bits >= S are 0)
        any |= row_any<W>(r) ? 1 : 0;
        row_store<W>((u64*)(mine + c * rw), r);
      }
    }
  }
  any = g8_max(any);
  if (gl == 0) { mine[nrows * rw] = 0u; mine[nrows * rw + 1] = (u32)any; }
  wave_fence();
  view_store_rows(lds, nrows, rw, cpp, ew, nrows * rw, P.allow_rejection, v.env0, P.B, out, pitch);
}
#endif
