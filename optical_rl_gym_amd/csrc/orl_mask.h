// orl_mask.h — action masks of the pending service (include/orl.h, orl_batch_action_mask); included by orl_kernels.hip behind
// orl_view.h, which holds what this view shares with the others: the kernel's opening (view_lanes), the decode of the pending service
// (view_pending) and the rows' way from LDS to memory (view_store_rows); the LDS budget rule (view_waves) is orl_view_plan.h's.
//
// Per env, one row of `dim` bytes (0/1) at a device pitch of round_up(dim, 16); consecutive envs are contiguous.
//   ORL_MASK_JOINT  RMSA / RWA: column p * S + s = action (path p, first slot / wavelength s); DeepRMSA: column p * j + b = action
//                   p * j + b.  A column is 1 iff stepping that action provisions the service: is_path_free (rmsa_env.py:163-200,
//                   623-636), the wavelength test of rwa_env.py:101-135 (385-400), get_available_blocks (deeprmsa_env.py:48-58,
//                   rmsa_env.py:667-697: block b of path p exists iff b < min(j, maximal free runs of >= n slots)).
//   ORL_MASK_PATH   PathOnlyFirstFitAction: column p = the wrapper's first fit finds a slot on path p — RMSA searches
//                   range(0, S - n) only (rmsa_env.py:848-871), RWA every wavelength (rwa_env.py:518-533).
// A path index >= n_paths[src, dst] is 0 (the reference raises IndexError).  The last column (reject) = allow_rejection.
// Fallback: a row with no provisioning column and allow_rejection == 0 gets every non-reject column set (every action of the
// space then rejects; a masked categorical never sees an all -inf row).
//
// Layout of the work: 8 lanes per env, lane = path (p = gl, gl + 8, ... for k > 8), 8 envs per wavefront, as k_obs8.  Each lane
// ANDs its path's link rows straight from global memory and leaves the path's columns as a bit row in LDS; then the wavefront
// streams its 8 envs' output rows (8 * pitch contiguous bytes) as 16-byte stores (view_store_rows: a 16-column chunk is a 16-bit
// field of the env's bitstring, expanded to bytes in registers).  4 wavefronts per workgroup: the launcher refuses the shapes whose
// rows do not allow them.  No atomics, no host synchronisation: graph-capturable.
#pragma once

// u32 words of LDS one env's bit rows take: k rows of `rw` words, a pad word (read past the last row's end, masked off) and
// the env's "has a provisioning column" flag.  rw: a whole slot row (joint RMSA / RWA), else one u64 (j <= 64 blocks, 1 bit).
__host__ __device__ inline int mask_row_words(int layout, int env_type, int W) {
  return (layout == ORL_MASK_JOINT && env_type != orl::ENV_DEEPRMSA) ? 2 * W : 2;
}
__host__ __device__ inline int mask_env_words(int layout, int env_type, int W, int K) { return K * mask_row_words(layout, env_type, W) + 2; }

#ifdef ORL_W  // (the kernel: the per-W units, orl_kernels.hip; the API unit takes the size above for its view_plan)
template <int W>
__global__ void __launch_bounds__(256) k_action_mask(DevParams P, unsigned char* out, int layout, int pitch) {
  const ViewLanes v = view_lanes();
  const int lane = v.lane, gl = v.gl;
  const int K = P.K, S = P.S, J = P.J;
  const bool deep = P.env_type == ENV_DEEPRMSA, rwa = P.env_type == ENV_RWA, path_layout = layout == ORL_MASK_PATH;
  const int rw = mask_row_words(layout, P.env_type, W), ew = K * rw + 2;
  const int cpp = path_layout ? 1 : (deep ? J : S);  // columns per path
  u32* lds = (u32*)orl_lds_raw + (size_t)v.wv * 8 * ew;
  u32* mine = lds + (lane >> 3) * ew;
  int any = 0;
  if (v.env < P.B) {
    const PendingSvc sv = view_pending(P, v.env);
    for (int p = gl; p < K; p += 8) {
      Row<W> r = row_mask_lo<W>(0);
      if (p < sv.np) {
        const int pidx = sv.pb + p;
        const Row<W> m = view_path_row<W>(P, sv.bm, pidx, 0);
        const int n = view_need(P, sv, pidx, rwa);
        r = row_runs_ge<W>(m, n);  // bit s: slots s .. s + n - 1 free on every hop (bits >= S are 0: s + n <= S)
        if (deep) {
          const int nb = row_popc<W>(row_and<W>(row_starts<W>(m), r));  // maximal free runs of >= n slots
          r = row_mask_lo<W>(nb < J ? nb : J);
        } else if (path_layout) {
          if (!rwa) r = row_and<W>(r, row_mask_lo<W>(S - n));
          r = row_mask_lo<W>(row_any<W>(r) ? 1 : 0);
        }
      }
      any |= row_any<W>(r) ? 1 : 0;
      u64* row = (u64*)(mine + p * rw);
      if (rw == 2 * W) row_store<W>(row, r);
      else row[0] = r.w[0];
    }
  }
  any = g8_max(any);
  if (gl == 0) { mine[K * rw] = 0u; mine[K * rw + 1] = (u32)any; }
  wave_fence();
  view_store_rows(lds, K, rw, cpp, ew, K * rw, P.allow_rejection, v.env0, P.B, out, pitch);
}
#endif
