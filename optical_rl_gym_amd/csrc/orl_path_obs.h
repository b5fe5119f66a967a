// orl_path_obs.h — the path-feature observation of the pending service (include/orl.h, orl_batch_path_features); included by
// orl_kernels.hip behind orl_view.h (the kernel's opening, the decode of the pending service and the LDS budget rule are shared
// with the other views and live there).
//
// Per env one row of dim = 1 + 2 N + R (2 j + 3) float32 values at a device pitch of round_up(dim, 4) floats; consecutive envs are
// contiguous.  The row is DeepRMSAEnv.observation (deeprmsa_env.py:60-121) with a block count j of the call's own, for every
// slot-map family: the header {bit_rate / 100 (RWA: 0), one-hot min(src, dst), one-hot max(src, dst)}, then one block of 2 j + 3
// values per row r — R = k rows (r = path) for RMSA, DeepRMSA and RWA, R = k C rows (r = p C + c, path-major as rmcsa_env.py:889-906)
// for RMCSA.  With m = the AND of the path's link rows in the core and n = the slots the service needs (RMSA / DeepRMSA: under the
// path's best modulation; RWA: 1; RMCSA: under the path's best modulation, or under modulation `mod` for every path when mod >= 0):
//   [2 b], [2 b + 1]  start and length of the b-th maximal free run of >= n slots, b < j: 2 (start - 0.5 S) / S, (length - 8) / 8
//   [2 j]             (n - 5.5) / 3.5
//   [2 j + 1]         2 (popcount(m) - 0.5 S) / S
//   [2 j + 2]         (popcount(m) / runs(m) - 4) / 4 when m has a free run
// and -1.0 wherever a value does not exist (a block beyond the last fitting run, a path index >= n_paths[src, dst]).  Every value
// is computed in float64 with the reference's expression, as obs8_env_w does, and rounded to float32 once.  Pad columns are 0.
// Nothing of the env is written.
//
// Layout of the work, as k_action_mask and k_obs8: 8 lanes per env, 8 envs per wavefront; the rows r = gl, gl + 8, ... are striped
// over the env's lanes, each of which ANDs its path's link rows straight from global memory.  Where the rows go:
//   staged  the wavefront's 8 rows (8 pitch floats, contiguous in the output too) are assembled in LDS and streamed as 16-byte
//           stores; 1 / 2 / 4 wavefronts per workgroup, what 48 KiB of LDS allow (view_waves)
//   direct  every lane stores its own blocks, one float per store — the shapes whose 8 rows do not fit (RMCSA with 31 cores and
//           j = 8: 11.8 kB per env); -DORL_PATH_OBS_STAGE=0 builds it for every shape (the A/B of DESIGN 4.5)
// No atomics, no host synchronisation: graph-capturable.
#pragma once

// (the row's shape and ORL_PATH_OBS_STAGE: orl_view_plan.h, view_shape / view_plan)

// one row's block: the 2 j + 3 values of the free-slot row m for a service of n slots
template <int W>
__device__ __forceinline__ void path_obs_block(const Row<W>& m, int n, int S, int J, float* o) {
  Row<W> r = row_runs_ge<W>(m, n);  // bit s: slots s .. s + n - 1 free
  const Row<W> zeros = row_andn<W>(row_mask_lo<W>(S), m);
  for (int b = 0; b < J; b++) {
    float f0 = -1.0f, f1 = -1.0f;
    if (row_any<W>(r)) {
      const int st = row_ctz<W>(r);
      const Row<W> z = row_andn<W>(zeros, row_mask_lo<W>(st));
      const int end = row_any<W>(z) ? row_ctz<W>(z) : S;
      f0 = (float)(2 * ((double)st - 0.5 * (double)S) / (double)S);
      f1 = (float)((double)(end - st - 8) / 8);
      r = row_andn<W>(r, row_mask_lo<W>(end));
    }
    o[2 * b] = f0;
    o[2 * b + 1] = f1;
  }
  const int tot = row_popc<W>(m), nruns = row_popc<W>(row_starts<W>(m));
  o[2 * J] = (float)(((double)n - 5.5) / 3.5);
  o[2 * J + 1] = (float)(2 * ((double)tot - 0.5 * (double)S) / (double)S);
  o[2 * J + 2] = nruns > 0 ? (float)(((double)tot / (double)nruns - 4) / 4) : -1.0f;
}

// the env's row into o (LDS or global): header and pad by the group's lanes, then the blocks r = gl, gl + 8, ...
template <int W>
__device__ __forceinline__ void path_obs_env(const DevParams& P, i64 env, int gl, int J, int mod, int dim, int pitch, float* o) {
  const PendingSvc sv = view_pending(P, env);
  const int br_idx = sv.br_idx, np = sv.np, pb = sv.pb;
  const u64* bm = sv.bm;
  const int N = P.N, K = P.K, S = P.S, WD = 2 * J + 3;
  const bool rwa = P.env_type == ENV_RWA, rmcsa = P.env_type == ENV_RMCSA;
  const int C = rmcsa ? P.C : 1, R = K * C;
  view_obs_header(sv, N, rwa, gl, dim, pitch, o);
  for (int r = gl; r < R; r += 8) {
    const int p = r / C, core = r - p * C;
    float* blk = o + 1 + 2 * N + r * WD;
    if (p < np) {
      const int pidx = pb + p;
      const Row<W> m = view_path_row<W>(P, bm, pidx, core);
      const int n = (rmcsa && mod >= 0) ? (int)P.nslots[br_idx * P.M + mod] : view_need(P, sv, pidx, rwa);
      path_obs_block<W>(m, n, S, J, blk);
    } else {
      for (int i = 0; i < WD; i++) blk[i] = -1.0f;
    }
  }
}

template <int W>
__global__ void __launch_bounds__(256) k_path_features(DevParams P, float* out, int J, int mod, int dim, int pitch, int staged) {
  const ViewLanes v = view_lanes();
  const int lane = v.lane, gl = v.gl;
  const i64 env0 = v.env0, env = v.env;
  if (!staged) {
    if (env < P.B) path_obs_env<W>(P, env, gl, J, mod, dim, pitch, out + env * pitch);
    return;
  }
  float* lds = (float*)orl_lds_raw + (size_t)v.wv * 8 * pitch;
  if (env < P.B) path_obs_env<W>(P, env, gl, J, mod, dim, pitch, lds + (lane >> 3) * pitch);
  wave_fence();
  // the wavefront's rows are one contiguous range of the output: 4 floats per lane and store
  const i64 left = P.B - env0;
  const int nch = (int)(left < 8 ? (left < 0 ? 0 : left) : 8) * (pitch >> 2);
  uint4* dst4 = (uint4*)(out + env0 * pitch);
  const uint4* src4 = (const uint4*)lds;
  for (int g = lane; g < nch; g += 64) dst4[g] = src4[g];
}
