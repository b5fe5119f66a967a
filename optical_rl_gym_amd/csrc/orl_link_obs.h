// orl_link_obs.h — the per-link feature observation of the pending service (include/orl.h, orl_batch_link_features); included by
// orl_kernels.hip behind orl_view.h (the kernel's opening, the decode of the pending service and the row header are shared
// with the other views and live there; the LDS budget rule: orl_view_plan.h).
//
// Per env one row of dim = 1 + 2 N + R F float32 values at a device pitch of round_up(dim, 4) floats; consecutive envs are
// contiguous.  The header is the path features' {bit_rate / 100 (RWA: 0), one-hot min(src, dst), one-hot max(src, dst)}; then one
// block of F = 10 + k values per slot row, R = C E blocks in the order of the slot maps (block r = c E + l, C = 1 outside RMCSA, l the
// link index of the topology's path_links).  With a = the free-slot row, S its slots, f = popcount(a):
//   [0] f / S      [1] maximal free runs / S      [2] longest free run / S
//   [3] first free slot / S, [4] (last free slot + 1) / S; both -1 when f == 0
//   [5] cur_external_fragmentation, [6] cur_link_compactness of the row as it stands (rmsa_env.py:492-528): the expressions the row
//       phase feeds into the running averages (orl_device_split.h), from the same integers (sp::row_stat_lane, non-cached form)
//   [7 .. 9] the link's running utilization, external_fragmentation and compactness (DevParams::lstat), cast to float32
//   [10 + p] 1.0 when the link is on candidate path p < n_paths[src, dst] of the pending pair, else 0.0
// Every value is computed in float64 and rounded to float32 once.  Pad columns are 0.  Nothing of the env is written.
//
// Layout of the work: 8 lanes per env, 8 envs per wavefront (view_lanes).  First the env's lanes turn the pending pair's path
// records into k link sets of 128 bits each in LDS (lane = path); then the rows r = gl, gl + 8, ... are striped over the env's lanes:
// the row's W words and the link's statistics record sit in the lane's registers, the link sets are read back as LDS broadcasts.
// Where the blocks go — always through LDS, two forms chosen by the launcher from the shape:
//   whole (chunk == 0)  the wavefront's 8 rows (8 pitch floats, contiguous in the output too) are assembled in LDS and streamed as
//                       16-byte stores; 1 / 2 / 4 wavefronts per workgroup, what 48 KiB of LDS allow (view_waves)
//   chunked (chunk > 0) the shapes whose 8 rows do not fit (RMCSA with 7 cores on 22 links: 9.4 kB per env): the header goes straight
//                       to memory, the blocks in rounds of `chunk` slot rows per env (a multiple of 8: every lane of the env does
//                       chunk / 8 of them) through LDS, each env's range of a round streamed as consecutive 4-byte stores, 256
//                       bytes per instruction
// (A third form, every lane storing its own blocks at a stride of 10 + k floats between lanes, lost to these at every shape
// measured — DESIGN 4.5, profiles/link_obs_rate_direct.jsonl — and is not kept.)
// No atomics, no host synchronisation: graph-capturable.
#pragma once

// (the row's shape: orl_view_plan.h, view_shape)

// LDS bytes of one wavefront: its 8 envs' K link sets of two words each, then `floats` floats of staging for each of the 8 envs (whole:
// the pitch; chunked: chunk x (10 + K))
__host__ __device__ inline size_t link_obs_wave_lds(int K, int floats) {
  return (size_t)8 * 2 * K * sizeof(u64) + (size_t)8 * floats * sizeof(float);
}

#ifdef ORL_W  // (the kernel: the per-W units, orl_kernels.hip; the API unit takes the size above for its view_plan)
// one slot row's block: the 10 + K values of row `a` of link l; ls: the link's record of DevParams::lstat, pm: the env's K link sets
template <int W>
__device__ __forceinline__ void link_obs_block(const Row<W>& a, int S, const sp::Recip& rS, const double* ls, const u64* pm, int l, int K,
                                               float* o) {
  RowStat st;
  int max_empty = 0, edge = 0;
  sp::row_stat_lane<W>(a.w, S, st, max_empty, edge);
  const int f = st.free_;
  int last = 0;  // last free slot + 1
#pragma unroll
  for (int w = 0; w < W; w++) last = a.w[w] ? 64 * w + 64 - (int)__builtin_clzll(a.w[w]) : last;
  double frag = 0.0, comp = 0.0;
  if (f > 0) {
    const int me = (st.nf > 1 && !(st.nf == 2 && edge == 2)) ? max_empty : 0;
    frag = 1.0 - sp::div_pos((double)me, (double)f);
    comp = st.nu > 1 ? sp::div_pos((double)(st.hi - st.lo), (double)(S - f)) * sp::div_pos(1.0, (double)st.nu) : 1.0;
  }
  const double2 l01 = *(const double2*)ls;
  const double l2 = ls[2];
  o[0] = (float)sp::div_by((double)f, rS);
  o[1] = (float)sp::div_by((double)st.nf, rS);
  o[2] = (float)sp::div_by((double)max_empty, rS);
  o[3] = f > 0 ? (float)sp::div_by((double)row_ctz<W>(a), rS) : -1.0f;
  o[4] = f > 0 ? (float)sp::div_by((double)last, rS) : -1.0f;
  o[5] = (float)frag;
  o[6] = (float)comp;
  o[7] = (float)l01.x;
  o[8] = (float)l01.y;
  o[9] = (float)l2;
  const u64* word = pm + (l >> 6);
  const int bit = l & 63;
  for (int p = 0; p < K; p++) o[10 + p] = ((word[2 * p] >> bit) & 1ull) ? 1.0f : 0.0f;
}

template <int W>
__global__ void __launch_bounds__(256) k_link_features(DevParams P, float* out, int dim, int pitch, int chunk) {
  const ViewLanes v = view_lanes();
  const int lane = v.lane, gl = v.gl, el = lane >> 3;
  const i64 env0 = v.env0, env = v.env;
  const int K = P.K, E = P.E, S = P.S, N = P.N;
  const int C = P.env_type == ENV_RMCSA ? P.C : 1, R = C * E, F = 10 + K;
  // the wavefront's LDS: the 8 envs' link sets (K x 2 words each), then the staging of its 8 envs (sf floats each)
  const int sf = chunk ? chunk * F : pitch;
  unsigned char* lds = orl_lds_raw + (size_t)v.wv * link_obs_wave_lds(K, sf);
  u64* pm = (u64*)lds + el * 2 * K;
  float* stage = (float*)(lds + 8 * 2 * K * sizeof(u64));
  float* row = out + env * pitch;                  // the env's output row (env < B)
  float* o = chunk ? row : stage + el * pitch;      // where its header and pad go, and — whole — its blocks
  const bool live = env < P.B;
  PendingSvc sv;
  if (live) {
    sv = view_pending(P, env);
    for (int p = gl; p < K; p += 8) {
      u64 lo = 0ull, hi = 0ull;
      if (p < sv.np) {
        const PathRec rec = path_rec_load(P, sv.pb + p);
        const int hops = path_rec_byte(rec, 0);
        for (int h = 0; h < hops; h++) {
          const int l = path_rec_byte(rec, 2 + h);  // < E <= 128
          lo |= l < 64 ? 1ull << l : 0ull;
          hi |= l < 64 ? 0ull : 1ull << (l - 64);
        }
      }
      pm[2 * p] = lo;
      pm[2 * p + 1] = hi;
    }
    view_obs_header(sv, N, P.env_type == ENV_RWA, gl, dim, pitch, o);
  }
  wave_fence();
  const sp::Recip rS = sp::recip_of((double)S);
  const double* ls = P.lstat + env * 4 * E;
  const int head = 1 + 2 * N;
  if (chunk) {
    const i64 left = P.B - env0;
    const int n_el = (int)(left < 8 ? (left < 0 ? 0 : left) : 8);
    for (int r0 = 0; r0 < R; r0 += chunk) {
      const int r1 = r0 + chunk < R ? r0 + chunk : R;
      if (live)
        for (int r = r0 + gl; r < r1; r += 8)
          link_obs_block<W>(row_load<W>(sv.bm + (size_t)r * W), S, rS, ls + 4 * (r % E), pm, r % E, K, stage + el * sf + (r - r0) * F);
      wave_fence();
      // env e's blocks r0 .. r1 - 1 are one contiguous range of its row: one float per lane and store
      const int nf = (r1 - r0) * F;
      for (int e = 0; e < n_el; e++) {
        float* dst = out + (env0 + e) * pitch + head + r0 * F;
        const float* src = stage + e * sf;
        for (int i = lane; i < nf; i += 64) dst[i] = src[i];
      }
      wave_fence();  // (the next round overwrites the staging)
    }
    return;
  }
  if (live)
    for (int r = gl; r < R; r += 8)
      link_obs_block<W>(row_load<W>(sv.bm + (size_t)r * W), S, rS, ls + 4 * (r % E), pm, r % E, K, o + head + r * F);
  wave_fence();
  // the wavefront's rows are one contiguous range of the output: 4 floats per lane and store
  const i64 left = P.B - env0;
  const int nch = (int)(left < 8 ? (left < 0 ? 0 : left) : 8) * (pitch >> 2);
  uint4* dst4 = (uint4*)(out + env0 * pitch);
  const uint4* src4 = (const uint4*)stage;
  for (int g = lane; g < nch; g += 64) dst4[g] = src4[g];
}
#endif
