// orl_qos_obs.h — MatrixObservationWithPaths (qos_constrained_ra.py:440-493) of the pending service of every QoSConstrainedRA
// env (include/orl.h, orl_batch_matrix_paths_observation); included by orl_api.hip behind orl_view.h.
//
// Per env a row of dim = E * S * (k + 1) + 1 bytes at a device pitch of round_up(dim, 16): the reference's [E, (k + 1) S] matrix
// flattened link-major, then the service class.  Every block b of S columns of link l is a prefix run of ones of length
//   len(l, 0) = S - a_l                                       (a_l: the link's counter of free units)
//   len(l, b) = min(S - a_l + 1, S)   if l lies on allowed path b - 1                               (1 <= b <= k)
//             = 1                     else if b >= 2, l lies on allowed path b - 2 and a_l = 0
//             = 0                     otherwise.
// Path p is allowed iff p < n_paths[src, dst] and (class != 0 or p == 0): class-0 services only take the shortest path (the
// `break` of the reference).  The "1" restates the reference's slice [start, start + S - a + 1): at a = 0 it runs one column
// into the next path's block, and is clipped at the end of the row, never carried into the next link's row.
//
// Layout of the work: one wavefront per env, ORL_QOBS_WAVES per workgroup.  Phase 1 leaves the env's E (k + 1) run lengths in
// LDS as u16, in row order: "segment" g = l (k + 1) + b covers columns [g S, (g + 1) S).  Phase 2: lane c writes the 16-byte
// chunks c, c + 64, ... of the row; a chunk starts in segment g at offset o (one division per lane, then stepped by 1 024
// columns without dividing) and walks its segments, each adding a run of ones to a 16-bit field expanded to bytes in
// registers (view_bits16_bytes of orl_view.h, shared with the action masks; the phase-2 walk, the class byte and the guard against a
// pair outside the topology are this view's own).  Only 16-byte stores, no atomics, no host synchronisation: graph-capturable.
#pragma once

#define ORL_QOBS_WAVES 4  // wavefronts (envs) per workgroup

// LDS bytes of one wavefront: E (k + 1) u16 run lengths, padded to 16 bytes
__host__ __device__ inline int qos_obs_wave_lds(int E, int K) { return (E * (K + 1) * 2 + 15) / 16 * 16; }

#ifndef ORL_W  // (the kernel: the API unit; the per-W units, orl_kernels.hip, take the size above for their view_plan)
__global__ void __launch_bounds__(256) k_qos_matrix_obs(DevParams P, unsigned char* out, int pitch) {
  const int lane = lane_id();
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const i64 env = (i64)blockIdx.x * ORL_QOBS_WAVES + wv;
  if (env >= P.B) return;
  const int N = P.N, E = P.E, K = P.K, S = P.S, K1 = K + 1, nseg = E * K1;
  unsigned short* len = (unsigned short*)(orl_lds_api + (size_t)wv * qos_obs_wave_lds(E, K));
  const u64* rec = P.scal + env * ORL_SCAL_WORDS;
  const u64 sd = rec[SC_SRC_DST];
  const int src = (int)(u32)sd, dst = (int)(sd >> 32), cls = (int)(rec[SC_BR_IDX] >> 32);  // class = the bit-rate index
  const bool pair_ok = (unsigned)src < (unsigned)N && (unsigned)dst < (unsigned)N;
  const int np = pair_ok ? P.n_paths[src * N + dst] : 0;
  const int n_allowed = cls == 0 ? (np < 1 ? np : 1) : np;
  const u64* cnt = P.bitmap + env * P.bm_words;  // QoSConstrainedRA: one counter of free units per link

  // ---- phase 1: run lengths.  Block 0 of every link, the path blocks 0 ...
  for (int l = lane; l < E; l += 64) {
    len[l * K1] = (unsigned short)(S - (int)(i64)cnt[l]);
    for (int b = 1; b < K1; b++) len[l * K1 + b] = 0;
  }
  wave_fence();
  // ... then the allowed paths in order, lane = hop (the links of a path are distinct): path p sets block p + 1 of its links
  // and, on a link without a free unit, the spill column of block p + 2.  A later path only writes blocks >= p + 2, with a
  // length >= 1: the order leaves every block at its len().
  const int pb = (src * N + dst) * K;
  for (int p = 0; p < n_allowed; p++) {
    const PathRec pr = path_rec_load(P, pb + p);
    const int hops = path_rec_byte(pr, 0);
    if (lane < hops) {
      const int l = path_rec_byte(pr, 2 + lane);
      if (l < E) {
        const int a = (int)(i64)cnt[l];
        len[l * K1 + p + 1] = (unsigned short)(a > 0 ? S - a + 1 : S);
        if (a == 0 && p + 2 < K1) len[l * K1 + p + 2] = 1;
      }
    }
    wave_fence();
  }

  // ---- phase 2: the row, 16 columns per lane and store
  const int ncols = nseg * S, nch = pitch >> 4;
  const int dq = 1024 / S, dr = 1024 - dq * S;  // a lane's next chunk: 1 024 columns = dq segments + dr columns further
  int g = (16 * lane) / S, off = 16 * lane - g * S;
  unsigned char* row = out + (size_t)env * pitch;
  for (int c = lane; c < nch; c += 64) {
    const int c0 = 16 * c;
    u32 bits = 0u;
    for (int i = 0, gg = g, o = off; i < 16 && gg < nseg; gg++, o = 0) {
      const int take = S - o < 16 - i ? S - o : 16 - i;
      int ones = (int)len[gg] - o;
      ones = ones < 0 ? 0 : (ones > take ? take : ones);
      bits |= ((1u << ones) - 1u) << i;
      i += take;
    }
    uint4 v = view_bits16_bytes(bits);
    const int j = ncols - c0;  // the class column (dim - 1); the pad columns behind it stay 0
    if (j >= 0 && j < 16) {
      const u32 cb = ((u32)cls & 255u) << (8 * (j & 3));
      const int w = j >> 2;
      v.x |= w == 0 ? cb : 0u;
      v.y |= w == 1 ? cb : 0u;
      v.z |= w == 2 ? cb : 0u;
      v.w |= w == 3 ? cb : 0u;
    }
    *(uint4*)(row + c0) = v;
    off += dr;
    g += dq;
    if (off >= S) { off -= S; g++; }
  }
}
#endif
