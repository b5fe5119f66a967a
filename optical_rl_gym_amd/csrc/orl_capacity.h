// orl_capacity.h — the network capacity view: what every node pair's candidate paths can still carry (include/orl.h,
// orl_batch_network_capacity); included by orl_kernels.hip and orl_api.hip behind orl_view.h (view_bits16_bytes) and
// orl_rmcsa_complete.h (m*(p): rmcsa_best_in_reach, the one definition of RMCSA's reach rule).
//
// Every other view describes the pending service on the k paths of its own pair.  This one describes the env's whole slot map: for
// every path index pidx = (src N + dst) K + p of the topology's path tables and core c < C' (C' = C for RMCSA, else 1)
//   m(pidx, c) = the AND of the path's link rows in core c (view_path_row), L = row_longest_run(m), F = popcount(m)
// and for every class r < n_cls (RWA: one class; else the n_br rows of the bit-rate table, what br_idx indexes)
//   need(pidx, r) = 1 (RWA) | nslots_path[pidx][r] (RMSA, DeepRMSA) | n_slots[r][m*] for m* = rmcsa_best_in_reach (RMCSA; 0: beyond reach)
//   serviceable(pair, r) = some existing path p of the pair and core c have need >= 1 and L(pidx, c) >= need(pidx, r)
//   ORL_CAPACITY_PATHS        int32 [N N K C' 2]: (L, F) of row q = pidx C' + c at columns 2 q, 2 q + 1; (-1, -1) where p >= n_paths
//   ORL_CAPACITY_SERVICEABLE  bytes [N N n_cls]: column pair n_cls + r = serviceable(pair, r)
//   ORL_CAPACITY_COUNTS       int32 [n_cls + N N]: per class the pairs with paths that are not serviceable, then per pair its
//                             serviceable classes — the two marginals of the matrix
// int32 rows at a pitch of round_up(dim, 4), byte rows of round_up(dim, 16), pad 0.
//
// Layout of the work: one wavefront per env, 1 / 2 / 4 wavefronts per workgroup (capacity_plan, orl_view_plan.h).  Where they fit
// (STAGED) the wavefront copies the env's slot maps into LDS once, at a row stride of W | 1 words: every link row is read by some 60
// paths on NSFNET, and with an odd stride in 64-bit words 32 different link rows start on 32 different bank pairs, where the maps'
// own stride of 2 or 8 words would put them on 16 or 4.  The lanes stripe over the path indices of all pairs; each ANDs its path's rows
// and takes (L, F).  PATHS streams them out as 8-byte stores, over (path, core).  The other two keep min(max_c L(pidx, c), 255) per path as
// one byte in LDS, then stripe over the (pair, class) cells, 64 per round: every lane tests its cell against the pair's k paths (a path
// that does not exist has 0 there and fits nothing, so the loop is uniform), and one ballot is 64 columns of the SERVICEABLE row.
// SERVICEABLE stores them at once, 16 bytes from each of four lanes (view_bits16_bytes).  COUNTS keeps its output row in LDS: per
// round the lanes of blocked cells add 1 to their class's count (an LDS integer atomic), lane j adds the popcount of pair0 + j's bits
// of the ballot to that pair's count (one lane per pair and round; an LDS atomic as well, so that no round's add depends on how the
// compiler orders another's), and the row leaves as 16-byte stores.  Integer adds
// are order-independent: the result is deterministic.  No global atomics, no host synchronisation: graph-capturable.  Env state and
// flags are only read.
// need(pidx, r) is static per batch: k_capacity_need writes it once, on the first call of SERVICEABLE or COUNTS, as a table of one
// byte per (pair, class, path) with the k paths of a cell side by side, padded with 0 to k8 = round_up(k, 8) — RMCSA's from the one
// device definition of the reach rule.  The longest runs lie the same way, k8 bytes per pair, so that a cell is one 8-byte load of each
// per 8 paths and byte compares in registers; a first version that read one byte per (cell, path) from either spent two thirds of
// its time issuing those loads.
#pragma once

// 64-bit words from one link row to the next in the LDS copy of the slot maps
__host__ __device__ inline int capacity_row_stride(int W) { return W | 1; }
// LDS bytes of one wavefront: the slot maps, the longest runs (per pair k8 = round_up(k, 8) bytes, one per path, capped at 255: the
// needs are bytes), and for COUNTS the output row at its pitch; 16-byte multiples each
__host__ __device__ inline size_t capacity_map_bytes(int W, int cores, int E) { return ((size_t)cores * E * capacity_row_stride(W) * 8 + 15) & ~(size_t)15; }
__host__ __device__ inline int capacity_k8(int K) { return (K + 7) & ~7; }
__host__ __device__ inline size_t capacity_path_bytes(int N, int K) { return ((size_t)N * N * capacity_k8(K) + 15) & ~(size_t)15; }
// bytes of the batch's need table: [N N][n_cls][k8]
__host__ __device__ inline size_t capacity_need_bytes(int N, int K, int n_cls) { return (size_t)N * N * n_cls * capacity_k8(K); }

#ifdef ORL_W  // (the kernels: the per-W units, orl_kernels.hip; the API unit takes the sizes above for capacity_plan)
// m(pidx, c) from the slot maps `maps` (LDS or global) whose link rows are rs words apart
template <int W> __device__ __forceinline__ Row<W> capacity_row(const PathRec& r, const u64* maps, int rs, int E, int S, int core) {
  Row<W> m = row_mask_lo<W>(S);
  const int hops = path_rec_byte(r, 0);
  const u64* base = maps + (size_t)core * E * rs;
  for (int h = 0; h < hops; h++) m = row_and<W>(m, row_load<W>(base + path_rec_byte(r, 2 + h) * rs));
  return m;
}
// need[(pair n_cls + r) k8 + p] = need(pair K + p, r) for p < K, else 0: RWA 1; RMSA / DeepRMSA the path's best modulation's slots;
// RMCSA n_slots[r][m*(pidx, r)], 0 where no modulation is within reach
template <int W> __global__ void __launch_bounds__(256) k_capacity_need(DevParams P, unsigned char* need, int n_cls) {
  const int K8 = capacity_k8(P.K);
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (i64)capacity_need_bytes(P.N, P.K, n_cls)) return;
  const i64 cell = i / K8;
  const int p = (int)(i - cell * K8), pair = (int)(cell / n_cls), r = (int)(cell - (i64)pair * n_cls), pidx = pair * P.K + p;
  int n = 0;
  if (p < P.K) {
    if (P.env_type == ENV_RWA) n = 1;
    else if (P.env_type == ENV_RMCSA) {
      const unsigned char* nsl = P.nslots + r * P.M;
      const int m = rmcsa_best_in_reach(P, nsl, P.path_length[pidx], r);
      n = m >= 0 ? (int)nsl[m] : 0;
    } else n = (int)P.nslots_path[(size_t)pidx * P.n_br + r];
  }
  need[i] = (unsigned char)n;
}

// need: the batch's table [N N][n_cls][k8] (SERVICEABLE, COUNTS)
template <int W, bool STAGED>
__global__ void __launch_bounds__(256) k_network_capacity(DevParams P, void* out, const unsigned char* need, int layout, int n_cls, int pitch,
                                                          int wave_bytes) {
  const int lane = lane_id(), wv = (int)(threadIdx.x >> 6);
  const i64 env = (i64)blockIdx.x * (blockDim.x >> 6) + wv;
  if (env >= P.B) return;  // (whole wavefronts; no workgroup barrier below)
  const int N = P.N, K = P.K, S = P.S, E = P.E;
  const int C = P.env_type == ENV_RMCSA ? P.C : 1, NN = N * N, NP = NN * K;
  unsigned char* lds = orl_lds_raw + (size_t)wv * wave_bytes;
  const u64* maps = P.bitmap + env * P.bm_words;
  int rs = W;
  if (STAGED) {
    u64* lm = (u64*)lds;
    rs = capacity_row_stride(W);
    for (int i = lane; i < C * E * W; i += 64) {
      const int row = i / W;
      lm[row * rs + (i - row * W)] = maps[i];
    }
    wave_fence();
    maps = lm;
    lds += capacity_map_bytes(W, C, E);
  }
  if (layout == ORL_CAPACITY_PATHS) {
    int* row = (int*)out + env * pitch;
    const int total = NP * C;
    for (int q = lane; q < total; q += 64) {
      const int pidx = q / C, c = q - pidx * C, pair = pidx / K;
      int2 v = make_int2(-1, -1);
      if (pidx - pair * K < P.n_paths[pair]) {
        const Row<W> m = capacity_row<W>(path_rec_load(P, pidx), maps, rs, E, S, c);
        v = make_int2(row_longest_run<W>(m), row_popc<W>(m));
      }
      ((int2*)row)[q] = v;
    }
    for (int i = 2 * total + lane; i < pitch; i += 64) row[i] = 0;
    return;
  }
  // max over the cores of L per path as one byte (the needs are bytes: min(L, 255) >= need exactly where L >= need), k8 per pair; 0
  // for a path that does not exist and for the pad, which therefore fit no class
  const int K8 = capacity_k8(K), W8 = K8 >> 3;
  unsigned char* lmax = lds;
  for (int i = lane; i < NN * W8; i += 64) ((u64*)lmax)[i] = 0ull;
  wave_fence();
  int* cnt = (int*)(lds + capacity_path_bytes(N, K));  // COUNTS: the env's output row
  const bool counts = layout == ORL_CAPACITY_COUNTS;
  for (int pidx = lane; pidx < NP; pidx += 64) {
    const int pair = pidx / K;
    int L = 0;
    if (pidx - pair * K < P.n_paths[pair]) {
      const PathRec rec = path_rec_load(P, pidx);
      for (int c = 0; c < C; c++) {
        const int l = row_longest_run<W>(capacity_row<W>(rec, maps, rs, E, S, c));
        L = l > L ? l : L;
      }
    }
    lmax[pair * K8 + (pidx - pair * K)] = (unsigned char)(L < 255 ? L : 255);
  }
  if (counts)
    for (int i = lane; i < pitch; i += 64) cnt[i] = 0;
  wave_fence();
  // the (pair, class) cells, 64 per round in the order of the SERVICEABLE row: cell = pair n_cls + r; pair0 / r0: lane 0's, kept
  // without a division like every lane's own
  const int cells = NN * n_cls, dq = 64 / n_cls, dr = 64 - dq * n_cls;
  int pair = lane / n_cls, r = lane - pair * n_cls, pair0 = 0, r0 = 0;
  unsigned char* brow = (unsigned char*)out + env * pitch;
  // the lane's cell of the round in the need table (cell = pair n_cls + r is its index there), 64 cells further every round; the next
  // round's first word is requested before this round's arithmetic: where few wavefronts share a SIMD (germany50 at 8 192 envs) the
  // round is otherwise one exposed round trip each
  const u64* nd = (const u64*)need + (size_t)lane * W8;
  u64 ahead = lane < cells ? nd[0] : 0ull;
  for (int base = 0; base < cells; base += 64) {
    const bool live = base + lane < cells;
    const u64 first = ahead;
    const u64* mine = nd;
    nd += (size_t)64 * W8;
    ahead = base + 64 + lane < cells ? nd[0] : 0ull;
    bool ok = false;
    if (live) {
      const u64* lm8 = (const u64*)lmax + pair * W8;
      for (int w = 0; w < W8; w++) {
        const u64 nw = w ? mine[w] : first, lw = lm8[w];
#pragma unroll
        for (int j = 0; j < 8; j++)  // need >= 1 and L >= need: need - 1 < L unsigned
          ok = ok || (((u32)(nw >> (8 * j)) & 0xffu) - 1u < ((u32)(lw >> (8 * j)) & 0xffu));
      }
    }
    const u64 b = __ballot(ok);
    if (!counts) {
      // 16 cells per lane and 16-byte store, by the round's first four lanes (cells >= N N n_cls are 0: the pad columns)
      if (lane < 4 && base + 16 * lane < pitch) *(uint4*)(brow + base + 16 * lane) = view_bits16_bytes((u32)(b >> (16 * lane)) & 0xffffu);
    } else {
      // per class: the pairs with paths that are not serviceable (an LDS integer add per such cell: order-independent); per pair: its
      // serviceable classes, lane j adding the round's bits of pair0 + j (one lane per pair and round)
      if (live && !ok && P.n_paths[pair] > 0) atomicAdd(cnt + r, 1);
      const int pj = pair0 + lane, lo = pj * n_cls - base, hi = lo + n_cls;
      const int l0 = lo > 0 ? lo : 0, h0 = hi < 64 ? hi : 64;
      if (pj < NN && h0 > l0) {
        u64 v = b >> l0;
        if (h0 - l0 < 64) v &= (1ull << (h0 - l0)) - 1ull;
        atomicAdd(cnt + n_cls + pj, (int)__popcll(v));
      }
    }
    pair += dq; r += dr;
    if (r >= n_cls) { r -= n_cls; pair++; }
    pair0 += dq; r0 += dr;
    if (r0 >= n_cls) { r0 -= n_cls; pair0++; }
  }
  if (counts) {
    wave_fence();
    uint4* dst4 = (uint4*)((int*)out + env * pitch);
    const uint4* src4 = (const uint4*)cnt;
    for (int g = lane; g < pitch >> 2; g += 64) dst4[g] = src4[g];
  }
}
#endif
