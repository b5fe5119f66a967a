// orl_capacity_after.h — what each candidate placement of the pending service leaves the network (include/orl.h,
// orl_batch_capacity_after); included by orl_kernels.hip and orl_api.hip behind orl_capacity.h (capacity_row, the k8-byte layout of
// longest runs and needs, k_capacity_need's table) and orl_view.h (view_pending).
//
// For an env with slot maps A and a candidate (row, s, n) — row = p C' + c in the path features' row order, p a path of the PENDING
// service's pair, c a core, [s, s + n) a window of slots — A - cand is A with the window taken on every link of p in core c, and
//   after(q)[r] = the ordered pairs with paths for which class r is NOT serviceable on A - cand_q
//               = the first n_cls columns of ORL_CAPACITY_COUNTS evaluated on A - cand_q
// A candidate is present iff 0 <= row < k C', p < n_paths[pair], n >= 1, 0 <= s and s + n <= S; an absent one has -1 throughout.  Row Q,
// one past the last candidate, is the baseline on A itself.
//   ORL_AFTER_CLASSES  int32 [(Q + 1) n_cls]: row q = after(q)
//   ORL_AFTER_TOTAL    int32 [Q + 1]: the sum of row q over the classes, -1 for an absent candidate
// at a pitch of round_up(dim, 4), pad 0.  The candidates come from one of three tables, all through after_decode:
//   ORL_AFTER_ROUTE   the (s*, c*, n, free) rows of orl_batch_route_spectrum / orl_batch_route_cores: candidate q = (q, col 0, col 2)
//   ORL_AFTER_BLOCKS  the block table of one j: candidate q = r j + b = block b of row r, n = col 0 of the row, s the block's lower
//                     (ORL_BLOCK_FIRST) or upper end (ORL_BLOCK_LAST); a block with start >= S does not exist
//   ORL_AFTER_GIVEN   [Q][3] rows (row, s, n) from the host
// Whatever a table holds is validated by the presence rule alone.
//
// Layout of the work: as k_network_capacity — one wavefront per env, no workgroup barrier, the maps staged in LDS at a stride of
// W | 1 words where capacity_after_plan says so, else read from global memory by the same code.  The wavefront first runs the COUNTS
// pass: per path min(max over the cores of L, 255) as one byte, k8 per pair (`lbase`), and the baseline class counts.  A candidate
// then costs only what it changes.  Taking the window out of core c of path p changes the AND-row of exactly the paths that share a
// link with p, and only in core c: the candidate's link set is two 64-bit words (E <= 128), every lane walking its share of the
// path tables tests its paths' links against it, and only sharing paths recompute.  RMCSA: a sharing path recomputes its C rows
// and takes the window out of core c's — per-(path, core) bytes would multiply the largest LDS term by C (31 cores: past the limit on
// NSFNET already), while the rows of a sharing path are a fraction of the pass.  The lanes stripe over the PAIRS, 64 per round: a lane
// walks its pair's k paths and assembles the pair's new k8 words — the old byte of a path that shares no link, the recomputed one of a
// path that does — in a scratch of its own (k8 bytes per lane; a second whole copy of the longest runs would put star65's 2 x 33 808
// bytes past the limit).  One ballot names the round's pairs with a word that differs from the baseline's; for each of them in turn
// the lanes stripe over the pair's classes, test the cell old against new — one 8-byte load of the need table per lane and 8 paths,
// side by side in memory — and add 1 to the class's count of the candidate's row for every cell that was serviceable and no longer is
// (an LDS integer atomic: order-independent).  A first version in which the pair's own lane walked its classes one after the other
// cost as much as a recount.  The baseline bytes are never written, so nothing is restored.  The row starts as the baseline's.  It leaves
// as 16-byte stores where n_cls is a multiple of 4, else one int32 per lane; TOTAL keeps its Q + 1 sums in LDS and streams them out
// at the end.  No global atomics, no host synchronisation: graph-capturable.  Env state, flags and the tables are only read.
#pragma once

#define ORL_AFTER_MAX_CANDIDATES 1024  // (= include/orl.h's ORL_AFTER_MAX_Q: the API unit checks the two against each other)

// LDS bytes of one wavefront beside the maps: the baseline's longest runs, every lane's scratch of k8 bytes for its pair's new ones,
// the class counts twice (baseline and the candidate's row) and, for TOTAL, the output row of Q + 1 sums; 16-byte multiples each
__host__ __device__ inline size_t capacity_after_cls_bytes(int n_cls) { return ((size_t)n_cls * 4 + 15) & ~(size_t)15; }
__host__ __device__ inline size_t capacity_after_total_bytes(int Q) { return ((size_t)(Q + 1) * 4 + 15) & ~(size_t)15; }
__host__ __device__ inline size_t capacity_after_fixed_bytes(int N, int K, int n_cls, int Q, bool total) {
  return capacity_path_bytes(N, K) + (size_t)64 * capacity_k8(K) + 2 * capacity_after_cls_bytes(n_cls) + (total ? capacity_after_total_bytes(Q) : 0);
}

#ifdef ORL_W  // (the kernels: the per-W units, orl_kernels.hip)
// candidate q of the env's table `tab` (its row of the route / core table, of the block table of J blocks, or its [Q][3] given rows);
// n = 0: none
struct AfterCand { int row, s, n; };
__device__ __forceinline__ AfterCand after_decode(const int* tab, int source, int J, int placement, int S, int q) {
  AfterCand c = {0, 0, 0};
  if (source == ORL_AFTER_ROUTE) {
    const int4 t = *(const int4*)(tab + 4 * q);  // (s*, c*, n, free)
    c.row = q; c.s = t.x; c.n = t.x >= S ? 0 : t.z;
  } else if (source == ORL_AFTER_BLOCKS) {
    const int r = q / J, b = q - r * J;
    const int* row = tab + r * (2 + 2 * J);
    const int2 blk = *(const int2*)(row + 2 + 2 * b);  // (start, length)
    c.row = r; c.n = blk.x >= S ? 0 : row[0];
    c.s = placement == ORL_BLOCK_LAST ? blk.x + blk.y - c.n : blk.x;
  } else {
    c.row = tab[3 * q]; c.s = tab[3 * q + 1]; c.n = tab[3 * q + 2];
  }
  return c;
}
// need >= 1 and L >= need for some of the 8 paths of a word pair (need - 1 < L unsigned)
__device__ __forceinline__ bool after_fits8(u64 nw, u64 lw) {
  bool ok = false;
#pragma unroll
  for (int j = 0; j < 8; j++) ok = ok || (((u32)(nw >> (8 * j)) & 0xffu) - 1u < ((u32)(lw >> (8 * j)) & 0xffu));
  return ok;
}

// tab: the candidates' table, tstride int32 per env; need: the batch's table [N N][n_cls][k8]
template <int W, bool STAGED>
__global__ void __launch_bounds__(256) k_capacity_after(DevParams P, int* out, const unsigned char* need, const int* tab, int tstride, int source, int J,
                                                        int placement, int Q, int layout, int n_cls, int pitch, int wave_bytes) {
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
  const int K8 = capacity_k8(K), W8 = K8 >> 3;
  const bool total = layout == ORL_AFTER_TOTAL;
  unsigned char* lbase = lds;
  u64* mine = (u64*)(lbase + capacity_path_bytes(N, K)) + (size_t)lane * W8;  // this lane's scratch
  int* cbase = (int*)(lbase + capacity_path_bytes(N, K) + (size_t)64 * K8);
  int* acc = (int*)((unsigned char*)cbase + capacity_after_cls_bytes(n_cls));
  int* tot = (int*)((unsigned char*)acc + capacity_after_cls_bytes(n_cls));
  const int ncls4 = (int)(capacity_after_cls_bytes(n_cls) >> 2);
  // the COUNTS pass: the baseline bytes (0 for a path that does not exist and for the pad) ...
  for (int i = lane; i < NN * W8; i += 64) ((u64*)lbase)[i] = 0ull;
  for (int i = lane; i < ncls4; i += 64) cbase[i] = 0;
  wave_fence();
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
    lbase[pair * K8 + (pidx - pair * K)] = (unsigned char)(L < 255 ? L : 255);
  }
  wave_fence();
  // ... and the baseline class counts, a lane per (pair, class) cell
  const int cells = NN * n_cls;
  for (int cell = lane; cell < cells; cell += 64) {
    const int pair = cell / n_cls;
    if (P.n_paths[pair] <= 0) continue;
    const u64* nd = (const u64*)need + (size_t)cell * W8;
    const u64* l8 = (const u64*)lbase + pair * W8;
    bool ok = false;
    for (int w = 0; w < W8; w++) ok = ok || after_fits8(nd[w], l8[w]);
    if (!ok) atomicAdd(cbase + (cell - pair * n_cls), 1);
  }
  wave_fence();

  const PendingSvc sv = view_pending(P, env);
  const int R = K * C;
  const int* mytab = tab + env * (i64)tstride;
  int* orow = out + env * pitch;
  for (int q = 0; q <= Q; q++) {
    bool present = true;
    int p = 0, core = 0;
    AfterCand cd = {0, 0, 0};
    if (q < Q) {
      cd = after_decode(mytab, source, J, placement, S, q);
      present = cd.row >= 0 && cd.row < R && cd.n >= 1 && cd.n <= S && cd.s >= 0 && cd.s <= S - cd.n;
      if (present) {
        p = cd.row / C; core = cd.row - p * C;
        present = p < sv.np;
      }
    }
    if (!present) {
      if (total) { if (lane == 0) tot[q] = -1; }
      else for (int i = lane; i < n_cls; i += 64) orow[q * n_cls + i] = -1;
      continue;
    }
    for (int i = lane; i < ncls4; i += 64) acc[i] = cbase[i];
    wave_fence();
    if (q < Q) {
      // the candidate's link set
      const PathRec crec = path_rec_load(P, sv.pb + p);
      const int chops = path_rec_byte(crec, 0);
      u64 m0 = 0ull, m1 = 0ull;
      for (int h = 0; h < chops; h++) {
        const int l = path_rec_byte(crec, 2 + h);
        if (l < 64) m0 |= 1ull << l; else m1 |= 1ull << (l - 64);
      }
      // a lane per pair, 64 pairs per round: the pair's new k8 words into the lane's scratch; then, pair by pair of those with a changed
      // word, the lanes over the pair's classes: the cell old against new
      const u64* scratch = (const u64*)(lbase + capacity_path_bytes(N, K));
      for (int pair0 = 0; pair0 < NN; pair0 += 64) {
        const int pair = pair0 + lane;
        bool changed = false;
        if (pair < NN) {
          const int np = P.n_paths[pair] < K ? P.n_paths[pair] : K;
          const u64* lb8 = (const u64*)lbase + pair * W8;
          for (int w = 0; w < W8; w++) {
            const u64 ow = lb8[w];
            u64 nw = ow;
            for (int j = 0; j < 8 && 8 * w + j < np; j++) {
              const PathRec rec = path_rec_load(P, pair * K + 8 * w + j);
              const int hops = path_rec_byte(rec, 0);
              bool shares = false;
              for (int h = 0; h < hops; h++) {
                const int l = path_rec_byte(rec, 2 + h);
                shares = shares || (((l < 64 ? m0 >> l : m1 >> (l - 64)) & 1ull) != 0ull);
              }
              if (!shares) continue;
              int L = 0;
              for (int c = 0; c < C; c++) {
                Row<W> m = capacity_row<W>(rec, maps, rs, E, S, c);
                if (c == core) m = row_andn<W>(m, row_range<W>(cd.s, cd.n));
                const int l = row_longest_run<W>(m);
                L = l > L ? l : L;
              }
              nw = (nw & ~(0xffull << (8 * j))) | ((u64)(L < 255 ? L : 255) << (8 * j));
            }
            mine[w] = nw;
            changed = changed || nw != ow;
          }
        }
        u64 ch = __ballot(changed);
        wave_fence();
        while (ch) {
          const int l = __builtin_ctzll(ch);
          ch &= ch - 1ull;
          const int cp = pair0 + l;
          const u64* lb8 = (const u64*)lbase + cp * W8;
          const u64* lc8 = scratch + l * W8;
          for (int r = lane; r < n_cls; r += 64) {
            const u64* nd = (const u64*)need + ((size_t)cp * n_cls + r) * W8;
            bool was = false, is = false;
            for (int w = 0; w < W8; w++) {
              const u64 nw = nd[w];
              was = was || after_fits8(nw, lb8[w]);
              is = is || after_fits8(nw, lc8[w]);
            }
            if (was && !is) atomicAdd(acc + r, 1);
          }
        }
        wave_fence();  // (the scratch is read before the next round rewrites it)
      }
    }
    if (total) {
      int s = 0;
      for (int i = lane; i < n_cls; i += 64) s += acc[i];
      s = wave_sum(s);
      if (lane == 0) tot[q] = s;
    } else if ((n_cls & 3) == 0) {
      uint4* dst4 = (uint4*)(orow + q * n_cls);
      for (int g = lane; g < n_cls >> 2; g += 64) dst4[g] = ((const uint4*)acc)[g];
    } else {
      for (int i = lane; i < n_cls; i += 64) orow[q * n_cls + i] = acc[i];
    }
    wave_fence();  // (the row is read before the next candidate resets it)
  }
  if (total) {
    for (int i = Q + 1 + lane; i < pitch; i += 64) tot[i] = 0;
    wave_fence();
    uint4* dst4 = (uint4*)orow;
    for (int g = lane; g < pitch >> 2; g += 64) dst4[g] = ((const uint4*)tot)[g];
  } else {
    for (int i = (Q + 1) * n_cls + lane; i < pitch; i += 64) orow[i] = 0;
  }
}
#endif
