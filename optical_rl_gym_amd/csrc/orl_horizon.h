// orl_horizon.h — the release-horizon observation: for how long each slot of the pending service's rows stays taken (include/orl.h,
// orl_batch_release_horizons); included by orl_kernels.hip and orl_api.hip behind orl_view.h (the decode of the pending service) and
// orl_blocks.h (n(r) and the block walk: block_need, block_next_run).
//
// For env e with clock now = SC_NOW and every row r of the path features' row order (r = p; RMCSA: r = p C + c), slot s:
//   H[r][s] = float32(max over the pending releases v that cover (r, s) of ev_time[v] - now), 0 where none does, -1 throughout a row
//             whose path does not exist (p >= n_paths[src, dst])
// v covers (r, s) when its path shares a link with path p of the pending pair, its core is c (RMCSA) and slot(v) <= s < slot(v) +
// max(n(v), 1).  Every pending release is later than now (the release loop has run), so every difference is a positive normal float32
// and the maximum is taken on the bit patterns as unsigned integers: rounding is monotone.
//   ORL_HORIZON_SLOTS   float32 [R S + 1]: H row-major, then float32(SC_HT), the pending service's holding time
//   ORL_HORIZON_BLOCKS  float32 [R 2 j + 1]: for block b < j of row r of orl_batch_block_table(j, modulation) the pair (H[r][start_b - 1],
//                       H[r][start_b + L_b]), +inf beyond the spectrum's edge, (-1, -1) for a block that does not exist or a row the
//                       service cannot use; then the holding time
// Rows at a pitch of round_up(dim, 4) floats, pad 0.
//
// Layout of the work: one wavefront per env, 1 / 2 / 4 wavefronts per workgroup (horizon_plan, orl_view_plan.h).  The wavefront keeps in
// LDS a table of the pending pair's paths by link (one word per link: bit p = candidate path p uses it; K <= 64, E <= 128), a window of
// H's columns and — ORL_HORIZON_BLOCKS — the env's output row.  Per round of `rows` rows: the window is set to 0 / -1, the lanes stripe
// over the env's release table up to its high-water mark (the arrays orl_batch_get_pending reads; +inf is an empty slot), OR the table's
// words of each live record's links — the candidate paths it meets — and issue one LDS atomic unsigned max per covered slot of every
// such path's row in the round, in one loop per lane over all of them (lanes are on different rows at once).  Then (wave_fence)
//   SLOTS   the window is columns [c0, c1) of the output row, c0 and c1 the round's first and end columns rounded down to 4 (the last
//           round's c1 = the pitch: the holding time and the pad ride along) — rows of H that straddle c0 or c1 are scattered into
//           both rounds' windows, so every 16-byte store is whole and each is issued by exactly one round
//   BLOCKS  the window is rows [r0, r1) whole; lane i redoes the block walk of row r0 + i (block_table_env's) and reads two words per
//           block; the output row leaves once, after the last round
// No global atomics, no host synchronisation: graph-capturable; the LDS maximum is order-independent, so the result is deterministic.
// Env state and flags are only read.
#pragma once

// a record of the release table (DevParams::ev_info): {pair_path:24 | slot:12 | n:8 | core:5 | bit_rate:15}
struct EvRec { int pidx, slot, n, core, bit_rate; };
__host__ __device__ inline EvRec ev_rec_decode(u64 v) {
  EvRec r;
  r.pidx = (int)(v & 0xffffffu);
  r.slot = (int)((v >> 24) & 0xfffu);
  r.n = (int)((v >> 36) & 0xffu);
  r.core = (int)((v >> 44) & 0x1fu);
  r.bit_rate = (int)((v >> 49) & 0x7fffu);
  return r;
}

// floats of a round's window of `rows` rows of S slots: up to 3 columns in front of them (c0 rounded down), the holding time and the pad
// behind them, rounded up to a 16-byte multiple
__host__ __device__ inline int horizon_window_floats(int rows, int S) { return (rows * S + 8 + 3) & ~3; }
// words of one env's link table: per link the set of candidate paths (bit p, K <= 64) that use it; an even number (16-byte multiple)
__host__ __device__ inline int horizon_link_words(int E) { return (E + 1) & ~1; }
// LDS bytes of one wavefront: the link table, `stage` floats of the output row (BLOCKS: its pitch; SLOTS: 0), the window
__host__ __device__ inline size_t horizon_wave_lds(int E, int S, int rows, int stage) {
  return (size_t)horizon_link_words(E) * sizeof(u64) + ((size_t)stage + horizon_window_floats(rows, S)) * sizeof(float);
}

#ifdef ORL_W  // (the kernel: the per-W units, orl_kernels.hip; the API unit takes the sizes above for horizon_plan)
// One live record of the release table into the window win = columns [c0, c0 + width) of H: the candidate paths it shares a link with are
// the OR of its links' words of the table lm (the links: bytes 2 .. of its path record; in_window keeps the paths with a row in the
// window), and every slot it holds in each such path's row takes an LDS atomic max of d, the bits of float32(release time - now)
__device__ __forceinline__ void horizon_scatter(const EvRec& v, const PathRec& rec, u32 d, const u64* lm, u64 in_window, int E, int S, int C, bool rmcsa,
                                                int c0, int width, u32* win) {
  u64 hits = 0ull, word = rec.q[0] >> 16, next1 = rec.q[1], next2 = rec.q[2], next3 = rec.q[3];
  int left = 6;
  for (int h = (int)(rec.q[0] & 0xffull); h > 0; h--) {
    const int l = (int)(word & 0xffull);
    hits |= l < E ? lm[l] : 0ull;
    word >>= 8;
    if (--left == 0) { word = next1; next1 = next2; next2 = next3; left = 8; }  // (the record's next word moves up)
  }
  hits &= in_window;
  const int n = v.n > 1 ? v.n : 1;  // (RWA: one wavelength)
  const int s0 = v.slot, s1 = v.slot + n < S ? v.slot + n : S;
  // one loop over the slots of every row hit, the rows taken off `hits` as the lane gets to them: lanes are on different rows at once
  int rel = 0, s = 0, e = 0;  // the row's first column relative to the window, the slots [s, e) of it left to do
  for (;;) {
    if (s >= e) {
      if (!hits) break;
      const int p = (int)__builtin_ctzll(hits);
      hits &= hits - 1ull;
      rel = (rmcsa ? p * C + v.core : p) * S - c0;
      s = s0 > -rel ? s0 : -rel;  // clipped to the window: 0 <= rel + s < width
      e = s1 < width - rel ? s1 : width - rel;
      continue;
    }
    atomicMax(win + (rel + s), d);
    s++;
  }
}

// The window [c0, c1) of H's columns (column r S + s) of env's rows into win: rows of missing paths -1, the others the maximum over the
// release table; by the whole wavefront, complete after the caller's wave_fence
__device__ __forceinline__ void horizon_window(const DevParams& P, i64 env, const u64* lm, int np, double now, int hwm, int c0, int c1, int lane, u32* win) {
  const int K = P.K, S = P.S;
  const bool rmcsa = P.env_type == ENV_RMCSA;
  const int C = rmcsa ? P.C : 1;
  if (c1 <= c0) return;
  const int rlo = c0 / S, rhi = (c1 - 1) / S;  // (c1 <= R S: the caller's)
  for (int r = rlo; r <= rhi; r++) {
    const u32 v = r / C < np ? 0u : __float_as_uint(-1.0f);
    for (int s = lane; s < S; s += 64) {
      const int col = r * S + s;
      if (col >= c0 && col < c1) win[col - c0] = v;
    }
  }
  wave_fence();
  // the candidate paths with a row in the window: bits plo .. phi
  const int plo = rlo / C, phi = rhi / C < K - 1 ? rhi / C : K - 1;
  const u64 in_window = (~0ull >> (63 - (phi - plo))) << plo;
  const double* et = P.ev_time + env * P.ev_cap;
  const u64* ei = P.ev_info + env * P.ev_cap;
  // Four records per lane and round trip: their times and records are loaded together, then their path records together.  The wavefront
  // has a handful of such dependent round trips in all, and they, not the arithmetic, are what it waits for.
  struct Ev { double t; u64 info; };
  const auto entry = [&](int i) { Ev v; v.t = i < hwm ? et[i] : __builtin_inf(); v.info = i < hwm ? ei[i] : 0ull; return v; };
  const auto path_of = [&](const Ev& v) { return path_rec_load(P, v.t < __builtin_inf() ? (int)(v.info & 0xffffffu) : 0); };  // (an empty slot: record 0, unused)
  const auto scatter = [&](const Ev& v, const PathRec& rec) {
    if (v.t < __builtin_inf())
      horizon_scatter(ev_rec_decode(v.info), rec, __float_as_uint((float)(v.t - now)), lm, in_window, P.E, S, C, rmcsa, c0, c1 - c0, win);
  };
  for (int i = lane; i < hwm; i += 256) {
    const Ev v0 = entry(i), v1 = entry(i + 64), v2 = entry(i + 128), v3 = entry(i + 192);
    const PathRec r0 = path_of(v0), r1 = path_of(v1), r2 = path_of(v2), r3 = path_of(v3);
    scatter(v0, r0);
    scatter(v1, r1);
    scatter(v2, r2);
    scatter(v3, r3);
  }
}

template <int W>
__global__ void __launch_bounds__(256) k_release_horizons(DevParams P, float* out, int layout, int J, int modulation, int dim, int pitch, int rows,
                                                          int wave_bytes) {
  const int lane = lane_id(), wv = (int)(threadIdx.x >> 6);
  const i64 env = (i64)blockIdx.x * (blockDim.x >> 6) + wv;
  if (env >= P.B) return;  // (whole wavefronts; no workgroup barrier below)
  const int K = P.K, S = P.S;
  const bool rwa = P.env_type == ENV_RWA, rmcsa = P.env_type == ENV_RMCSA;
  const int C = rmcsa ? P.C : 1, R = K * C;
  const bool blocks = layout == ORL_HORIZON_BLOCKS;
  unsigned char* lds = orl_lds_raw + (size_t)wv * wave_bytes;
  u64* lm = (u64*)lds;  // per link: bit p set when candidate path p of the pending pair uses it
  const int LW = horizon_link_words(P.E);
  float* stage = (float*)(lds + (size_t)LW * sizeof(u64));  // BLOCKS: the output row
  u32* win = (u32*)(stage + (blocks ? pitch : 0));
  const PendingSvc sv = view_pending(P, env);
  const int np = sv.np < K ? sv.np : K;
  const u64* rec = P.scal + env * ORL_SCAL_WORDS;
  const double now = __longlong_as_double((i64)rec[SC_NOW]);
  const float ht = (float)__longlong_as_double((i64)rec[SC_HT]);
  const int hw = (int)(u32)rec[SC_EV], hwm = hw < P.ev_cap ? hw : P.ev_cap;
  for (int l = lane; l < LW; l += 64) lm[l] = 0ull;
  wave_fence();
  for (int p = lane; p < np; p += 64) {  // (lane = path: two paths over one link meet in its word)
    const PathRec pr = path_rec_load(P, sv.pb + p);
    const int hops = path_rec_byte(pr, 0);
    for (int h = 0; h < hops; h++) {
      const int l = path_rec_byte(pr, 2 + h);
      if (l < P.E) atomicOr((unsigned long long*)lm + l, 1ull << p);
    }
  }
  float* row = out + env * pitch;
  if (blocks)
    for (int i = dim - 1 + lane; i < pitch; i += 64) stage[i] = i == dim - 1 ? ht : 0.0f;
  wave_fence();
  for (int r0 = 0; r0 < R; r0 += rows) {
    const int r1 = r0 + rows < R ? r0 + rows : R;
    if (!blocks) {
      const bool last = r1 == R;
      const int c0 = (r0 * S) & ~3, c1 = last ? pitch : (r1 * S) & ~3;
      horizon_window(P, env, lm, np, now, hwm, c0, last ? R * S : c1, lane, win);
      if (last)
        for (int i = R * S + lane; i < pitch; i += 64) win[i - c0] = i == R * S ? __float_as_uint(ht) : 0u;
      wave_fence();
      uint4* dst4 = (uint4*)(row + c0);
      const uint4* src4 = (const uint4*)win;
      for (int g = lane; g < (c1 - c0) >> 2; g += 64) dst4[g] = src4[g];
    } else {
      horizon_window(P, env, lm, np, now, hwm, r0 * S, r1 * S, lane, win);
      wave_fence();
      for (int r = r0 + lane; r < r1; r += 64) {
        const int p = r / C, core = r - p * C;
        float2* o = (float2*)(stage + r * 2 * J);
        const float* h = (const float*)win + (r - r0) * S;
        int mod, n = 0, nb = 0;
        if (p < np) n = block_need(P, sv, p, modulation, rwa, rmcsa, mod);
        if (n > 0) {
          const Row<W> m = view_path_row<W>(P, sv.bm, sv.pb + p, core);
          Row<W> f = row_runs_ge<W>(m, n);
          const Row<W> zeros = row_andn<W>(row_mask_lo<W>(S), m);
          int st, end;
          while (nb < J && block_next_run<W>(f, zeros, S, st, end))
            o[nb++] = make_float2(st > 0 ? h[st - 1] : __builtin_inff(), end < S ? h[end] : __builtin_inff());
        }
        for (int b = nb; b < J; b++) o[b] = make_float2(-1.0f, -1.0f);
      }
    }
    wave_fence();  // (the next round overwrites the window)
  }
  if (blocks) {
    uint4* dst4 = (uint4*)row;
    const uint4* src4 = (const uint4*)stage;
    for (int g = lane; g < pitch >> 2; g += 64) dst4[g] = src4[g];
  }
}
#endif
