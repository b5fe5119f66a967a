// orl_assign.h — spectrum-assignment rules for RMSA and RWA actions (include/orl.h, orl_batch_assign_spectrum); included by
// orl_kernels.hip behind orl_view.h (the kernel's opening and the decode of the pending service are shared with the other views).
//
// The agent gives nothing or a path; the kernel picks the first slot (RWA: the wavelength) s* out of
//   fits(p) = { s : s + n <= S, slots s .. s + n - 1 free on every hop of p }      (row_runs_ge of the path's AND-row m(p))
// under the launch's rule and writes the env's row of ORL_BUF_ACTIONS as (p, s*, 0, 0); no completion — a given path out of range,
// no path with a fit — is (K, S).  n_given = 0: the first path in order with a non-empty fits(p), then the rule on that path.
//   FIRST_FIT / LAST_FIT    the lowest / highest bit of fits(p)
//   BEST_FIT / EXACT_FIT    a maximal free run of m(p) of length L >= n is a maximal run of fits(p) of length L - n + 1 with the same
//                           start (a run of fits(p) never ends at a word's edge unless the run of m(p) goes on, so word edges need no
//                           case of their own): the set bits of row_starts(m) & fits = row_starts(fits) are the runs, and a run's
//                           last bit is the lowest "last bit of a run" at or above its start.  The winner's fits row goes to the
//                           group's lanes, lane w measures the runs that start in word w, and a g8_min over (L - n, start) keeps
//                           the shortest run (ties: the first); EXACT_FIT takes it when L == n and is FIRST_FIT else.
//   MOST_USED / LEAST_USED  u[w] = links of the env's whole slot map (all E) with slot w occupied; U(s) = u[s] + .. + u[s + n - 1];
//                           the s of fits(p) with the largest / smallest U(s), ties to the lowest s.
//
// Layout of the work: 8 lanes per env, 8 envs per wavefront, 4 wavefronts per workgroup; one candidate path per lane, in chunks of 8
// for k > 8; a ballot over the group picks the first path that fits and the group leaves the walk there.  Rules 0 and 1 are then the
// winning lane's alone, rules 2 and 3 the group's (above).  The counts of rules 4 and 5 (CNT: a second instantiation, so the other
// rules pay neither its registers nor its LDS) are shared by the group: lane w < W owns word w of the row — 64 slots — and runs over all E link rows, 8 bytes per
// lane and link, 64 contiguous bytes per group.  Its 64 counts are bit-sliced: 8 planes of 64 bits (E <= 128 < 256), plane j = bit
// j of the 64 counts, 16 VGPRs; four links go in at once through three carry-save adders (ones, twos -> one row of weight 4 that
// ripples through planes 2 .. 7), the last E mod 4 ripple in from plane 0: ~8 64-bit operations per link and word where a per-slot
// counter takes 64.  Byte counters in LDS from the start would cost one read-modify-write per occupied slot and link; the planes
// stay in registers until the one moment integers are needed: the lane expands them to 64 byte counters in LDS (4 slots per
// 32-bit store: a nibble of each plane spread to 4 bytes, view_nibble_bytes), the winner's fits row goes word by word to the
// lanes, and lane w slides the window sum over the set bits of its word — U(s + 1) = U(s) - u[s] + u[s + n] — so the 8 lanes scan
// 64 start slots each; the group's best (U, s) is a g8_max over one packed key.  LDS: per env W words of 64 + 4 bytes (17 dwords:
// the 8 lanes of a group start on 8 different banks) padded to = 8 (mod 32) dwords (the 4 envs of a 32-lane half then cover all 32
// banks): 136 dwords per env at W = 8, 17 KiB per workgroup, within view_waves()' 48 KiB at 4 wavefronts for every W.
// Lane 0 of the group stores the row as 16 bytes.  No atomics, no host synchronisation: graph-capturable.
// `given`: the path of env e at given[e * gstride] — the actions buffer itself with gstride 4 (every lane of the group has it in a
// register before lane 0 stores the row: the store's value depends on that load), or the batch's upload buffer (gstride 1).
#pragma once

// dwords of LDS one env's byte counters take (CNT): W words of 17 dwords, padded to 8 (mod 32)
__host__ __device__ inline int assign_env_dwords(int W) { return 17 * W + ((8 - 17 * W) & 31); }

#ifdef ORL_W  // (the kernel: the per-W units, orl_kernels.hip; the API unit takes the size above for its view_plan)
// BEST_FIT / EXACT_FIT on r = fits(p), by the group's lane gl: over the maximal runs of r that start in word gl (none for gl >= W)
// the smallest key (l << 10) | start, the run having l + 1 bits — a free run of n + l slots.  The run's last bit is the lowest
// "last bit of a run" at or above its start: in word gl, or the lowest one of the words above.  0x7fffffff: no run starts there
template <int W> __device__ __forceinline__ int assign_runs_key(const Row<W>& r, int gl) {
  const Row<W> st = row_starts<W>(r);                        // = row_starts(m) & fits
  const Row<W> en = row_andn<W>(r, row_shr_small<W>(r, 1));  // the last bit of every run
  u64 sw = 0ull, ew = 0ull;
  int later = 64 * W;
#pragma unroll
  for (int i = W - 1; i >= 0; i--) {
    if (i == gl) { sw = st.w[i]; ew = en.w[i]; }
    if (i > gl && en.w[i]) later = 64 * i + (int)__builtin_ctzll(en.w[i]);
  }
  int key = 0x7fffffff;
  while (sw) {
    const int b = (int)__builtin_ctzll(sw);
    sw &= sw - 1ull;
    const u64 x = ew & (~0ull << b);
    const int s = 64 * gl + b, e = x ? 64 * gl + (int)__builtin_ctzll(x) : later;
    const int k = ((e - s) << 10) | s;
    key = k < key ? k : key;
  }
  return key;
}

// a + b + c of three rows of equal weight: the sum row and the carry row (weight 2)
__device__ __forceinline__ void assign_csa(u64 a, u64 b, u64 c, u64& sum, u64& carry) {
  const u64 t = a ^ b;
  sum = t ^ c;
  carry = (a & b) | (t & c);
}
// the planes (bit j of 64 counts) + x of weight 2^FROM
template <int FROM> __device__ __forceinline__ void assign_ripple(u64 (&pl)[8], u64 x) {
#pragma unroll
  for (int j = FROM; j < 8; j++) {
    const u64 t = pl[j] & x;
    pl[j] ^= x;
    x = t;
  }
}

template <int W, bool CNT>
__global__ void __launch_bounds__(256) k_assign_spectrum(DevParams P, int rule, int n_given, const int* given, int gstride) {
  const ViewLanes v = view_lanes();
  if (v.env >= P.B) return;  // (whole groups: the ballot and the exchanges below stay within a group)
  const int lane = v.lane, gl = v.gl;
  const int K = P.K, S = P.S, E = P.E;
  const bool rwa = P.env_type == ENV_RWA;
  const PendingSvc sv = view_pending(P, v.env);
  const int np = sv.np, pb = sv.pb;
  const int gp = n_given >= 1 ? given[v.env * gstride] : 0;
  // the candidate paths [p0, p0 + total); a given path out of range: none
  const int p0 = n_given >= 1 ? gp : 0;
  const int total = n_given >= 1 ? ((gp >= 0 && gp < np) ? 1 : 0) : np;
  int best = -1, slot = 0;
  for (int base = 0; base < total && best < 0; base += 8) {
    const int q = base + gl;
    Row<W> r = row_mask_lo<W>(0);
    int n = 1;
    if (q < total) {
      const int pidx = pb + p0 + q;
      if (!rwa) n = (int)P.nslots_path[(size_t)pidx * P.n_br + sv.br_idx];
      // bit s: s .. s + n - 1 free on every hop (bits >= S of the AND-row are 0, so s + n <= S)
      r = row_runs_ge<W>(path_and_rec<W>(path_rec_load(P, pidx), sv.bm, E, S, 0), n);
    }
    const u32 fit = g8::gballot(row_any<W>(r), lane);
    if (!fit) continue;
    const int l = (int)__builtin_ctz(fit);
    best = base + l;
    if constexpr (!CNT) {
      if (rule == ORL_ASSIGN_FIRST_FIT || rule == ORL_ASSIGN_LAST_FIT) {
        slot = g8::gget(rule == ORL_ASSIGN_FIRST_FIT ? row_ctz<W>(r) : row_bitlen<W>(r) - 1, l, lane);
      } else {
        // the winner's row to every lane of the group; lane w takes the runs that start in word w
        Row<W> wr;
#pragma unroll
        for (int i = 0; i < W; i++) wr.w[i] = g8::gget(r.w[i], l, lane);
        const int key = g8_min(assign_runs_key<W>(wr, gl));  // the shortest run, the lowest start among equals
        // EXACT_FIT: the first run of exactly n slots (l == 0), else first fit
        slot = (rule == ORL_ASSIGN_EXACT_FIT && (key >> 10) != 0) ? row_ctz<W>(wr) : (key & 1023);
      }
    } else {
      // u[w] of this lane's 64 slots, bit-sliced
      u64 pl[8];
#pragma unroll
      for (int j = 0; j < 8; j++) pl[j] = 0ull;
      if (gl < W) {
        const u64* col = sv.bm + gl;
        int e = 0;
        for (; e + 4 <= E; e += 4) {
          const u64 a = ~col[(size_t)e * W], b = ~col[(size_t)(e + 1) * W], c = ~col[(size_t)(e + 2) * W], d = ~col[(size_t)(e + 3) * W];
          u64 s1, c1, c2, c3;
          assign_csa(pl[0], a, b, s1, c1);
          assign_csa(s1, c, d, pl[0], c2);
          assign_csa(pl[1], c1, c2, pl[1], c3);
          assign_ripple<2>(pl, c3);
        }
        for (; e < E; e++) assign_ripple<0>(pl, ~col[(size_t)e * W]);
      }
      // ... as 64 byte counters in LDS, 4 per store
      u32* mine = (u32*)orl_lds_raw + ((size_t)v.wv * 8 + (lane >> 3)) * assign_env_dwords(W);
      if (gl < W) {
        u32* o = mine + 17 * gl;
        for (int qd = 0; qd < 16; qd++) {
          u32 acc = 0u;
#pragma unroll
          for (int j = 0; j < 8; j++) acc += view_nibble_bytes((u32)(pl[j] >> (4 * qd)) & 15u) << j;
          o[qd] = acc;
        }
      }
      wave_fence();
      // word gl of the winner's fits row and its n
      u64 fw = 0ull;
#pragma unroll
      for (int i = 0; i < W; i++) {
        const u64 x = g8::gget(r.w[i], l, lane);
        if (i == gl) fw = x;
      }
      n = g8::gget(n, l, lane);
      const unsigned char* u = (const unsigned char*)mine;  // slot w at byte (w >> 6) * 68 + (w & 63)
      int key = -1;
      if (fw) {
        const int lo = 64 * gl + (int)__builtin_ctzll(fw), hi = 64 * gl + 63 - (int)__builtin_clzll(fw);
        int U = 0;
        for (int w = lo; w < lo + n; w++) U += (int)u[(w >> 6) * 68 + (w & 63)];
        for (int s = lo;; s++) {
          if ((fw >> (s & 63)) & 1ull) {
            // U <= 64 * 128 < 2^14, s < 2^10: the largest key = the best U, then the lowest s
            const int k = ((rule == ORL_ASSIGN_MOST_USED ? U : 16383 - U) << 10) | (1023 - s);
            key = k > key ? k : key;
          }
          if (s == hi) break;
          U += (int)u[((s + n) >> 6) * 68 + ((s + n) & 63)] - (int)u[(s >> 6) * 68 + (s & 63)];  // (s + n <= hi + n - 1 < S)
        }
      }
      key = g8_max(key);
      slot = 1023 - (key & 1023);
    }
  }
  if (gl == 0) {
    int4 a = make_int4(K, S, 0, 0);
    if (best >= 0) a = make_int4(p0 + best, slot, 0, 0);
    *(int4*)(P.actions + v.env * 4) = a;
  }
}
#endif
