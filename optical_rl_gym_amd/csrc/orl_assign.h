// orl_assign.h — spectrum-assignment rules for RMSA and RWA actions (include/orl.h, orl_batch_assign_spectrum), and what the rules
// are made of, which orl_route.h shares: the packed keys, the layout of the occupancy counts u[], the best / exact fit decision.
// Included by orl_kernels.hip behind orl_view.h (the kernel's opening and the decode of the pending service are shared with the other
// views).
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
//                           group's lanes, lane w measures the runs that start in word w (assign_runs_key), and a g8_min over
//                           (L - n, start) keeps the shortest run (ties: the first); assign_run_choice makes the slot of it.
//   MOST_USED / LEAST_USED  u[w] = links of the env's whole slot map (all E) with slot w occupied; U(s) = u[s] + .. + u[s + n - 1];
//                           the s of fits(p) with the largest / smallest U(s), ties to the lowest s: the group's counts in
//                           LDS, the winner's fits row word by word to the lanes, lane w sliding the window sum over the set
//                           bits of its word — U(s + 1) = U(s) - u[s] + u[s + n], the 8 lanes scan 64 start slots each — and
//                           a g8_max over (U, s).  Lane w < W counts its 64 slots over all E link rows in bit-sliced planes,
//                           four links at once through three carry-save adders, and expands the planes to byte counters only
//                           then.  This path is written out in the kernel below and again in orl_route.h
//                           (route_counts and its window loop): one shared form of it measured slower at W = 2.
//
// Layout of the work: 8 lanes per env, 8 envs per wavefront, 4 wavefronts per workgroup; one candidate path per lane, in chunks of 8
// for k > 8; a ballot over the group picks the first path that fits and the group leaves the walk there.  Rules 0 and 1 are then the
// winning lane's alone, the others the group's.  Rules 4 and 5 are a second instantiation (CNT), so the other rules pay neither the
// counts' registers nor their LDS.  Lane 0 of the group stores the row as 16 bytes.  No atomics, no host synchronisation:
// graph-capturable.
// `given`: the path of env e at given[e * gstride] — the actions buffer itself with gstride 4 (every lane of the group has it in a
// register before lane 0 stores the row: the store's value depends on that load), or the batch's upload buffer (gstride 1).
#pragma once

// LDS of the counts: per env W words of 64 byte counters + 4 bytes (17 dwords: the 8 lanes of a group start on 8 different banks),
// padded to = 8 (mod 32) dwords (the 4 envs of a 32-lane half then cover all 32 banks): 136 dwords per env at W = 8, 17 KiB per
// workgroup, within view_waves()' 48 KiB at 4 wavefronts for every W
enum { ASSIGN_WORD_DWORDS = 17 };
__host__ __device__ inline int assign_env_dwords(int W) { return ASSIGN_WORD_DWORDS * W + ((8 - ASSIGN_WORD_DWORDS * W) & 31); }
// the rules that need the counts, and their LDS
__host__ __device__ inline bool assign_rule_counted(int rule) { return rule == ORL_ASSIGN_MOST_USED || rule == ORL_ASSIGN_LEAST_USED; }

#ifdef ORL_W  // (the kernels: the per-W units, orl_kernels.hip; the API unit takes the two above for its view_plan)
// ---- packed keys: one int per candidate, reduced over the group with g8_min / g8_max; the fields against the accepted range -------
enum {
  KEY_SLOT_BITS = 10, KEY_SLOT_MAX = (1 << KEY_SLOT_BITS) - 1,  // a slot s, or KEY_SLOT_MAX - s where the lowest s wins a maximum
  KEY_SUM_BITS = 14, KEY_SUM_MAX = (1 << KEY_SUM_BITS) - 1,     // a window sum U(s) of n counts, or its complement
  KEY_NO_RUN = 0x7fffffff,                                      // the run key of "no run"
  COUNT_PLANES = 8,                                             // bit-sliced u[w]: plane j = bit j of 64 counts
};
static_assert(ORL_MAX_SLOTS <= KEY_SLOT_MAX, "a slot does not fit the keys' slot field");
static_assert(ORL_MAX_NEED * ORL_MAX_LINKS <= KEY_SUM_MAX, "U(s) <= n E does not fit the (U, s) key's sum field");
static_assert(((long long)ORL_MAX_SLOTS << KEY_SLOT_BITS | KEY_SLOT_MAX) < KEY_NO_RUN, "a run key reaches KEY_NO_RUN");
static_assert(ORL_MAX_LINKS < (1 << COUNT_PLANES), "u[w] <= E does not fit the count planes");

// (L - n, start) of a maximal free run of L slots: the smallest key = the shortest run, then the lowest start
__device__ __forceinline__ int key_run(int over, int start) { return (over << KEY_SLOT_BITS) | start; }
__device__ __forceinline__ int key_run_over(int key) { return key >> KEY_SLOT_BITS; }
__device__ __forceinline__ int key_run_start(int key) { return key & KEY_SLOT_MAX; }
// (U(s), s) under MOST_USED / LEAST_USED: the largest key = the largest / smallest U, then the lowest s
__device__ __forceinline__ int key_sum(int rule, int U, int s) {
  return ((rule == ORL_ASSIGN_MOST_USED ? U : KEY_SUM_MAX - U) << KEY_SLOT_BITS) | (KEY_SLOT_MAX - s);
}
__device__ __forceinline__ int key_sum_U(int rule, int key) { return rule == ORL_ASSIGN_MOST_USED ? (key >> KEY_SLOT_BITS) : KEY_SUM_MAX - (key >> KEY_SLOT_BITS); }
__device__ __forceinline__ int key_sum_slot(int key) { return KEY_SLOT_MAX - (key & KEY_SLOT_MAX); }

// ---- best fit / exact fit ---------------------------------------------------------------------------------------------------------
// On r = fits(p), by the group's lane gl: over the maximal runs of r that start in word gl (none for gl >= W) the smallest
// key_run(l, start), the run having l + 1 bits — a free run of n + l slots.  The run's last bit is the lowest "last bit of a run" at
// or above its start: in word gl, or the lowest one of the words above.  KEY_NO_RUN: no run starts there
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
  int key = KEY_NO_RUN;
  while (sw) {
    const int b = (int)__builtin_ctzll(sw);
    sw &= sw - 1ull;
    const u64 x = ew & (~0ull << b);
    const int s = 64 * gl + b, e = x ? 64 * gl + (int)__builtin_ctzll(x) : later;
    const int k = key_run(e - s, s);
    key = k < key ? k : key;
  }
  return key;
}
// The rule's slot and cost (orl_route.h) from the smallest run key of r = fits(p), which has a set bit: BEST_FIT the shortest run;
// EXACT_FIT the same if it has exactly n slots, else first fit
template <int W> __device__ __forceinline__ void assign_run_choice(int rule, int key, const Row<W>& r, int& slot, int& cost) {
  const int over = key_run_over(key);
  if (rule == ORL_ASSIGN_BEST_FIT || over == 0) { slot = key_run_start(key); cost = over; }
  else { slot = row_ctz<W>(r); cost = 1 + slot; }
}

// ---- most used / least used -------------------------------------------------------------------------------------------------------
// a + b + c of three rows of equal weight: the sum row and the carry row (weight 2)
__device__ __forceinline__ void assign_csa(u64 a, u64 b, u64 c, u64& sum, u64& carry) {
  const u64 t = a ^ b;
  sum = t ^ c;
  carry = (a & b) | (t & c);
}
// the planes + x of weight 2^FROM
template <int FROM> __device__ __forceinline__ void assign_ripple(u64 (&pl)[COUNT_PLANES], u64 x) {
#pragma unroll
  for (int j = FROM; j < COUNT_PLANES; j++) {
    const u64 t = pl[j] & x;
    pl[j] ^= x;
    x = t;
  }
}
// u[w] of the byte counters in LDS: slot w at byte (w >> 6) * 68 + (w & 63) of the env's part
__device__ __forceinline__ int assign_count(const unsigned char* u, int w) { return (int)u[(w >> 6) * (4 * ASSIGN_WORD_DWORDS) + (w & 63)]; }

template <int W, bool CNT>
__global__ void __launch_bounds__(256) k_assign_spectrum(DevParams P, int rule, int n_given, const int* given, int gstride) {
  const ViewLanes v = view_lanes();
  if (v.env >= P.B) return;  // (whole groups: the ballot and the exchanges below stay within a group)
  const int lane = v.lane, gl = v.gl;
  const int E = P.E;
  const bool rwa = P.env_type == ENV_RWA;
  const PendingSvc sv = view_pending(P, v.env);
  const int np = sv.np;
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
      const int pidx = sv.pb + p0 + q;
      n = view_need(P, sv, pidx, rwa);
      // bit s: s .. s + n - 1 free on every hop (bits >= S of the AND-row are 0, so s + n <= S)
      r = row_runs_ge<W>(view_path_row<W>(P, sv.bm, pidx, 0), n);
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
        int cost;
        assign_run_choice<W>(rule, g8_min(assign_runs_key<W>(wr, gl)), wr, slot, cost);
      }
    } else {
      // u[w] of this lane's 64 slots, bit-sliced (the same construction as route_counts, orl_route.h: kept apart)
      u64 pl[COUNT_PLANES];
#pragma unroll
      for (int j = 0; j < COUNT_PLANES; j++) pl[j] = 0ull;
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
        u32* o = mine + ASSIGN_WORD_DWORDS * gl;
        for (int qd = 0; qd < 16; qd++) {
          u32 acc = 0u;
#pragma unroll
          for (int j = 0; j < COUNT_PLANES; j++) acc += view_nibble_bytes((u32)(pl[j] >> (4 * qd)) & 15u) << j;
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
      const unsigned char* u = (const unsigned char*)mine;
      int key = -1;
      if (fw) {
        const int lo = 64 * gl + (int)__builtin_ctzll(fw), hi = 64 * gl + 63 - (int)__builtin_clzll(fw);
        int U = 0;
        for (int w = lo; w < lo + n; w++) U += assign_count(u, w);
        for (int s = lo;; s++) {
          if ((fw >> (s & 63)) & 1ull) {
            const int k = key_sum(rule, U, s);
            key = k > key ? k : key;
          }
          if (s == hi) break;
          U += assign_count(u, s + n) - assign_count(u, s);  // (s + n <= hi + n - 1 < S)
        }
      }
      slot = key_sum_slot(g8_max(key));
    }
  }
  if (gl == 0) view_store_action<false>(P, v.env, best >= 0, make_int4(p0 + best, slot, 0, 0));
}
#endif
