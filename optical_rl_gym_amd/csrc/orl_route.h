// orl_route.h — routing rules and the per-path assignment table for RMSA and RWA actions (include/orl.h, orl_batch_route_spectrum);
// included by orl_kernels.hip behind orl_view.h and orl_assign.h, whose n(p), m(p), fits(p), u[], U(s), keys, counts' layout and best /
// exact fit decision are the ones used here.
//
// For EVERY candidate path p of the env's pending service the kernel computes the winner (s*(p), c*(p)) of the launch's rule — the
// slot orl_batch_assign_spectrum would choose on p, and an integer cost of that choice, smaller = better:
//   FIRST_FIT   c* = s*                         LAST_FIT    c* = S - n - s*
//   BEST_FIT    c* = L - n (L: the chosen run)  EXACT_FIT   c* = 0 for a run with L == n, else 1 + s*
//   MOST_USED   c* = n E - U(s*)                LEAST_USED  c* = U(s*)
//   MIN_CUTS    the s of fits(p) with the fewest cuts (ties: the lowest s), c* = cuts(p, s*); cuts(p, s) = the hops l of p on which
//               slots s - 1 and s + n both exist and are free: the block would split a free run of link l in two
// writes row p of the env's table as one 16-byte store (s*, c*, n(p), free(p) = popcount m(p)) — (S, ORL_ROUTE_NO_FIT, n, free)
// where nothing fits, (S, ORL_ROUTE_NO_FIT, 0, 0) for n_paths <= p < K — and reduces the rows to one action (p, s*(p), 0, 0) in
// ORL_BUF_ACTIONS under the launch's route over the paths that fit: KSP the lowest p, BEST the smallest c* (ties: the lowest p),
// LEAST_LOADED the largest free(p) (ties: the lowest p); no path fits: (K, S).
//
// Layout of the work: as k_assign_spectrum — 8 lanes per env, one candidate path per lane, chunks of 8 for k > 8 — but with no
// early exit: the table needs every path.  The route's running best stays in a register across the chunks, as ONE packed key
// reduced with g8_min (key_route).  Three instantiations, chosen by the launcher from the rule (route_mode_of):
//   ROUTE_PLAIN    rules 0 - 3: every lane on its own fits row (assign_runs_key word by word for best / exact fit); no LDS
//   ROUTE_COUNTED  rules 4, 5: u[] once per group into LDS, then the paths of the chunk that fit in turn: the path's fits row goes
//                  word by word to the group's lanes, lane w scans the window over word w, a g8_max gives the path's winner to its lane
//   ROUTE_CUTS     rule 6, bit-parallel: for hop l with free row f, (f << 1) & (f >> n) has bit s set exactly where a block at s
//                  cuts link l (bits >= S of f are 0 and nothing is shifted in at bit 0: the slots S and -1 do not exist); the rows
//                  of the hops add up in bit-sliced planes, the minimum over the set bits of fits(p) is taken plane by plane from
//                  the top (cand & ~plane where that is non-empty), its lowest bit is s*, and the count is read back from the
//                  planes at s*.  5 W 64-bit registers the other rules do not carry.
// No atomics, no host synchronisation: graph-capturable.  Env state and flags are only read.
#pragma once

enum { ROUTE_PLAIN = 0, ROUTE_COUNTED = 1, ROUTE_CUTS = 2 };
__host__ __device__ inline int route_mode_of(int rule) {
  return rule == ORL_ASSIGN_MIN_CUTS ? ROUTE_CUTS : (assign_rule_counted(rule) ? ROUTE_COUNTED : ROUTE_PLAIN);
}

#ifdef ORL_W  // (the kernel: the per-W units, orl_kernels.hip)
// (primary, p, s*) of a path that fits: the smallest key = the route's choice.  primary = 0 (KSP), c* (BEST) or S - free(p)
// (LEAST_LOADED); every key lies below ORL_ROUTE_NO_FIT, the key of "no fit"
enum { KEY_PATH_BITS = 6, KEY_PATH_MAX = (1 << KEY_PATH_BITS) - 1, ROUTE_CUT_PLANES = 5 };
constexpr long long kRoutePrimaryMax = ORL_MAX_NEED * ORL_MAX_LINKS > ORL_MAX_SLOTS ? ORL_MAX_NEED * ORL_MAX_LINKS : ORL_MAX_SLOTS;  // c* <= n E, 1 + s* or S - free <= S
static_assert(ORL_MAX_PATHS <= KEY_PATH_MAX + 1, "a path does not fit the route key's path field");
static_assert(((kRoutePrimaryMax << KEY_PATH_BITS | KEY_PATH_MAX) << KEY_SLOT_BITS | KEY_SLOT_MAX) < ORL_ROUTE_NO_FIT, "a route key reaches ORL_ROUTE_NO_FIT");
static_assert(ORL_MAX_HOPS < (1 << ROUTE_CUT_PLANES), "cuts(p, s) <= hops does not fit the cut planes");
__device__ __forceinline__ int key_route(int primary, int p, int s) { return (primary << (KEY_PATH_BITS + KEY_SLOT_BITS)) | (p << KEY_SLOT_BITS) | s; }
__device__ __forceinline__ int key_route_path(int key) { return (key >> KEY_SLOT_BITS) & KEY_PATH_MAX; }
__device__ __forceinline__ int key_route_slot(int key) { return key & KEY_SLOT_MAX; }

// a >> st, 1 <= st <= 64 (a service of 64 slots shifts by a whole word)
template <int W> __device__ __forceinline__ Row<W> route_shr(const Row<W>& a, int st) {
  if (st < 64) return row_shr_small<W>(a, st);
  Row<W> r;
#pragma unroll
  for (int i = 0; i < W; i++) r.w[i] = (i + 1 < W) ? a.w[i + 1] : 0ull;
  return r;
}
// a << 1 (bit 0 = 0; the top bit of the last word is dropped)
template <int W> __device__ __forceinline__ Row<W> route_shl1(const Row<W>& a) {
  Row<W> r;
#pragma unroll
  for (int i = 0; i < W; i++) r.w[i] = (a.w[i] << 1) | ((i > 0) ? (a.w[i - 1] >> 63) : 0ull);
  return r;
}

// m(p) of the path record, and into pl[j] bit j of cuts(p, s) for every s at once (ROUTE_CUTS)
template <int W> __device__ __forceinline__ Row<W> route_and_cuts(const PathRec& rec, const u64* bm, int S, int n, Row<W> (&pl)[ROUTE_CUT_PLANES]) {
  const Row<W> all = row_mask_lo<W>(S);
  Row<W> m = all;
#pragma unroll
  for (int j = 0; j < ROUTE_CUT_PLANES; j++) pl[j] = row_mask_lo<W>(0);
  const int hops = path_rec_byte(rec, 0);
  for (int h = 0; h < hops; h++) {
    const Row<W> f = row_and<W>(row_load<W>(bm + path_rec_byte(rec, 2 + h) * W), all);
    m = row_and<W>(m, f);
    Row<W> x = row_and<W>(route_shl1<W>(f), route_shr<W>(f, n));  // bit s: f[s - 1] and f[s + n]
#pragma unroll
    for (int j = 0; j < ROUTE_CUT_PLANES; j++) {  // planes += x
#pragma unroll
      for (int i = 0; i < W; i++) {
        const u64 t = pl[j].w[i] & x.w[i];
        pl[j].w[i] ^= x.w[i];
        x.w[i] = t;
      }
    }
  }
  return m;
}

// The winner (slot, cost) of rules 0 - 3 on r = fits(p) of a service of n slots, r having a set bit: every lane on its own row
// (ROUTE_PLAIN; orl_route_cores.h takes the same per (path, core) pair)
template <int W> __device__ __forceinline__ void route_plain_winner(int rule, const Row<W>& r, int S, int n, int& slot, int& cost) {
  if (rule == ORL_ASSIGN_FIRST_FIT) {
    slot = row_ctz<W>(r);
    cost = slot;
  } else if (rule == ORL_ASSIGN_LAST_FIT) {
    slot = row_bitlen<W>(r) - 1;
    cost = S - n - slot;
  } else {
    // the shortest run of the lane's own row (ties: the lowest start), over the runs of every word
    int key = KEY_NO_RUN;
#pragma unroll
    for (int i = 0; i < W; i++) {
      const int k = assign_runs_key<W>(r, i);
      key = k < key ? k : key;
    }
    assign_run_choice<W>(rule, key, r, slot, cost);
  }
}
// The winner of ORL_ASSIGN_MIN_CUTS on r = fits(p), r having a set bit, from the planes of route_and_cuts: the minimum over the set
// bits plane by plane from the top, its lowest bit, and the count read back from the planes there (ROUTE_CUTS)
template <int W> __device__ __forceinline__ void route_cuts_winner(const Row<W>& r, const Row<W> (&pl)[ROUTE_CUT_PLANES], int& slot, int& cost) {
  Row<W> cand = r;
#pragma unroll
  for (int j = ROUTE_CUT_PLANES - 1; j >= 0; j--) {
    const Row<W> t = row_andn<W>(cand, pl[j]);
    if (row_any<W>(t)) cand = t;
  }
  slot = row_ctz<W>(cand);
  cost = 0;
#pragma unroll
  for (int j = 0; j < ROUTE_CUT_PLANES; j++) {  // cuts(q, slot) back from the planes
    u64 x = 0ull;
#pragma unroll
    for (int i = 0; i < W; i++)
      if (i == (slot >> 6)) x = pl[j].w[i];
    cost |= (int)((x >> (slot & 63)) & 1ull) << j;
  }
}

// u[] of the env as byte counters in the group's part of LDS (ROUTE_COUNTED): the construction and layout of k_assign_spectrum<W,
// true> (orl_assign.h, which has it inline; assign_count reads both) — lane w < W counts the 64 slots of word w over all E link
// rows in bit-sliced planes and expands them to bytes.  Complete for the group's lanes on return.
template <int W> __device__ __forceinline__ const unsigned char* route_counts(const PendingSvc& sv, int E, const ViewLanes& v) {
  const int gl = v.gl;
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
  u32* mine = (u32*)orl_lds_raw + ((size_t)v.wv * 8 + (v.lane >> 3)) * assign_env_dwords(W);
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
  return (const unsigned char*)mine;
}

template <int W, int MODE>
__global__ void __launch_bounds__(256) k_route_spectrum(DevParams P, int rule, int route, int4* table) {
  const ViewLanes v = view_lanes();
  if (v.env >= P.B) return;  // (whole groups: the exchanges below stay within a group)
  const int lane = v.lane, gl = v.gl;
  const int K = P.K, S = P.S, E = P.E;
  const bool rwa = P.env_type == ENV_RWA;
  const PendingSvc sv = view_pending(P, v.env);
  const int np = sv.np < K ? sv.np : K;
  const unsigned char* u = nullptr;
  if constexpr (MODE == ROUTE_COUNTED) u = route_counts<W>(sv, E, v);
  int best = ORL_ROUTE_NO_FIT;
  for (int base = 0; base < K; base += 8) {
    const int q = base + gl;
    Row<W> r = row_mask_lo<W>(0);  // fits(q)
    int n = 0, nfree = 0, slot = S, cost = ORL_ROUTE_NO_FIT;
    Row<W> pl[MODE == ROUTE_CUTS ? ROUTE_CUT_PLANES : 1];
    if (q < np) {
      const int pidx = sv.pb + q;
      n = view_need(P, sv, pidx, rwa);
      const PathRec rec = path_rec_load(P, pidx);
      Row<W> m;
      if constexpr (MODE == ROUTE_CUTS) m = route_and_cuts<W>(rec, sv.bm, S, n, pl);
      else m = path_and_rec<W>(rec, sv.bm, E, S, 0);
      nfree = row_popc<W>(m);
      // bit s: s .. s + n - 1 free on every hop (bits >= S of the AND-row are 0, so s + n <= S)
      r = row_runs_ge<W>(m, n);
    }
    if constexpr (MODE == ROUTE_PLAIN) {
      if (row_any<W>(r)) route_plain_winner<W>(rule, r, S, n, slot, cost);
    } else if constexpr (MODE == ROUTE_COUNTED) {
      // the paths of the chunk that fit, in turn: word gl of the path's fits row and its n to every lane of the group
      u32 fit = g8::gballot(row_any<W>(r), lane);
      while (fit) {
        const int l = (int)__builtin_ctz(fit);
        fit &= fit - 1u;
        u64 fw = 0ull;
#pragma unroll
        for (int i = 0; i < W; i++) {
          const u64 x = g8::gget(r.w[i], l, lane);
          if (i == gl) fw = x;
        }
        const int nl = g8::gget(n, l, lane);
        int key = -1;
        if (fw) {
          const int lo = 64 * gl + (int)__builtin_ctzll(fw), hi = 64 * gl + 63 - (int)__builtin_clzll(fw);
          int U = 0;
          for (int w = lo; w < lo + nl; w++) U += assign_count(u, w);
          for (int s = lo;; s++) {
            if ((fw >> (s & 63)) & 1ull) {
              const int k = key_sum(rule, U, s);
              key = k > key ? k : key;
            }
            if (s == hi) break;
            U += assign_count(u, s + nl) - assign_count(u, s);  // (s + nl <= hi + nl - 1 < S)
          }
        }
        key = g8_max(key);
        if (gl == l) {
          const int U = key_sum_U(rule, key);
          slot = key_sum_slot(key);
          cost = rule == ORL_ASSIGN_MOST_USED ? n * E - U : U;
        }
      }
    } else {
      if (row_any<W>(r)) route_cuts_winner<W>(r, pl, slot, cost);
    }
    if (q < K) table[v.env * K + q] = make_int4(slot, cost, n, nfree);
    int key = ORL_ROUTE_NO_FIT;
    if (cost != ORL_ROUTE_NO_FIT) key = key_route(route == ORL_ROUTE_KSP ? 0 : (route == ORL_ROUTE_BEST ? cost : S - nfree), q, slot);
    key = g8_min(key);
    best = key < best ? key : best;
  }
  if (gl == 0) view_store_action<false>(P, v.env, best != ORL_ROUTE_NO_FIT, make_int4(key_route_path(best), key_route_slot(best), 0, 0));
}
#endif
