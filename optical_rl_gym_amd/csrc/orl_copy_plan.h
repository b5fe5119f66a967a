// orl_copy_plan.h — the host-side decisions of orl_batch_copy_envs (orl_api.hip): which pair lists it takes and which two batches
// have per-env rows that can be copied into each other.
//
// Like the form choice (orl_persist_form.h) and the run plan (orl_run_plan.h) both are pure functions, pinned without a device by
// tests/test_copy_plan.py (orl_debug_copy_pairs_check).  No HIP call in here.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "orl_device.h"

#define ORL_COPY_WHY 200  // bytes of a refusal's text

// The pairs a copy really moves: the caller's list without the no-ops (src == dst inside one batch).
struct CopyPairs {
  bool ok = false;
  std::vector<long long> src, dst;
};

// Index rules of a copy of n pairs (src[p] of a batch of B_src envs -> dst[p] of a batch of B_dst envs; same_batch: the two are one):
//   * every index lies inside its batch;
//   * no destination is written twice;
//   * inside one batch, no destination is also the source of another pair (pairs with src == dst are no-ops and dropped first):
//     the kernel is a single pass with no ordering between workgroups, so a row that is both read and written would be read
//     either before or after its overwrite.  A permutation goes through a scratch batch.
// O(n + B) with one bit per env.  `why` (ORL_COPY_WHY bytes) says which pair broke which rule.
static inline CopyPairs copy_pairs_check(int64_t B_src, int64_t B_dst, bool same_batch, int64_t n, const int64_t* src, const int64_t* dst,
                                         char* why) {
  CopyPairs out;
  why[0] = 0;
  if (n < 0) { snprintf(why, ORL_COPY_WHY, "n is %lld: the number of pairs cannot be negative", (long long)n); return out; }
  if (n == 0) { out.ok = true; return out; }
  if (!src || !dst) { snprintf(why, ORL_COPY_WHY, "null index array with n = %lld", (long long)n); return out; }
  std::vector<uint64_t> written((size_t)(B_dst + 63) / 64, 0), read;
  if (same_batch) read.assign((size_t)(B_src + 63) / 64, 0);
  for (int64_t p = 0; p < n; p++) {
    const int64_t s = src[p], d = dst[p];
    if (s < 0 || s >= B_src) {
      snprintf(why, ORL_COPY_WHY, "pair %lld: source index %lld outside [0, %lld)", (long long)p, (long long)s, (long long)B_src);
      return out;
    }
    if (d < 0 || d >= B_dst) {
      snprintf(why, ORL_COPY_WHY, "pair %lld: destination index %lld outside [0, %lld)", (long long)p, (long long)d, (long long)B_dst);
      return out;
    }
    uint64_t& w = written[(size_t)d >> 6];
    if (w >> (d & 63) & 1) {
      snprintf(why, ORL_COPY_WHY, "pair %lld: destination index %lld occurs twice", (long long)p, (long long)d);
      return out;
    }
    w |= 1ull << (d & 63);
    if (same_batch && s == d) continue;  // a no-op
    if (same_batch) read[(size_t)s >> 6] |= 1ull << (s & 63);
    out.src.push_back(s);
    out.dst.push_back(d);
  }
  if (same_batch)
    for (size_t p = 0; p < out.dst.size(); p++) {
      const long long d = out.dst[p];
      if (read[(size_t)d >> 6] >> (d & 63) & 1) {
        snprintf(why, ORL_COPY_WHY,
                 "env %lld is the destination of one pair (%lld -> %lld) and the source of another: a copy inside one batch is a single "
                 "pass; go through a scratch batch",
                 d, out.src[p], d);
        out.src.clear();
        out.dst.clear();
        return out;
      }
    }
  out.ok = true;
  return out;
}

// Do the per-env rows of two batches have one layout and one meaning?  Everything that sizes a section of the snapshot
// (state_sections, orl_api.hip) or decides what its entries index: the family, the topology's sizes, the spectrum, the pending-release
// capacity, the bit-rate table's size and mode, which histograms are kept, the QoS classes, the second streams.  The traffic rates
// are configuration and may differ.  (The topology tables' content is the caller's to compare: DevParams holds device pointers.)
static inline bool copy_layout_compatible(const orl::DevParams& a, const orl::DevParams& b, char* why) {
  why[0] = 0;
#define ORL_COPY_SAME_(F, WHAT)                                                                                     \
  if (a.F != b.F) {                                                                                                 \
    snprintf(why, ORL_COPY_WHY, "the batches differ in %s (%lld and %lld)", WHAT, (long long)a.F, (long long)b.F); \
    return false;                                                                                                   \
  }
  ORL_COPY_SAME_(env_type, "env family")
  ORL_COPY_SAME_(N, "nodes")
  ORL_COPY_SAME_(E, "links")
  ORL_COPY_SAME_(K, "k_paths")
  ORL_COPY_SAME_(H, "hops of the longest path")
  ORL_COPY_SAME_(M, "modulation formats")
  ORL_COPY_SAME_(S, "num_spectrum_resources")
  ORL_COPY_SAME_(C, "num_spatial_resources")
  ORL_COPY_SAME_(J, "j")
  ORL_COPY_SAME_(ev_cap, "event capacity (the loads they were created for)")
  ORL_COPY_SAME_(n_br, "number of bit rates")
  ORL_COPY_SAME_(bit_rate_mode, "bit-rate mode")
  ORL_COPY_SAME_(n_classes, "QoS classes")
  ORL_COPY_SAME_(bm_words, "slot-map words")
  ORL_COPY_SAME_(cs_words, "compactness-sum words")
#undef ORL_COPY_SAME_
  if (!a.br_hist != !b.br_hist || !a.act_hist != !b.act_hist) {
    snprintf(why, ORL_COPY_WHY, "one batch keeps bit-rate / action marginals and the other does not");
    return false;
  }
  if (!a.act2d != !b.act2d || a.act2d_words != b.act2d_words) {
    snprintf(why, ORL_COPY_WHY, "one batch was created with action_histograms and the other without");
    return false;
  }
  if (!a.mt2 != !b.mt2) {
    snprintf(why, ORL_COPY_WHY,
             "one batch carries second random streams (it was reseeded) and the other does not: seed() the other batch first — an all-zero "
             "mask allocates the streams without reseeding an env");
    return false;
  }
  return true;
}
