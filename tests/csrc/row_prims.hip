// row_prims.hip — test-only unit (tests/test_row_prims.py): thin kernels around the slot-row primitives of orl_device.h and
// orl_device_split.h, one extern "C" launcher per row width W in {1, 2, 5, 8}.  Every launcher takes HOST pointers, copies in,
// launches, copies out and returns the first HIP error (0 = ok).  Nothing here is part of the library.
#include <initializer_list>
#include "orl_device.h"
#include "orl_device_g8.h"
#include "orl_device_split.h"

using namespace orl;

namespace {

struct DevBuf {
  void* d = nullptr;
  size_t bytes;
  int err = 0;
  DevBuf(const void* h, size_t n, bool copy_in) : bytes(n ? n : 8) {
    err = (int)hipMalloc(&d, bytes);
    if (!err && h && copy_in && n) err = (int)hipMemcpy(d, h, n, hipMemcpyHostToDevice);
    if (!err && !copy_in) err = (int)hipMemset(d, 0xff, bytes);
  }
  int down(void* h, size_t n) { return n ? (int)hipMemcpy(h, d, n, hipMemcpyDeviceToHost) : 0; }
  ~DevBuf() { if (d) (void)hipFree(d); }
};
inline int finish() {
  int e = (int)hipGetLastError();
  const int s = (int)hipDeviceSynchronize();
  return e ? e : s;
}
inline int first_of(std::initializer_list<int> errs) {  // the first HIP error of several buffers, 0 if none
  for (const int e : errs)
    if (e) return e;
  return 0;
}
inline unsigned blocks_of(size_t n, int per) { return (unsigned)((n + per - 1) / per); }

#define RP_BASIC_INTS 19
// one thread per row: everything that takes the row alone
template <int W>
__global__ void k_basic(const u64* rows, int nrows, int S, int* out, u64* starts, int* wl) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)nrows) return;
  const Row<W> r = row_load<W>(rows + i * W);
  u64 a[W];
#pragma unroll
  for (int w = 0; w < W; w++) a[w] = r.w[w];
  int* o = out + i * RP_BASIC_INTS;
  o[0] = row_popc<W>(r);
  o[1] = row_ctz<W>(r);
  o[2] = row_bitlen<W>(r);
  o[3] = row_longest_run<W>(r);
  int occ = -1, fb = -1;
  link_summary<W>(r, S, occ, fb);
  o[4] = occ; o[5] = fb;
  RowStat st;
  int me = -1, edge = -1;
  sp::row_stat_lane<W, false>(a, S, st, me, edge);
  o[6] = st.free_; o[7] = st.nf; o[8] = st.nu; o[9] = st.lo; o[10] = st.hi; o[11] = st.occ; o[12] = st.fb; o[13] = me; o[14] = edge;
  occ = -1; fb = -1;
  sp::row_occ_fb<W>(a, S, occ, fb);
  o[15] = occ; o[16] = fb;
  o[17] = sp::row_longest_free<W>(a);
  o[18] = (int)sp::row_inner_cache<W>(a);
  const Row<W> s = row_starts<W>(r);
#pragma unroll
  for (int w = 0; w < W; w++) {
    starts[i * W + w] = s.w[w];
    wl[(i * W + w) * 2] = word_longest_run(a[w]);
    wl[(i * W + w) * 2 + 1] = (a[w] != ~0ull) ? word_longest_run_flat(a[w]) : -1;  // (its precondition: at least one zero bit)
  }
}

// row_runs_ge for n = 1 .. 64: one thread per (row, n)
template <int W>
__global__ void k_runs_ge(const u64* rows, int nrows, u64* out) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)nrows * 64) return;
  const Row<W> r = row_runs_ge<W>(row_load<W>(rows + (idx >> 6) * W), (int)(idx & 63) + 1);
#pragma unroll
  for (int w = 0; w < W; w++) out[idx * W + w] = r.w[w];
}

// nth_block for every n of ns[] and want = 1 .. 8: one thread per (row, n, want) -> {found, start (-1: none)}
template <int W>
__global__ void k_nth(const u64* rows, int nrows, int S, const int* ns, int n_ns, int* out) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)nrows * n_ns * 8) return;
  const int want = (int)(idx & 7) + 1;
  const int n = ns[(idx >> 3) % n_ns];
  const size_t i = (idx >> 3) / n_ns;
  int start = -1;
  out[idx * 2] = nth_block<W>(row_load<W>(rows + i * W), S, n, want, start);
  out[idx * 2 + 1] = start;
}

// row_shr_small for st = 1 .. 63 and row_shr_lt32 for st = 1 .. 31: one thread per (row, st)
template <int W>
__global__ void k_shr(const u64* rows, int nrows, u64* out_small, u64* out_lt32) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)nrows * 63) return;
  const size_t i = idx / 63;
  const int st = (int)(idx % 63) + 1;
  const Row<W> r = row_load<W>(rows + i * W);
  const Row<W> a = row_shr_small<W>(r, st);
#pragma unroll
  for (int w = 0; w < W; w++) out_small[idx * W + w] = a.w[w];
  if (st < 32) {
    const Row<W> b = row_shr_lt32<W>(r, st);
#pragma unroll
    for (int w = 0; w < W; w++) out_lt32[(i * 31 + st - 1) * W + w] = b.w[w];
  }
}

// row_mask_lo(n) for n = 0 .. 64 W
template <int W>
__global__ void k_mask_lo(u64* out) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n > 64 * W) return;
  const Row<W> r = row_mask_lo<W>(n);
#pragma unroll
  for (int w = 0; w < W; w++) out[(size_t)n * W + w] = r.w[w];
}

// one thread per mask (s0[m], n[m]): row_range always; mask2 / mask2_word / mask_words / row_apply_mask where 1 <= n <= 63 and the
// mask lies inside the row (the split pipeline's masks).  buf[m] holds a row of the caller's: odd m provision, even m release.
template <int W>
__global__ void k_masks(const int* s0s, const int* ns, int nmask, int S, u64* out_range, u64* out_mask2, u32* out_words, u64* buf) {
  const size_t m = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= (size_t)nmask) return;
  const int s0 = s0s[m], n = ns[m];
  const Row<W> r = row_range<W>(s0, n);
#pragma unroll
  for (int w = 0; w < W; w++) out_range[m * W + w] = r.w[w];
  if (s0 >= 0 && n >= 1 && n <= 63 && s0 + n <= S && S <= 64 * W) {
    const sp::Mask2 mm = sp::mask2(s0, n);
#pragma unroll
    for (int w = 0; w < W; w++) out_mask2[m * W + w] = sp::mask2_word(mm, w);
    out_words[m] = sp::mask_words(s0, n);
    sp::row_apply_mask(buf + m * W, s0, n, (m & 1) != 0);
  }
}

// row_run_below / row_run_from for every p in 0 .. S: one thread per (row, p)
template <int W>
__global__ void k_runs(const u64* rows, int nrows, int S, int* out_below, int* out_from) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)nrows * (S + 1)) return;
  const size_t i = idx / (S + 1);
  const int p = (int)(idx % (S + 1));
  u64 a[W];
#pragma unroll
  for (int w = 0; w < W; w++) a[w] = rows[i * W + w];
  out_below[idx] = sp::row_run_below<W>(a, p);
  out_from[idx] = sp::row_run_from<W>(a, p);
}

// the 8-lane form: group g of a wavefront holds row 8 * wavefront + g, lane w of the group word w (0 for w >= W); EVERY lane writes
// what it got (nrows is a multiple of 8, one wavefront per block)
template <int W>
__global__ void k_row8(const u64* rows, int nrows, int S, int* out) {
  const int lane = lane_id();
  const int w = lane & 7;
  const size_t row = (size_t)blockIdx.x * 8 + (lane >> 3);
  const bool have = row < (size_t)nrows;
  const u64 a = (have && w < W) ? rows[row * W + w] : 0ull;
  RowStat st;
  row_stat<W, true>(a, w, S, st);
  const int longest = row_longest_run8<W>(a, w);
  if (have) {
    int* o = out + (row * 8 + w) * 8;
    o[0] = st.free_; o[1] = st.nf; o[2] = st.nu; o[3] = st.lo; o[4] = st.hi; o[5] = st.occ; o[6] = st.fb; o[7] = longest;
  }
}

#define RP_CACHED_INTS 10
// cached form: row1 = row0 with one mask applied; summarised with the cache word of row0 (variant 0) and with an all-unknown cache
// word (variant 1), update = true.  out[row][variant] = {free, nf, nu, lo, hi, occ, fb, max_empty, edge, cache word after}
template <int W>
__global__ void k_cached(const u64* rows, int nrows, int S, const int* s0s, const int* ns, int* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)nrows) return;
  const int s0 = s0s[i], n = ns[i];
  if (s0 < 0 || n < 1 || n > 63 || s0 + n > S) return;
  u64 a[W];
#pragma unroll
  for (int w = 0; w < W; w++) a[w] = rows[i * W + w];
  u32 cw[2];
  cw[0] = sp::row_inner_cache<W>(a);
  cw[1] = 0u;
#pragma unroll
  for (int w = 0; w < W; w++) cw[1] |= 63u << (6 * w);
  const sp::Mask2 mm = sp::mask2(s0, n);
#pragma unroll
  for (int w = 0; w < W; w++) a[w] ^= sp::mask2_word(mm, w);
  for (int v = 0; v < 2; v++) {
    RowStat st;
    int me = -1, edge = -1;
    sp::row_stat_lane<W, true>(a, S, st, me, edge, &cw[v], sp::mask_words(s0, n), true);
    int* o = out + (i * 2 + v) * RP_CACHED_INTS;
    o[0] = st.free_; o[1] = st.nf; o[2] = st.nu; o[3] = st.lo; o[4] = st.hi; o[5] = st.occ; o[6] = st.fb; o[7] = me; o[8] = edge;
    o[9] = (int)cw[v];
  }
}

// incremental form: RowInc starts from init[row] = {free, nu, lo, hi, longest}; `chain` masks per row, {s0, n, provision}; after each
// one the row's words and the five fields are written out
template <int W>
__global__ void k_inc(const u64* rows, int nrows, int S, const int* init, const int* masks, int chain, u64* out_rows, int* out_fields) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)nrows) return;
  u64 a[W];
#pragma unroll
  for (int w = 0; w < W; w++) a[w] = rows[i * W + w];
  sp::RowInc s;
  s.free_ = init[i * 5]; s.nu = init[i * 5 + 1]; s.lo = init[i * 5 + 2]; s.hi = init[i * 5 + 3]; s.me = init[i * 5 + 4];
  for (int c = 0; c < chain; c++) {
    const int* m = masks + (i * chain + c) * 3;
    if (m[0] < 0 || m[1] < 1 || m[1] > 63 || m[0] + m[1] > S) return;
    sp::row_inc_apply<W>(a, S, m[0], m[1], m[2] != 0, s);
#pragma unroll
    for (int w = 0; w < W; w++) out_rows[(i * chain + c) * W + w] = a[w];
    int* o = out_fields + (i * chain + c) * 5;
    o[0] = s.free_; o[1] = s.nu; o[2] = s.lo; o[3] = s.hi; o[4] = s.me;
  }
}

#define RP_TRY(x) do { const int e_ = (x); if (e_) return e_; } while (0)

template <int W> int run_basic(const u64* rows, int nrows, int S, int* out, u64* starts, int* wl) {
  const size_t rb = (size_t)nrows * W * 8;
  DevBuf r(rows, rb, true), o(nullptr, (size_t)nrows * RP_BASIC_INTS * 4, false), s(nullptr, rb, false), l(nullptr, (size_t)nrows * W * 8, false);
  RP_TRY(first_of({r.err, o.err, s.err, l.err}));
  k_basic<W><<<blocks_of(nrows, 256), 256>>>((const u64*)r.d, nrows, S, (int*)o.d, (u64*)s.d, (int*)l.d);
  RP_TRY(finish());
  RP_TRY(o.down(out, (size_t)nrows * RP_BASIC_INTS * 4));
  RP_TRY(s.down(starts, rb));
  return l.down(wl, (size_t)nrows * W * 8);
}
template <int W> int run_runs_ge(const u64* rows, int nrows, u64* out) {
  const size_t ob = (size_t)nrows * 64 * W * 8;
  DevBuf r(rows, (size_t)nrows * W * 8, true), o(nullptr, ob, false);
  RP_TRY(first_of({r.err, o.err}));
  k_runs_ge<W><<<blocks_of((size_t)nrows * 64, 256), 256>>>((const u64*)r.d, nrows, (u64*)o.d);
  RP_TRY(finish());
  return o.down(out, ob);
}
template <int W> int run_nth(const u64* rows, int nrows, int S, const int* ns, int n_ns, int* out) {
  const size_t ob = (size_t)nrows * n_ns * 8 * 2 * 4;
  DevBuf r(rows, (size_t)nrows * W * 8, true), n(ns, (size_t)n_ns * 4, true), o(nullptr, ob, false);
  RP_TRY(first_of({r.err, n.err, o.err}));
  k_nth<W><<<blocks_of((size_t)nrows * n_ns * 8, 256), 256>>>((const u64*)r.d, nrows, S, (const int*)n.d, n_ns, (int*)o.d);
  RP_TRY(finish());
  return o.down(out, ob);
}
template <int W> int run_shr(const u64* rows, int nrows, u64* out_small, u64* out_lt32) {
  const size_t sb = (size_t)nrows * 63 * W * 8, lb = (size_t)nrows * 31 * W * 8;
  DevBuf r(rows, (size_t)nrows * W * 8, true), a(nullptr, sb, false), b(nullptr, lb, false);
  RP_TRY(first_of({r.err, a.err, b.err}));
  k_shr<W><<<blocks_of((size_t)nrows * 63, 256), 256>>>((const u64*)r.d, nrows, (u64*)a.d, (u64*)b.d);
  RP_TRY(finish());
  RP_TRY(a.down(out_small, sb));
  return b.down(out_lt32, lb);
}
template <int W> int run_mask_lo(u64* out) {
  const size_t ob = (size_t)(64 * W + 1) * W * 8;
  DevBuf o(nullptr, ob, false);
  RP_TRY(first_of({o.err}));
  k_mask_lo<W><<<blocks_of(64 * W + 1, 64), 64>>>((u64*)o.d);
  RP_TRY(finish());
  return o.down(out, ob);
}
template <int W> int run_masks(const int* s0s, const int* ns, int nmask, int S, u64* out_range, u64* out_mask2, u32* out_words, u64* buf) {
  const size_t wb = (size_t)nmask * W * 8;
  DevBuf s(s0s, (size_t)nmask * 4, true), n(ns, (size_t)nmask * 4, true), a(nullptr, wb, false), b(nullptr, wb, false),
      c(nullptr, (size_t)nmask * 4, false), d(buf, wb, true);
  RP_TRY(first_of({s.err, n.err, a.err, b.err, c.err, d.err}));
  k_masks<W><<<blocks_of(nmask, 256), 256>>>((const int*)s.d, (const int*)n.d, nmask, S, (u64*)a.d, (u64*)b.d, (u32*)c.d, (u64*)d.d);
  RP_TRY(finish());
  RP_TRY(a.down(out_range, wb));
  RP_TRY(b.down(out_mask2, wb));
  RP_TRY(c.down(out_words, (size_t)nmask * 4));
  return d.down(buf, wb);
}
template <int W> int run_runs(const u64* rows, int nrows, int S, int* out_below, int* out_from) {
  const size_t ob = (size_t)nrows * (S + 1) * 4;
  DevBuf r(rows, (size_t)nrows * W * 8, true), a(nullptr, ob, false), b(nullptr, ob, false);
  RP_TRY(first_of({r.err, a.err, b.err}));
  k_runs<W><<<blocks_of((size_t)nrows * (S + 1), 256), 256>>>((const u64*)r.d, nrows, S, (int*)a.d, (int*)b.d);
  RP_TRY(finish());
  RP_TRY(a.down(out_below, ob));
  return b.down(out_from, ob);
}
template <int W> int run_row8(const u64* rows, int nrows, int S, int* out) {
  if (nrows % 8) return -1;
  const size_t ob = (size_t)nrows * 64 * 4;
  DevBuf r(rows, (size_t)nrows * W * 8, true), o(nullptr, ob, false);
  RP_TRY(first_of({r.err, o.err}));
  k_row8<W><<<(unsigned)(nrows / 8), 64>>>((const u64*)r.d, nrows, S, (int*)o.d);
  RP_TRY(finish());
  return o.down(out, ob);
}
template <int W> int run_cached(const u64* rows, int nrows, int S, const int* s0s, const int* ns, int* out) {
  if (W > 5) return -1;  // the cache word holds five 6-bit entries
  const size_t ob = (size_t)nrows * 2 * RP_CACHED_INTS * 4;
  DevBuf r(rows, (size_t)nrows * W * 8, true), s(s0s, (size_t)nrows * 4, true), n(ns, (size_t)nrows * 4, true), o(nullptr, ob, false);
  RP_TRY(first_of({r.err, s.err, n.err, o.err}));
  k_cached<(W > 5 ? 5 : W)><<<blocks_of(nrows, 256), 256>>>((const u64*)r.d, nrows, S, (const int*)s.d, (const int*)n.d, (int*)o.d);
  RP_TRY(finish());
  return o.down(out, ob);
}
template <int W> int run_inc(const u64* rows, int nrows, int S, const int* init, const int* masks, int chain, u64* out_rows, int* out_fields) {
  const size_t rb = (size_t)nrows * chain * W * 8, fb = (size_t)nrows * chain * 5 * 4;
  DevBuf r(rows, (size_t)nrows * W * 8, true), i(init, (size_t)nrows * 5 * 4, true), m(masks, (size_t)nrows * chain * 3 * 4, true),
      a(nullptr, rb, false), b(nullptr, fb, false);
  RP_TRY(first_of({r.err, i.err, m.err, a.err, b.err}));
  k_inc<W><<<blocks_of(nrows, 64), 64>>>((const u64*)r.d, nrows, S, (const int*)i.d, (const int*)m.d, chain, (u64*)a.d, (int*)b.d);
  RP_TRY(finish());
  RP_TRY(a.down(out_rows, rb));
  return b.down(out_fields, fb);
}

}  // namespace

#define RP_INST(W) \
  extern "C" int rp_basic_w##W(const u64* rows, int nrows, int S, int* out, u64* starts, int* wl) { return run_basic<W>(rows, nrows, S, out, starts, wl); } \
  extern "C" int rp_runs_ge_w##W(const u64* rows, int nrows, u64* out) { return run_runs_ge<W>(rows, nrows, out); } \
  extern "C" int rp_nth_w##W(const u64* rows, int nrows, int S, const int* ns, int n_ns, int* out) { return run_nth<W>(rows, nrows, S, ns, n_ns, out); } \
  extern "C" int rp_shr_w##W(const u64* rows, int nrows, u64* a, u64* b) { return run_shr<W>(rows, nrows, a, b); } \
  extern "C" int rp_mask_lo_w##W(u64* out) { return run_mask_lo<W>(out); } \
  extern "C" int rp_masks_w##W(const int* s0s, const int* ns, int nmask, int S, u64* a, u64* b, u32* c, u64* buf) { return run_masks<W>(s0s, ns, nmask, S, a, b, c, buf); } \
  extern "C" int rp_runs_w##W(const u64* rows, int nrows, int S, int* a, int* b) { return run_runs<W>(rows, nrows, S, a, b); } \
  extern "C" int rp_row8_w##W(const u64* rows, int nrows, int S, int* out) { return run_row8<W>(rows, nrows, S, out); } \
  extern "C" int rp_cached_w##W(const u64* rows, int nrows, int S, const int* s0s, const int* ns, int* out) { return run_cached<W>(rows, nrows, S, s0s, ns, out); } \
  extern "C" int rp_inc_w##W(const u64* rows, int nrows, int S, const int* init, const int* masks, int chain, u64* a, int* b) { return run_inc<W>(rows, nrows, S, init, masks, chain, a, b); }
RP_INST(1)
RP_INST(2)
RP_INST(5)
RP_INST(8)

extern "C" int rp_basic_ints() { return RP_BASIC_INTS; }
extern "C" int rp_cached_ints() { return RP_CACHED_INTS; }
