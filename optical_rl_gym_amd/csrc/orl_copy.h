// orl_copy.h — k_copy_envs: env dst[p] of one batch becomes a copy of env src[p] of another (or of the same) batch, on the device
// (orl_batch_copy_envs, orl_api.hip).  Included by orl_api.hip: independent of the row width W, one instantiation.
//
// The state of an env is one row in each of the snapshot's sections (state_sections).  One workgroup per pair; its wavefronts share
// the sections out among themselves (wavefront w takes sections w, w + waves, ...), so the loads of up to four sections are in flight
// per workgroup; inside a section the lanes stride over chunks of the section's granularity — 16 bytes where the row size and both
// row addresses allow it, else 8 or 4, decided per section on the host — and a lane issues all the loads of a batch of
// ORL_COPY_BATCH chunks before its first store (rows up to 4 KB at 16 bytes: one batch).  Source and destination rows never
// overlap (copy_pairs_check, orl_copy_plan.h), which is what lets the loads be hoisted over the stores.
// Vector loads and stores only: no atomics, no LDS, no scratch.
#pragma once
#include "orl_device.h"

#define ORL_COPY_MAX_SECTIONS 14
#define ORL_COPY_BATCH 4
// threads per workgroup (= per pair).  256 against 64, cfg2, 65 536 pairs into a second batch: see DESIGN.md 4.8
#ifndef ORL_COPY_THREADS
#define ORL_COPY_THREADS 256
#endif
enum { COPY_PLAIN = 0, COPY_SCAL = 1, COPY_RNG = 2 };  // what keep_rng does to a section: nothing, merge the stream positions, skip

struct CopySection {
  const unsigned char* src;  // the section's array in the source batch
  unsigned char* dst;        // ... in the destination batch
  orl::u32 row_bytes;        // bytes per env
  orl::u32 gran : 8;         // bytes per access: 16, 8 or 4 (divides row_bytes and both bases)
  orl::u32 kind : 8;         // COPY_*
};
struct CopyTable {
  CopySection s[ORL_COPY_MAX_SECTIONS];
};

namespace orl {

// A batch of loaded chunks has to be in registers here: nothing but an ordering point for the compiler (no instruction), without
// which it sinks every load into the predicated block of its store — load, s_waitcnt vmcnt(0), store, four times over, the
// serialised pattern of DESIGN.md 4.3 (tools/isa_serial_loads.py).
static_assert(ORL_COPY_BATCH == 4, "copy_batch_ready names the four values of a batch");
__device__ __forceinline__ void copy_batch_ready(u32 (&v)[4]) { asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3])); }
__device__ __forceinline__ void copy_batch_ready(u64 (&v)[4]) { asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3])); }
__device__ __forceinline__ void copy_batch_ready(ulonglong2 (&v)[4]) {
  asm volatile("" : "+v"(v[0].x), "+v"(v[0].y), "+v"(v[1].x), "+v"(v[1].y), "+v"(v[2].x), "+v"(v[2].y), "+v"(v[3].x), "+v"(v[3].y));
}

// (every load of a batch is issued unconditionally, a chunk index past the row's end clamped to its last chunk — a repeated read
// of a line the lane's neighbours fetch anyway — so that the batch is straight-line code: predicated loads into an array made
// the compiler park the values in LDS)
template <typename T> __device__ __forceinline__ void copy_row(const T* __restrict__ s, T* __restrict__ d, int n, int lane) {
  for (int i = lane; i < n; i += 64 * ORL_COPY_BATCH) {
    T v[ORL_COPY_BATCH];
#pragma unroll
    for (int k = 0; k < ORL_COPY_BATCH; k++) v[k] = s[i + 64 * k < n ? i + 64 * k : n - 1];
    copy_batch_ready(v);
#pragma unroll
    for (int k = 0; k < ORL_COPY_BATCH; k++)
      if (i + 64 * k < n) d[i + 64 * k] = v[k];
  }
}

// keep_rng: the bits of word w of the scalar record that stay the destination's — the position in its stream (high half of
// SC_ID_MTPOS), the position in its second stream (high half of SC_HINT) and the mark that it has one (ORL_FLAG_MT2, in the flag
// half of SC_FLAGS).  Everything else, the service id in the low half of SC_ID_MTPOS included, is the source's.
__device__ __forceinline__ u64 copy_keep_mask(int w) {
  return (w == SC_ID_MTPOS || w == SC_HINT) ? 0xffffffff00000000ull : w == SC_FLAGS ? ((u64)ORL_FLAG_MT2 << 32) : 0ull;
}

// pairs: [2][n] env indices, sources then destinations
__global__ void __launch_bounds__(256) k_copy_envs(CopyTable T, int n_sec, const long long* __restrict__ pairs, i64 n, int keep_rng) {
  const i64 p = blockIdx.x;
  const i64 si = pairs[p], di = pairs[n + p];
  const int lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), waves = (int)(blockDim.x >> 6);
  for (int s = wave; s < n_sec; s += waves) {
    const CopySection sec = T.s[s];
    if (keep_rng && sec.kind == COPY_RNG) continue;  // the destination keeps its own streams
    const unsigned char* sp = sec.src + si * (i64)sec.row_bytes;
    unsigned char* dp = sec.dst + di * (i64)sec.row_bytes;
    if (keep_rng && sec.kind == COPY_SCAL) {
      // 16 lanes, one 16-byte chunk each: the destination's old words are read first, merged in registers, stored once
      if (lane < ORL_SCAL_WORDS / 2) {
        const ulonglong2 a = ((const ulonglong2*)sp)[lane], o = ((const ulonglong2*)dp)[lane];
        const u64 mx = copy_keep_mask(2 * lane), my = copy_keep_mask(2 * lane + 1);
        ulonglong2 r;
        r.x = (a.x & ~mx) | (o.x & mx);
        r.y = (a.y & ~my) | (o.y & my);
        ((ulonglong2*)dp)[lane] = r;
      }
      continue;
    }
    if (sec.gran == 16) copy_row((const ulonglong2*)sp, (ulonglong2*)dp, (int)(sec.row_bytes >> 4), lane);
    else if (sec.gran == 8) copy_row((const u64*)sp, (u64*)dp, (int)(sec.row_bytes >> 3), lane);
    else copy_row((const u32*)sp, (u32*)dp, (int)(sec.row_bytes >> 2), lane);
  }
}

}  // namespace orl
