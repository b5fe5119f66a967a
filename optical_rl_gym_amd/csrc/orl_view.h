// orl_view.h — what the per-step device views of the pending service share (orl_mask.h, orl_rmcsa_mask.h, orl_path_obs.h,
// orl_link_obs.h, orl_qos_obs.h); included by orl_kernels.hip and orl_api.hip, after orl_device.h.
//
//   view_bits16_bytes  a 16-bit field -> 16 bytes of 0/1, one 16-byte store's worth (every byte view)
//   view_lanes         the opening of an 8-lanes-per-env kernel: 8 envs per wavefront, blockDim / 64 wavefronts per workgroup
//   view_pending       the pending service of an env, decoded from its scalar record
//   view_need          the slots the pending service needs on a path
//   view_path_row      the AND-row of a path's links, from its record
//   view_store_action  an env's row of ORL_BUF_ACTIONS, or its family's reject row, as one 16-byte store
//   view_obs_header    the float32 header of the feature rows (orl_path_obs.h, orl_link_obs.h) and their pad columns
//   view_store_rows    a wavefront's 8 envs' bit rows in LDS -> their output rows of 0/1 bytes, as 16-byte stores
// (The host side of the views — row shapes, launch geometry, the LDS budget rule view_waves — is orl_view_plan.h.  orl_device.h has no decode of the scalar record short of the whole Env; k_policy reads the svc_desc word instead.)
#pragma once

// 4 bits -> 4 bytes of 0/1 (bit i lands at bit 8 i; the four partial products do not overlap)
__device__ __forceinline__ u32 view_nibble_bytes(u32 x) { return (x * 0x00204081u) & 0x01010101u; }
// bit i of the low 16 -> byte i
__device__ __forceinline__ uint4 view_bits16_bytes(u32 bits) {
  uint4 o;
  o.x = view_nibble_bytes(bits & 15u);
  o.y = view_nibble_bytes((bits >> 4) & 15u);
  o.z = view_nibble_bytes((bits >> 8) & 15u);
  o.w = view_nibble_bytes((bits >> 12) & 15u);
  return o;
}

// lane of the wavefront, lane of the env's group of 8, wavefront of the workgroup, wavefronts per workgroup; the wavefront's first
// env and this lane's env (either may be >= B)
struct ViewLanes { int lane, gl, wv, waves; i64 env0, env; };
__device__ __forceinline__ ViewLanes view_lanes() {
  ViewLanes v;
  v.lane = lane_id(); v.gl = v.lane & 7; v.wv = (int)(threadIdx.x >> 6); v.waves = (int)(blockDim.x >> 6);
  v.env0 = ((i64)blockIdx.x * v.waves + v.wv) * 8;
  v.env = v.env0 + (v.lane >> 3);
  return v;
}

// the pending service of env (< B): SC_SRC_DST and SC_BR_IDX of its record; br: the raw word (bit_rate | br_idx << 32), np: the
// pair's number of paths, pb: index of its first path, bm: the env's slot maps
struct PendingSvc { int src, dst, br_idx; u64 br; int np, pb; const u64* bm; };
__device__ __forceinline__ PendingSvc view_pending(const DevParams& P, i64 env) {
  const u64* rec = P.scal + env * ORL_SCAL_WORDS;
  const u64 sd = rec[SC_SRC_DST];
  PendingSvc s;
  s.br = rec[SC_BR_IDX];
  s.src = (int)(u32)sd; s.dst = (int)(sd >> 32); s.br_idx = (int)(s.br >> 32);
  s.np = P.n_paths[s.src * P.N + s.dst];
  s.pb = (s.src * P.N + s.dst) * P.K;
  s.bm = P.bitmap + env * P.bm_words;
  return s;
}

// slots the pending service needs on path pidx (an index into the path tables: sv.pb + p) at its best modulation; RWA: one wavelength
__device__ __forceinline__ int view_need(const DevParams& P, const PendingSvc& sv, int pidx, bool rwa) {
  return rwa ? 1 : (int)P.nslots_path[(size_t)pidx * P.n_br + sv.br_idx];
}
// m(pidx): the AND of the path's link rows in `core` of the slot maps bm, bits >= S clear
template <int W> __device__ __forceinline__ Row<W> view_path_row(const DevParams& P, const u64* bm, int pidx, int core) {
  return path_and_rec<W>(path_rec_load(P, pidx), bm, P.E, P.S, core);
}
// env's row of ORL_BUF_ACTIONS, by one lane: `row` if found, else the reject action of the kernel's family — RMCSA (K, M, C, S), the
// others (K, S, 0, 0); each caller serves one of the two, so the family is the caller's constant
template <bool RMCSA> __device__ __forceinline__ void view_store_action(const DevParams& P, i64 env, bool found, int4 row) {
  int4 a = RMCSA ? make_int4(P.K, P.M, P.C, P.S) : make_int4(P.K, P.S, 0, 0);
  if (found) a = row;
  *(int4*)(P.actions + env * 4) = a;
}

// The header of a feature row o (LDS or global) of dim columns at a pitch of `pitch`, by the env group's 8 lanes: bit_rate / 100 (RWA:
// 0), the one-hots of min(src, dst) and max(src, dst) over N nodes each (deeprmsa_env.py:62-68); the pad columns dim .. pitch - 1 = 0
__device__ __forceinline__ void view_obs_header(const PendingSvc& sv, int N, bool rwa, int gl, int dim, int pitch, float* o) {
  const int mn = sv.src < sv.dst ? sv.src : sv.dst, mx = sv.src < sv.dst ? sv.dst : sv.src;
  const float rate = rwa ? 0.0f : (float)((double)(int)(u32)sv.br / 100);
  for (int i = gl; i < 1 + 2 * N; i += 8) o[i] = (i == 0) ? rate : ((i == 1 + mn || i == 1 + N + mx) ? 1.0f : 0.0f);
  for (int i = dim + gl; i < pitch; i += 8) o[i] = 0.0f;
}

// The wavefront's 8 output rows (envs env0 .. env0 + 7, those < B) from its LDS image: env el's words at lds + el * ew hold nrows
// bit rows of rw u32 words each (cpp <= 32 rw columns per row: column r * cpp + s of the output = bit s of row r), at word `tail`
// = the end of the last row a pad word — read past that row's end and masked off — and behind it the env's "has a
// provisioning column" flag.  The last column (nrows * cpp: reject) = allow_rejection; a row without a provisioning column and
// allow_rejection == 0 gets every other column set (the fallback of orl_mask.h); the pad columns up to `pitch` (a multiple of 16)
// are 0.  16 columns (bytes) per lane and store.  The image must be complete (wave_fence) before the call.
__device__ __forceinline__ void view_store_rows(const u32* lds, int nrows, int rw, int cpp, int ew, int tail, int allow_rejection, i64 env0,
                                                i64 B, unsigned char* out, int pitch) {
  const int ncols = nrows * cpp, nch = pitch >> 4;
  const int allow = allow_rejection != 0;
  for (int g = lane_id(); g < 8 * nch; g += 64) {
    const int el = g / nch, c = g - el * nch;
    const i64 e = env0 + el;
    if (e >= B) break;
    const u32* rows = lds + el * ew;
    const int c0 = 16 * c, c1 = c0 + 16 < ncols ? c0 + 16 : ncols;
    u32 bits = 0u;
    if (!allow && !rows[tail + 1]) {
      bits = c1 > c0 ? (1u << (c1 - c0)) - 1u : 0u;  // fallback
    } else {
      for (int col = c0; col < c1;) {
        const int r = col / cpp, s = col - r * cpp;
        const int take = cpp - s < c1 - col ? cpp - s : c1 - col;  // <= 16
        const u32* rp = rows + r * rw + (s >> 5);
        const int off = s & 31;
        u32 v = rp[0] >> off;
        if (off) v |= rp[1] << (32 - off);
        bits |= (v & ((1u << take) - 1u)) << (col - c0);
        col += take;
      }
    }
    if (allow && ncols >= c0 && ncols < c0 + 16) bits |= 1u << (ncols - c0);  // reject column
    *(uint4*)(out + e * pitch + c0) = view_bits16_bytes(bits);
  }
}
