// rng_prims.hip — test-only unit (tests/test_rng_prims.py): thin kernels around the random draws of orl_device.h (Rng: 32-word
// window, one wavefront per env), orl_device_g8.h (RngG: 16-word window, 8 lanes per env) and orl_device_split.h (svc_generate:
// the persistent kernel's look-ahead), and around orl_log.  Every launcher takes HOST pointers, checks what the kernels index
// with, copies in, launches, copies out and returns the first HIP error (0 = ok, -1 = refused argument).  Nothing here is part
// of the library.
#include <initializer_list>
#include <string.h>
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
inline int first_of(std::initializer_list<int> errs) {
  for (const int e : errs)
    if (e) return e;
  return 0;
}
#define RG_TRY(x) do { const int e_ = (x); if (e_) return e_; } while (0)

__global__ void k_log(const double* x, double* out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = orl_log(x[i]);
}

// ---- word streams: n x rng_u32 from the update-behind state at pos, then the commit ---------------------------------------------
// one wavefront per case
__global__ void __launch_bounds__(64) k_words64(u32* mt, int* pos, int n, u32* words) {
  const int lane = lane_id();
  const size_t c = blockIdx.x;
  Env e;
  e.mt = mt + c * 624;
  e.mt_pos = pos[c];
  Rng r;
  rng_fill(e, r, lane);
  for (int k = 0; k < n; k++) {
    const u32 w = rng_u32(e, r, lane);
    if (lane == 0) words[c * (size_t)n + k] = w;
  }
  rng_commit(e, r, lane);
  if (lane == 0) pos[c] = e.mt_pos;
}
// 8 lanes per case, 8 cases per wavefront; split: the commit in its two halves (position, then the stores)
__global__ void __launch_bounds__(64) k_words8(u32* mt, int* pos, int n, int split, u32* words) {
  const int lane = lane_id(), gl = lane & 7;
  const size_t c = (size_t)blockIdx.x * 8 + (lane >> 3);
  g8::EnvG e;
  e.mt = mt + c * 624;
  e.mt_pos = pos[c];
  g8::RngG r;
  g8::rng_fill(e, r, gl);
  for (int k = 0; k < n; k++) {
    const u32 w = g8::rng_u32(e, r, lane);
    if (gl == (k & 7)) words[c * (size_t)n + k] = w;  // (every lane of the group holds the word: a different one writes each)
  }
  if (split) {
    g8::rng_commit_pos(e, r);
    const int p = e.mt_pos;
    g8::rng_commit_stores(e, r, gl);
    if (gl == 0) pos[c] = p;
  } else {
    g8::rng_commit(e, r, gl);
    if (gl == 0) pos[c] = e.mt_pos;
  }
}

// ---- draws: `reps` times one operation per case, then the commit ------------------------------------------------------------------
enum { OP_RANDOM = 0, OP_EXPO = 1, OP_CHOICE = 2, OP_CHOICE_PRE = 3, OP_RANDBELOW = 4 };
struct DrawArgs { int op, reps, n, rand_n, rand_bits; double lam; const double* cum; };

__device__ __forceinline__ u64 f64_bits(double v) { return (u64)__double_as_longlong(v); }

__global__ void __launch_bounds__(64) k_draw64(u32* mt, int* pos, DrawArgs a, u64* out) {
  const int lane = lane_id();
  const size_t c = blockIdx.x;
  Env e;
  e.mt = mt + c * 624;
  e.mt_pos = pos[c];
  Rng r;
  rng_fill(e, r, lane);
  const double cum_my = (a.op == OP_CHOICE_PRE) ? a.cum[lane < a.n - 1 ? lane : a.n - 1] : 0.0;
  for (int k = 0; k < a.reps; k++) {
    u64 v = 0ull;
    if (a.op == OP_RANDOM) v = f64_bits(rng_random(e, r, lane));
    else if (a.op == OP_EXPO) v = f64_bits(rng_expovariate(e, r, lane, a.lam));
    else if (a.op == OP_CHOICE) v = (u64)(u32)rng_choice(e, r, lane, a.cum, a.n);
    else if (a.op == OP_CHOICE_PRE) v = (u64)(u32)rng_choice_pre(e, r, lane, cum_my, a.n);
    else {  // randint's _randbelow as next_service writes it
      u32 w = rng_u32(e, r, lane) >> (32 - a.rand_bits);
      while ((int)w >= a.rand_n) w = rng_u32(e, r, lane) >> (32 - a.rand_bits);
      v = w;
    }
    if (lane == 0) out[c * (size_t)a.reps + k] = v;
  }
  rng_commit(e, r, lane);
  if (lane == 0) pos[c] = e.mt_pos;
}
__global__ void __launch_bounds__(64) k_draw8(u32* mt, int* pos, DrawArgs a, u64* out) {
  const int lane = lane_id(), gl = lane & 7;
  const size_t c = (size_t)blockIdx.x * 8 + (lane >> 3);
  g8::EnvG e;
  e.mt = mt + c * 624;
  e.mt_pos = pos[c];
  g8::RngG r;
  g8::rng_fill(e, r, gl);
  for (int k = 0; k < a.reps; k++) {
    u64 v = 0ull;
    if (a.op == OP_RANDOM) v = f64_bits(g8::rng_random(e, r, lane));
    else if (a.op == OP_EXPO) v = f64_bits(g8::rng_expovariate(e, r, lane, a.lam));
    else if (a.op == OP_CHOICE) v = (u64)(u32)g8::rng_choice(e, r, lane, a.cum, a.n);
    else {
      u32 w = g8::rng_u32(e, r, lane) >> (32 - a.rand_bits);
      while ((int)w >= a.rand_n) w = g8::rng_u32(e, r, lane) >> (32 - a.rand_bits);
      v = w;
    }
    if (gl == (k & 7)) out[c * (size_t)a.reps + k] = v;
  }
  g8::rng_commit(e, r, gl);
  if (gl == 0) pos[c] = e.mt_pos;
}

// ---- svc_generate: one group of 8 lanes per case ------------------------------------------------------------------------------
#define RG_SENT_F64 0x7ff8dead00000001ull
#define RG_SENT_PK 0xdeadbeefu
#define RG_SENT_CNT (-7)
template <int ENV>
__global__ void __launch_bounds__(64) k_svc(DevParams P, u64* rec, u32* mt, const double2* rates, const int* n_want,
                                            const unsigned char* active, u64* q, u64* ht, u32* pk, int* cnt) {
  const int lane = lane_id();
  const size_t c = (size_t)blockIdx.x * 8 + (lane >> 3);
  sp::SvcBuf sb;
  sb.q = __longlong_as_double((i64)RG_SENT_F64);
  sb.ht = __longlong_as_double((i64)RG_SENT_F64);
  sb.pk = RG_SENT_PK;
  sb.cnt = RG_SENT_CNT;
  sp::svc_generate<ENV>(P, rec + c * ORL_SCAL_WORDS, mt + c * 624, rates ? rates + (size_t)blockIdx.x * 8 : nullptr, lane, n_want[c], sb,
                        active[c] != 0);
  const size_t o = c * 8 + (lane & 7);
  q[o] = f64_bits(sb.q); ht[o] = f64_bits(sb.ht); pk[o] = sb.pk; cnt[o] = sb.cnt;
}

inline bool pos_ok(const int* pos, int nc) {
  for (int i = 0; i < nc; i++)
    if (pos[i] < 0 || pos[i] >= 624) return false;
  return true;
}

}  // namespace

extern "C" int rg_log(const double* x, double* out, long long n) {
  if (n <= 0) return -1;
  DevBuf a(x, (size_t)n * 8, true), b(nullptr, (size_t)n * 8, false);
  RG_TRY(first_of({a.err, b.err}));
  k_log<<<(unsigned)((n + 255) / 256), 256>>>((const double*)a.d, (double*)b.d, (size_t)n);
  RG_TRY(finish());
  return b.down(out, (size_t)n * 8);
}

extern "C" int rg_words(int lanes, u32* mt, int* pos, int nc, int n, int split, u32* words) {
  if (nc <= 0 || n <= 0 || !pos_ok(pos, nc) || (lanes != 64 && lanes != 8) || (lanes == 8 && nc % 8)) return -1;
  const size_t mb = (size_t)nc * 624 * 4, wb = (size_t)nc * n * 4;
  DevBuf m(mt, mb, true), p(pos, (size_t)nc * 4, true), w(nullptr, wb, false);
  RG_TRY(first_of({m.err, p.err, w.err}));
  if (lanes == 64) k_words64<<<(unsigned)nc, 64>>>((u32*)m.d, (int*)p.d, n, (u32*)w.d);
  else k_words8<<<(unsigned)(nc / 8), 64>>>((u32*)m.d, (int*)p.d, n, split, (u32*)w.d);
  RG_TRY(finish());
  RG_TRY(m.down(mt, mb));
  RG_TRY(p.down(pos, (size_t)nc * 4));
  return w.down(words, wb);
}

extern "C" int rg_draw(int lanes, u32* mt, int* pos, int nc, int op, int reps, double lam, const double* cum, int n, int rand_n,
                       int rand_bits, u64* out) {
  if (nc <= 0 || reps <= 0 || !pos_ok(pos, nc) || (lanes != 64 && lanes != 8) || (lanes == 8 && nc % 8)) return -1;
  if (op < OP_RANDOM || op > OP_RANDBELOW || (op == OP_CHOICE_PRE && (lanes != 64 || n > 64))) return -1;
  if ((op == OP_CHOICE || op == OP_CHOICE_PRE) && (n < 1 || !cum)) return -1;
  if (op == OP_RANDBELOW && (rand_n < 1 || rand_bits < 1 || rand_bits > 31 || rand_n >= (1 << rand_bits))) return -1;  // (else no word is ever accepted)
  const size_t mb = (size_t)nc * 624 * 4, ob = (size_t)nc * reps * 8;
  DevBuf m(mt, mb, true), p(pos, (size_t)nc * 4, true), t(cum, cum ? (size_t)n * 8 : 0, true), o(nullptr, ob, false);
  RG_TRY(first_of({m.err, p.err, t.err, o.err}));
  DrawArgs a;
  a.op = op; a.reps = reps; a.n = n; a.rand_n = rand_n; a.rand_bits = rand_bits; a.lam = lam; a.cum = (const double*)t.d;
  if (lanes == 64) k_draw64<<<(unsigned)nc, 64>>>((u32*)m.d, (int*)p.d, a, (u64*)o.d);
  else k_draw8<<<(unsigned)(nc / 8), 64>>>((u32*)m.d, (int*)p.d, a, (u64*)o.d);
  RG_TRY(finish());
  RG_TRY(m.down(mt, mb));
  RG_TRY(p.down(pos, (size_t)nc * 4));
  return o.down(out, ob);
}

// kind: 0 = ENV_RMSA, randint bit rates; 1 = ENV_RMSA, discrete bit rates; 2 = ENV_RWA.  rates: [nc][2] or null (the two scalars).
// rec: [nc][ORL_SCAL_WORDS], mt: [nc][624], both in and out; q / ht (bit patterns) / pk / cnt: [nc][8], one entry per lane.
extern "C" int rg_svc(int kind, int N, const double* cum_src, const double* cum_dst, int rand_n, int rand_bits, int n_br,
                      const double* cum_br, double lambda_a, double lambda_h, const double* rates, int nc, u64* rec, u32* mt,
                      const int* n_want, const unsigned char* active, u64* q, u64* ht, u32* pk, int* cnt) {
  if (kind < 0 || kind > 2 || N < 2 || N > 512 || nc <= 0 || nc % 8 || !cum_src || !cum_dst) return -1;
  if (kind == 0 && (rand_n < 1 || rand_n > 4096 || rand_bits < 1 || rand_bits > 31 || rand_n >= (1 << rand_bits))) return -1;
  if (kind == 1 && (n_br < 1 || n_br > 4096 || !cum_br)) return -1;
  for (int i = 0; i < nc; i++) {
    if (n_want[i] < 0 || n_want[i] > 8) return -1;
    if ((rec[(size_t)i * ORL_SCAL_WORDS + SC_ID_MTPOS] >> 32) >= 624ull) return -1;
  }
  const size_t rb = (size_t)nc * ORL_SCAL_WORDS * 8, mb = (size_t)nc * 624 * 4, lb = (size_t)nc * 8;
  DevBuf cs(cum_src, (size_t)N * 8, true), cd(cum_dst, (size_t)N * N * 8, true), cb(cum_br, kind == 1 ? (size_t)n_br * 8 : 0, true),
      rt(rates, rates ? (size_t)nc * 16 : 0, true), r(rec, rb, true), m(mt, mb, true), nw(n_want, (size_t)nc * 4, true),
      ac(active, (size_t)nc, true), oq(nullptr, lb * 8, false), oh(nullptr, lb * 8, false), op(nullptr, lb * 4, false),
      oc(nullptr, lb * 4, false);
  RG_TRY(first_of({cs.err, cd.err, cb.err, rt.err, r.err, m.err, nw.err, ac.err, oq.err, oh.err, op.err, oc.err}));
  DevParams P;
  memset(&P, 0, sizeof(P));
  P.env_type = kind == 2 ? ENV_RWA : ENV_RMSA;
  P.N = N; P.cum_src = (const double*)cs.d; P.cum_dst = (const double*)cd.d;
  P.bit_rate_mode = kind == 1 ? 1 : 0; P.rand_n = rand_n; P.rand_bits = rand_bits; P.n_br = n_br;
  P.cum_br = kind == 1 ? (const double*)cb.d : nullptr;
  P.lambda_a = lambda_a; P.lambda_h = lambda_h;
  P.rates = rates ? (const double2*)rt.d : nullptr;
  const double2* rw = rates ? (const double2*)rt.d : nullptr;
  if (kind == 2)
    k_svc<ENV_RWA><<<(unsigned)(nc / 8), 64>>>(P, (u64*)r.d, (u32*)m.d, rw, (const int*)nw.d, (const unsigned char*)ac.d, (u64*)oq.d,
                                                (u64*)oh.d, (u32*)op.d, (int*)oc.d);
  else
    k_svc<ENV_RMSA><<<(unsigned)(nc / 8), 64>>>(P, (u64*)r.d, (u32*)m.d, rw, (const int*)nw.d, (const unsigned char*)ac.d, (u64*)oq.d,
                                                 (u64*)oh.d, (u32*)op.d, (int*)oc.d);
  RG_TRY(finish());
  RG_TRY(r.down(rec, rb));
  RG_TRY(m.down(mt, mb));
  RG_TRY(oq.down(q, lb * 8));
  RG_TRY(oh.down(ht, lb * 8));
  RG_TRY(op.down(pk, lb * 4));
  return oc.down(cnt, lb * 4);
}

// {ORL_SCAL_WORDS, SC_ID_MTPOS, SC_FLAGS, ORL_FLAG_EV_OVERFLOW, 8 * ORL_SVC_WIN, sentinel pk, sentinel cnt}
extern "C" void rg_consts(long long* out) {
  out[0] = ORL_SCAL_WORDS; out[1] = SC_ID_MTPOS; out[2] = SC_FLAGS; out[3] = ORL_FLAG_EV_OVERFLOW; out[4] = 8 * ORL_SVC_WIN;
  out[5] = (long long)RG_SENT_PK; out[6] = RG_SENT_CNT; out[7] = (long long)RG_SENT_F64;
}
