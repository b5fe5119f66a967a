// view_rows.hip — test-only unit (tests/test_view_rows_gpu.py): a thin kernel around view_store_rows of orl_view.h, the way from a
// wavefront's bit rows in LDS to its 8 envs' output rows that the action-mask kernels share.  The launcher takes HOST pointers,
// copies in, launches, copies out and returns the first HIP error (0 = ok).  Nothing here is part of the library.
#include "orl_device.h"

using namespace orl;

#include "orl_view.h"  // (behind the using-directive, as in the library's units)

extern __shared__ __attribute__((aligned(16))) unsigned char vr_lds[];

// one wavefront per 8 envs: its part of the caller's image (per env `ew` = nrows * rw + 2 words: the bit rows, the pad word, the
// flag word) into LDS, then the shared streamer
__global__ void __launch_bounds__(64) k_view_rows(const u32* image, int nrows, int rw, int cpp, int allow_rejection, i64 B, unsigned char* out, int pitch) {
  const ViewLanes v = view_lanes();
  const int ew = nrows * rw + 2;
  u32* lds = (u32*)vr_lds;
  const u32* mine = image + v.env0 * ew;
  for (int i = v.lane; i < 8 * ew; i += 64) lds[i] = mine[i];
  wave_fence();
  view_store_rows(lds, nrows, rw, cpp, ew, nrows * rw, allow_rejection, v.env0, B, out, pitch);
}

// image: [blocks * 8][nrows * rw + 2] u32; out: [blocks * 8][pitch] bytes, handed to the device as the caller filled it and read back
// whole (blocks = ceil(B / 8): the rows of the envs >= B are there to be left alone)
extern "C" int vr_store_rows(const void* image, int nrows, int rw, int cpp, int allow_rejection, long long B, void* out, int pitch) {
  const int ew = nrows * rw + 2;
  const size_t blocks = (size_t)((B + 7) / 8), img_bytes = blocks * 8 * ew * sizeof(u32), out_bytes = blocks * 8 * (size_t)pitch;
  if (B < 1 || nrows < 1 || rw < 1 || cpp < 1 || cpp > 32 * rw || pitch % 16 || pitch < nrows * cpp + 1 || 8 * ew * sizeof(u32) > 48 * 1024)
    return -1;
  void *d_img = nullptr, *d_out = nullptr;
  int err = (int)hipMalloc(&d_img, img_bytes);
  if (!err) err = (int)hipMalloc(&d_out, out_bytes);
  if (!err) err = (int)hipMemcpy(d_img, image, img_bytes, hipMemcpyHostToDevice);
  if (!err) err = (int)hipMemcpy(d_out, out, out_bytes, hipMemcpyHostToDevice);
  if (!err) {
    hipLaunchKernelGGL(k_view_rows, dim3((unsigned)blocks), dim3(64), 8 * ew * sizeof(u32), 0, (const u32*)d_img, nrows, rw, cpp, allow_rejection,
                       (i64)B, (unsigned char*)d_out, pitch);
    err = (int)hipGetLastError();
    const int s = (int)hipDeviceSynchronize();
    if (!err) err = s;
  }
  if (!err) err = (int)hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost);
  if (d_img) (void)hipFree(d_img);
  if (d_out) (void)hipFree(d_out);
  return err;
}
