// view_plan_sweep.cpp — csrc/orl_view_plan.h under the host sanitizers: view_shape and view_plan over the full product of the sizes
// tests/test_view_plan.py samples (every env family, row width, k, core count 1 .. 31, link count, modulation count, j, batch size,
// view and layout / rule / j), with the properties of that test asserted on every call.  Host code only, no device, no library:
//
//   hipcc --offload-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -I optical_rl_gym_amd/csrc tools/view_plan_sweep.cpp -o view_plan_sweep && ./view_plan_sweep
//
// Prints the number of calls and of refused plans; any sanitizer report or failed property ends it with a non-zero status.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/orl.h"
#include "orl_device.h"
using namespace orl;
// the per-env LDS sizes without their kernels, as the API unit takes them; orl_qos_obs.h as the per-W units do
#include "orl_mask.h"
#include "orl_rmcsa_mask.h"
#include "orl_assign.h"
#include "orl_link_obs.h"
#define ORL_W 1
#include "orl_qos_obs.h"
#undef ORL_W
#include "orl_view_plan.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s fails (env %d W %d B %lld N %d E %d K %d C %d S %d J %d M %d view %d arg %d)\n", __FILE__, __LINE__, #c, \
  P.env_type, W, (long long)P.B, P.N, P.E, P.K, P.C, P.S, P.J, P.M, view, arg); exit(1); } } while (0)

int main() {
  const int WS[7][2] = {{1, 64}, {2, 65}, {2, 128}, {5, 129}, {5, 320}, {8, 321}, {8, 512}};
  const int KS[] = {1, 5, 8, 9, 23, 24, 38, 39, 64}, ES[] = {1, 22, 43, 88, 128}, NS[] = {2, 14, 512}, JS[] = {1, 8}, MS[] = {1, 6, 32, 33};
  const long long BS[] = {1, 31, 32, 33, 65536};
  const int n_args[VIEW_COUNT] = {4, 4, 1, 6, 2, 1, 1};
  const int path_j[] = {1, 8};
  long long calls = 0, refused = 0, sum = 0;
  DevParams P;
  memset(&P, 0, sizeof P);
  for (int env = 0; env <= ORL_ENV_QOS; env++)
    for (const auto& ws : WS)
      for (int K : KS)
        for (int C = 1; C <= 31; C++)
          for (int E : ES)
            for (int N : NS)
              for (int J : JS)
                for (int M : MS)
                  for (long long B : BS) {
                    const int W = ws[0];
                    P.env_type = env; P.B = B; P.N = N; P.E = E; P.K = K; P.C = C; P.S = ws[1]; P.J = J; P.M = M;
                    for (int view = 0; view < VIEW_COUNT; view++)
                      for (int a = 0; a < n_args[view]; a++) {
                        const int arg = view == VIEW_PATH_FEATURES ? path_j[a] : a;
                        const ViewShape s = view_shape(P, view, arg);
                        const ViewPlan p = view_plan(P, W, view, arg);
                        calls++;
                        CHECK(s.pitch >= s.dim && s.pitch * s.elem_bytes % 16 == 0 && s.pitch - s.dim < 16 / s.elem_bytes);
                        if (!p.ok) {
                          refused++;
                          CHECK(!p.waves && !p.block && !p.grid && !p.lds_bytes && !p.staged && !p.chunk && !p.counted);
                          continue;
                        }
                        const long long per_wg = (view == VIEW_MATRIX_PATHS_OBS ? 1 : 8) * p.waves;
                        CHECK(p.waves == 1 || p.waves == 2 || p.waves == 4);
                        CHECK(p.block == 64 * p.waves);
                        CHECK(p.lds_bytes <= (view == VIEW_MATRIX_PATHS_OBS ? kViewLdsMax : kViewLdsDefault));
                        CHECK(((long long)p.grid - 1) * per_wg < B && B <= (long long)p.grid * per_wg);
                        CHECK(p.chunk >= 0 && p.chunk % 8 == 0 && (view == VIEW_LINK_FEATURES || !p.chunk));
                        sum += (long long)p.lds_bytes + p.grid + p.chunk + s.dim;
                      }
                  }
  printf("%lld calls, %lld refused, checksum %lld\n", calls, refused, sum);
  return 0;
}
