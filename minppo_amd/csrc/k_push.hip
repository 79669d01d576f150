// k_push.hip - mppo_push_fill: the random pushes' draw (push.h) written out as the [N][6] wrench array mppo_env_step_xfrc takes.  The engine and the
// evaluator draw inside the environment kernel and launch nothing here; this is the same function of (seed, rank, environment, step) for a caller who
// writes their sequences out by hand, and for the tests that hold the two bit-equal.
#include "push.h"

namespace mppo {

__global__ void __launch_bounds__(256) push_fill_kernel(PushDraw p, int N, const int* __restrict__ ctr, int mul, int add, float* __restrict__ xfrc) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const unsigned step = (ctr ? (unsigned)ctr[0] : 0u) * (unsigned)mul + (unsigned)add;  // (modulo 2^32: no signed overflow)
  float fx = 0.f, fy = 0.f;
  if (p.force > 0.f) (void)push_draw(p, (unsigned)n, step, &fx, &fy);
  float* o = xfrc + (size_t)n * 6;
  o[0] = fx; o[1] = fy; o[2] = 0.f; o[3] = 0.f; o[4] = 0.f; o[5] = 0.f;
}

int32_t push_fill_launch(const PushDraw& p, int N, const int* ctr, int mul, int add, float* xfrc, hipStream_t stream) {
  hipLaunchKernelGGL(push_fill_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, p, N, ctr, mul, add, xfrc);
  MPPO_CHECK_LAUNCH("push_fill_kernel");
  return MPPO_OK;
}

}  // namespace mppo

extern "C" int32_t mppo_push_fill(const mppo_push_cfg_t* cfg, int32_t N, const int32_t* counter, int32_t counter_mul, int32_t counter_add, float* xfrc, void* stream) {
  using namespace mppo;
  MPPO_REQUIRE(cfg && xfrc, "mppo_push_fill: null configuration / output");
  MPPO_REQUIRE(N >= 1, "mppo_push_fill: N = %d", N);
  MPPO_TRY(check_push_cfg("mppo_push_fill", cfg));
  return push_fill_launch(push_draw_of(*cfg), N, counter, counter_mul, counter_add, xfrc, static_cast<hipStream_t>(stream));
}
