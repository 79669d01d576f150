// k_rewnorm.hip - reward scaling: the rewards of a rollout divided by the running standard deviation of the discounted return, before GAE reads them.
// The reference has no counterpart (train.py:185-205 takes the raw reward); what users of PPO know as gym's `NormalizeReward`, SB3's
// `VecNormalize(norm_reward=True)` and Brax's `reward_scaling`.  Off by default.
//
//   reward_norm_apply_kernel  once per rollout, one thread per environment (the geometry of gae_kernel: loads coalesced over n), forward over t = 0 .. T - 1:
//                             ret = ret * gamma + reward[t][n] in float32 - a multiply, then an add, two roundings - from ret = carry[n];
//                             d = (double)ret - (double)table[0] goes into S1 = sum d and S2 = sum d^2; scaled[t][n] = reward[t][n] * table[1] in float32,
//                             clamped to [-clip, clip] where clip > 0; then, where done[t][n], ret = 0 (SB3's order: the return that ends an episode is
//                             counted, then the carry restarts); at the end carry[n] = ret.  table = [mean32 | inv_std32]: the mean only shifts the
//                             sums (as in k_obsnorm.hip) - rewards are scaled, never centred.
//                             partial[g] = (S1, S2) of workgroup g in float64, in ONE order: the thread's own steps in t order, then the 64 lanes of its
//                             wave (wave_sum_f64 of wave_ops.h), then the four waves in wave order.  No atomics, nothing that depends on which wave
//                             arrives first: the same inputs give the same bytes.  Threads with n >= N add zeros and write nothing.
//
// The running statistics need no kernel of their own: obs_norm_update_kernel (k_obsnorm.hip) with O = 1 and table_ld = 1 is Chan's merge of the [G][2]
// partials into (n | mean | M2) and writes [mean32 | inv_std32].
//
// This file is compiled without floating-point contraction (minppo_amd/build.py): `ret * gamma + reward` is specified as two float32 roundings, and the tests
// restate it so; a fused multiply-add would round once and differ in the last bit.
#include <wave_ops.h>

#include "rewnorm.h"

namespace mppo {

// (`reward` and `scaled` may be one array: a thread reads its own words of a chunk before it writes them, and nobody else's)
__global__ void __launch_bounds__(kRewNormThreads) reward_norm_apply_kernel(int T, int N, float gamma, const float* reward, const unsigned char* __restrict__ done,
                                                                            float* __restrict__ carry, const float* __restrict__ table, float clip, float* scaled,
                                                                            double* __restrict__ partial) {
  __shared__ double red[kRewNormThreads / 64][2];
  const int n = (int)blockIdx.x * kRewNormThreads + (int)threadIdx.x;
  double s1 = 0.0, s2 = 0.0;
  if (n < N) {
    const double mean = (double)table[0];
    const float inv_std = table[1];
    float ret = carry[n];
    // the T steps in chunks of eight whose loads are all requested before the first is consumed (the recurrence is a dependent chain, the loads are not)
    for (int t0 = 0; t0 < T; t0 += 8) {
      float r8[8];
      unsigned char d8[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int t = t0 + u < T ? t0 + u : T - 1;
        r8[u] = reward[(size_t)t * N + n];
        d8[u] = done[(size_t)t * N + n];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (t0 + u < T) {
          const float r = r8[u];
          ret = ret * gamma + r;
          const double d = (double)ret - mean;
          s1 += d;
          s2 += d * d;
          float v = r * inv_std;
          if (clip > 0.f) v = v > clip ? clip : (v < -clip ? -clip : v);  // (a NaN stays a NaN)
          scaled[(size_t)(t0 + u) * N + n] = v;
          if (d8[u]) ret = 0.f;
        }
      }
    }
    carry[n] = ret;
  }
  if (partial) {  // (the same in every thread)
    s1 = wave_sum_f64(s1);
    s2 = wave_sum_f64(s2);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = s1; red[threadIdx.x >> 6][1] = s2; }
    __syncthreads();
    if (threadIdx.x < 2) {  // one thread per sum: the waves in wave order
      double sum = red[0][threadIdx.x];
      for (int w = 1; w < kRewNormThreads / 64; ++w) sum += red[w][threadIdx.x];
      partial[(size_t)blockIdx.x * 2 + threadIdx.x] = sum;
    }
  }
}

int32_t reward_norm_apply_launch(int T, int N, float gamma, const float* reward, const unsigned char* done, float* carry, const float* table, float clip, float* scaled,
                                 double* partial, hipStream_t stream) {
  hipLaunchKernelGGL(reward_norm_apply_kernel, dim3(reward_norm_partials(N)), dim3(kRewNormThreads), 0, stream, T, N, gamma, reward, done, carry, table, clip, scaled,
                     partial);
  MPPO_CHECK_LAUNCH("reward_norm_apply_kernel");
  return MPPO_OK;
}

}  // namespace mppo

using namespace mppo;

extern "C" int32_t mppo_reward_norm_partials(int32_t N) { return N >= 1 ? reward_norm_partials(N) : 0; }

extern "C" int32_t mppo_reward_norm_apply(int32_t T, int32_t N, float gamma, const float* reward, const uint8_t* done, float* carry, const float* table, float clip,
                                          float* scaled, double* partial, void* stream) {
  MPPO_REQUIRE(T >= 1 && N >= 1, "mppo_reward_norm_apply: T = %d steps, N = %d environments", T, N);
  MPPO_REQUIRE(reward && done && carry && table && scaled, "mppo_reward_norm_apply: null reward / done / carry / table / scaled");
  MPPO_REQUIRE(clip >= 0.f, "mppo_reward_norm_apply: clip %g is negative (or not a number)", (double)clip);
  MPPO_REQUIRE(((reinterpret_cast<uintptr_t>(reward) | reinterpret_cast<uintptr_t>(carry) | reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(scaled)) & 3) == 0 &&
                   (reinterpret_cast<uintptr_t>(partial) & 7) == 0,
               "mppo_reward_norm_apply: reward / carry / table / scaled must be 4-byte aligned, the partials 8-byte aligned");
  return reward_norm_apply_launch(T, N, gamma, reward, done, carry, table, clip, scaled, partial, static_cast<hipStream_t>(stream));
}
