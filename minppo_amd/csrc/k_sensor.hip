// k_sensor.hip - sensor noise and actuation latency (sensor.h): what the policy reads is the simulator's value plus noise, what it commands reaches the
// actuators some env steps later.  The reference has neither (env.py:245-261 returns the exact observation, env.py:148-196 applies the action at once);
// legged_gym's `add_noise` / `noise_scale_vec`, MuJoCo Playground's `noise_config` and action latency, Isaac Lab's `ActionDelay` are what users know.  Both
// are launches of their own beside the environment step - no flag in the step kernel or the row pass (DESIGN.md 3.9 has what one costs) - and off by default.
//
//   obs_noise_kernel     behind every env step (and the reset), on the rows it wrote: one lane per Philox block = four neighbouring columns of one row, lanes laid
//                        out along the row, so a wave reads and writes 1 KiB of consecutive words.  One 16-byte load and store per lane where the rows allow it
//                        (obs and sigma 16-byte aligned, obs_ld a multiple of 4), the one-column form otherwise.  A lane whose four sigmas are all zero leaves
//                        before it draws; a column whose sigma is zero, and the pad columns, are never written: every word has one writer, no atomics.
//   delay_fill_kernel    once: the latency table d[N].
//   action_delay_kernel  in front of every env step: one lane per (environment, action dimension) reads the ring's slot (timestep - d) mod D, writes the policy's
//                        action into slot timestep mod D and the delayed one into applied[N][A].  The ring is [D][N][A]: the timestep is the same in every
//                        environment that was reset together, so the written slot is one contiguous [N][A] block and the read one is contiguous per environment.
#include "sensor.h"

namespace mppo {

constexpr int kSensorThreads = 256;

__device__ __forceinline__ float noisy(float x, unsigned w, float s) {
  const float u = uniform_from_bits(w, -s, s);
#if defined(__HIP_DEVICE_COMPILE__)
  return __fadd_rn(x, u);
#else
  return x + u;
#endif
}

template <bool kVec>
__global__ void __launch_bounds__(kSensorThreads) obs_noise_kernel(ObsNoiseDraw p, int N, int O, int nblk, float* __restrict__ obs, int obs_ld,
                                                                   const float* __restrict__ sigma, const int* __restrict__ ctr, int mul, int add) {
  const long long g = (long long)blockIdx.x * kSensorThreads + threadIdx.x;
  if (g >= (long long)N * nblk) return;
  const int n = (int)(g / nblk), b = (int)(g - (long long)n * nblk), c0 = 4 * b;
  float s[4];
  if constexpr (kVec) {
    const float4 q = *reinterpret_cast<const float4*>(sigma + c0);
    s[0] = q.x; s[1] = q.y; s[2] = q.z; s[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = c0 + k < O ? sigma[c0 + k] : 0.f;
  }
  bool on[4], any = false, all = true;
#pragma unroll
  for (int k = 0; k < 4; ++k) { on[k] = c0 + k < O && s[k] > 0.f; any = any || on[k]; all = all && on[k]; }
  if (!any) return;
  const unsigned step = (ctr ? (unsigned)ctr[0] : 0u) * (unsigned)mul + (unsigned)add;  // (modulo 2^32: no signed overflow)
  const U4 r = obs_noise_block(p, (unsigned)n, step, (unsigned)b);
  const unsigned w[4] = {r.x, r.y, r.z, r.w};
  float* row = obs + (size_t)n * obs_ld + c0;
  float x[4];
  if constexpr (kVec) {
    const float4 q = *reinterpret_cast<const float4*>(row);
    x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = on[k] ? row[k] : 0.f;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) if (on[k]) x[k] = noisy(x[k], w[k], s[k]);
  if (kVec && all) {
    *reinterpret_cast<float4*>(row) = make_float4(x[0], x[1], x[2], x[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) if (on[k]) row[k] = x[k];
  }
}

__global__ void __launch_bounds__(kSensorThreads) delay_fill_kernel(DelayDraw p, int N, int* __restrict__ delay) {
  const int n = blockIdx.x * kSensorThreads + threadIdx.x;
  if (n < N) delay[n] = delay_draw(p, (unsigned)n);
}

__global__ void __launch_bounds__(kSensorThreads) action_delay_kernel(int N, int A, int D, const int* __restrict__ delay, const int* __restrict__ timestep,
                                                                      const int* __restrict__ episode_lengths, const float* __restrict__ action, int act_ld,
                                                                      float* __restrict__ hist, float* __restrict__ applied, int applied_ld) {
  const long long e = (long long)blockIdx.x * kSensorThreads + threadIdx.x;
  const long long NA = (long long)N * A;
  if (e >= NA) return;
  const int n = (int)(e / A), i = (int)(e - (long long)n * A);
  const unsigned ts = (unsigned)timestep[n];
  const int k = episode_lengths[n], d = delay[n];
  const float a = action[(size_t)n * act_ld + i];
  float out = a;  // d = 0: the very bits of the policy's action
  if (d != 0) out = k < d ? 0.f : hist[(size_t)((ts - (unsigned)d) % (unsigned)D) * NA + e];  // (read before the write below: d = D names the same slot)
  hist[(size_t)(ts % (unsigned)D) * NA + e] = a;
  applied[(size_t)n * applied_ld + i] = out;
}

int32_t check_obs_noise_cfg(const char* who, const mppo_obs_noise_cfg_t* c) {
  MPPO_REQUIRE(c, "%s: null observation-noise configuration", who);
  MPPO_REQUIRE(c->rank >= 0 && c->rank < 256, "%s: rank %d (0 .. 255)", who, c->rank);
  return MPPO_OK;
}

int32_t check_obs_noise_scale(const char* who, const float* scale, int O) {
  MPPO_REQUIRE(O >= 1 && (O + 3) / 4 <= 65536, "%s: %d observation columns (1 .. 262144: the Philox block index has 16 bits)", who, O);
  if (scale)
    for (int j = 0; j < O; ++j) MPPO_REQUIRE(scale[j] >= 0.f, "%s: noise scale %g of column %d is negative (or not a number)", who, (double)scale[j], j);
  return MPPO_OK;
}

int32_t check_action_delay_cfg(const char* who, const mppo_action_delay_cfg_t* c) {
  MPPO_REQUIRE(c, "%s: null action-delay configuration", who);
  MPPO_REQUIRE(c->min >= 0, "%s: action delay minimum %d is negative", who, c->min);
  MPPO_REQUIRE(c->min <= c->max, "%s: action delay minimum %d > maximum %d", who, c->min, c->max);
  MPPO_REQUIRE(c->max <= kMaxActionDelay, "%s: action delay maximum %d (at most %d env steps)", who, c->max, kMaxActionDelay);
  MPPO_REQUIRE(c->rank >= 0 && c->rank < 256, "%s: rank %d (0 .. 255)", who, c->rank);
  return MPPO_OK;
}

ObsNoiseDraw obs_noise_draw_of(const mppo_obs_noise_cfg_t& c) { return ObsNoiseDraw{c.seed, kStreamObsNoise + ((unsigned long long)c.rank << 16)}; }

DelayDraw delay_draw_of(const mppo_action_delay_cfg_t& c) { return DelayDraw{c.min, c.max, c.seed, kStreamDelay + ((unsigned long long)c.rank << 16)}; }

int32_t obs_noise_launch(const ObsNoiseDraw& p, int N, int O, float* obs, int obs_ld, const float* sigma, const int* ctr, int mul, int add, hipStream_t stream) {
  const int nblk = (O + 3) / 4;
  const dim3 grid(cdiv((long)N * nblk, kSensorThreads)), block(kSensorThreads);
  const bool vec = obs_ld % 4 == 0 && ((reinterpret_cast<uintptr_t>(obs) | reinterpret_cast<uintptr_t>(sigma)) & 15) == 0;
  if (vec) hipLaunchKernelGGL(obs_noise_kernel<true>, grid, block, 0, stream, p, N, O, nblk, obs, obs_ld, sigma, ctr, mul, add);
  else hipLaunchKernelGGL(obs_noise_kernel<false>, grid, block, 0, stream, p, N, O, nblk, obs, obs_ld, sigma, ctr, mul, add);
  MPPO_CHECK_LAUNCH("obs_noise_kernel");
  return MPPO_OK;
}

int32_t action_delay_fill_launch(const DelayDraw& p, int N, int* delay, hipStream_t stream) {
  hipLaunchKernelGGL(delay_fill_kernel, dim3(cdiv(N, kSensorThreads)), dim3(kSensorThreads), 0, stream, p, N, delay);
  MPPO_CHECK_LAUNCH("delay_fill_kernel");
  return MPPO_OK;
}

int32_t action_delay_launch(int N, int A, int D, const int* delay, const int* timestep, const int* episode_lengths, const float* action, int act_ld, float* hist,
                            float* applied, int applied_ld, hipStream_t stream) {
  hipLaunchKernelGGL(action_delay_kernel, dim3(cdiv((long)N * A, kSensorThreads)), dim3(kSensorThreads), 0, stream, N, A, D, delay, timestep, episode_lengths, action,
                     act_ld, hist, applied, applied_ld);
  MPPO_CHECK_LAUNCH("action_delay_kernel");
  return MPPO_OK;
}

}  // namespace mppo

using namespace mppo;

extern "C" int32_t mppo_obs_noise_apply(const mppo_obs_noise_cfg_t* cfg, int32_t N, int32_t O, float* obs, int32_t obs_ld, const float* sigma, const int32_t* counter,
                                        int32_t counter_mul, int32_t counter_add, void* stream) {
  MPPO_REQUIRE(obs && sigma, "mppo_obs_noise_apply: null observation / sigma");
  MPPO_REQUIRE(N >= 1, "mppo_obs_noise_apply: N = %d", N);
  MPPO_TRY(check_obs_noise_cfg("mppo_obs_noise_apply", cfg));
  MPPO_TRY(check_obs_noise_scale("mppo_obs_noise_apply", nullptr, O));
  MPPO_REQUIRE(obs_ld >= ((O + 3) & ~3), "mppo_obs_noise_apply: obs_ld %d < padded observation width %d", obs_ld, (O + 3) & ~3);
  MPPO_REQUIRE(((reinterpret_cast<uintptr_t>(obs) | reinterpret_cast<uintptr_t>(sigma)) & 3) == 0, "mppo_obs_noise_apply: observation and sigma must be 4-byte aligned");
  return obs_noise_launch(obs_noise_draw_of(*cfg), N, O, obs, obs_ld, sigma, counter, counter_mul, counter_add, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mppo_action_delay_fill(const mppo_action_delay_cfg_t* cfg, int32_t N, int32_t* delay, void* stream) {
  MPPO_REQUIRE(delay, "mppo_action_delay_fill: null output");
  MPPO_REQUIRE(N >= 1, "mppo_action_delay_fill: N = %d", N);
  MPPO_TRY(check_action_delay_cfg("mppo_action_delay_fill", cfg));
  return action_delay_fill_launch(delay_draw_of(*cfg), N, delay, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mppo_action_delay_apply(const mppo_action_delay_cfg_t* cfg, int32_t N, int32_t A, const int32_t* delay, const int32_t* timestep,
                                           const int32_t* episode_lengths, const float* action, int32_t act_ld, float* hist, float* applied, int32_t applied_ld,
                                           void* stream) {
  MPPO_REQUIRE(delay && timestep && episode_lengths && action && hist && applied, "mppo_action_delay_apply: null delay / timestep / episode_lengths / action / history / applied");
  MPPO_REQUIRE(N >= 1 && A >= 1, "mppo_action_delay_apply: N = %d, A = %d", N, A);
  MPPO_TRY(check_action_delay_cfg("mppo_action_delay_apply", cfg));
  MPPO_REQUIRE(cfg->max >= 1, "mppo_action_delay_apply: action delay maximum 0 is \"no latency\" - there is nothing to launch");
  MPPO_REQUIRE(act_ld >= A && applied_ld >= A, "mppo_action_delay_apply: act_ld %d / applied_ld %d < A = %d", act_ld, applied_ld, A);
  return action_delay_launch(N, A, cfg->max, delay, timestep, episode_lengths, action, act_ld, hist, applied, applied_ld, static_cast<hipStream_t>(stream));
}
