// k_limit.hip - the episode time limit (limit.h): mppo_env_time_limit truncates the environments that have reached it, the evaluator's two counting stages.
//
// The reference has no time limit (env.py:238-242 ends an episode on height only); Brax's EpisodeWrapper(episode_length), legged_gym and MuJoCo Playground train
// with one and treat reaching it as a truncation, not a failure.  It is a launch of its own behind the step (not a flag in the step kernel's epilogue:
// DESIGN.md 3.9 has what a run-time flag costs that kernel in registers): a truncated environment gets exactly what the epilogue (k_physics.hip, `if (done)`)
// writes for an ended episode - the flags, the returned_* metrics, zeroed running metrics, the reset record as its state row and the record's first OP words as
// its observation row - and every other environment keeps every bit.
//
//   time_limit_kernel        workgroups of 4 waves, a wave for 4 environments, the 16 lanes of a DPP row for one (one-wave workgroups measured no faster:
//                            profiles/time_limit_rate.txt): every lane of the row loads its environment's
//                            `done` and `episode_lengths` (one address per row: the test costs two loads; `timestep` is read only where a staggered first limit
//                            is due, the draw itself is arithmetic), lane 0 of the row writes the `truncated` byte.  A wave none of whose environments is
//                            truncated leaves there - truncations are rare, as ended episodes are for the step kernel - so the reset record is not even read.
//                            Otherwise the rows of the truncated environments copy the record, lane g words g, g + 16, ...: coalesced along the row.  Every word
//                            has one writer: no atomics.
//   eval_limit_count_kernel  once per evaluated step: one thread per environment counts its truncations and its terminations (done and not truncated).
//   eval_limit_reduce_kernel once at the end, ONE workgroup in a fixed order: the truncations' sum and the number of environments with a termination.
#include <wave_ops.h>

#include "limit.h"
#include "model_view.h"

namespace mppo {

const ModelView& model_view(const mppo_model* m);

constexpr int kLimitThreads = 256, kLimitLanes = 16, kLimitEnvs = kLimitThreads / kLimitLanes;

__global__ void __launch_bounds__(kLimitThreads) time_limit_kernel(LimitCfg c, int N, int rec_dim, int OP, float* __restrict__ state, const float* __restrict__ reset_rec,
                                                                    float* __restrict__ obs, int obs_ld, unsigned char* __restrict__ done,
                                                                    unsigned char* __restrict__ truncated, mppo_env_metrics_t met) {
  const int g = threadIdx.x & (kLimitLanes - 1);
  const int env = blockIdx.x * kLimitEnvs + (int)(threadIdx.x / kLimitLanes);
  const bool valid = env < N;
  bool trunc = false;
  int len = 0;
  if (valid) {
    len = met.episode_lengths[env];
    const bool ended = done[env] != 0;  // (its lengths are zero already: an environment that fell in this very step is a termination)
    trunc = !ended && len >= c.length;
    // the staggered first limit: still in the first episode since the reset, at the length drawn for this environment
    if (c.stagger && !ended && !trunc && (unsigned)len == limit_first(c, (unsigned)env)) trunc = met.timestep[env] == len;
    if (g == 0) truncated[env] = trunc ? 1 : 0;
  }
  if (!wave_any(trunc)) return;
  if (!trunc) return;
  if (g == 0) {  // what the step kernel's epilogue writes under `done` (reward and timestep stay)
    done[env] = 1;
    met.returned_episode_returns[env] = met.episode_returns[env];
    met.returned_episode_lengths[env] = len;
    met.returned_episode[env] = 1;
    met.episode_returns[env] = 0.f;
    met.episode_lengths[env] = 0;
  }
  float* recw = state + (size_t)env * rec_dim;
  float* obsw = obs ? obs + (size_t)env * obs_ld : nullptr;
  constexpr int kChunk = 4;  // (the loads of a chunk are all requested before the first store)
  for (int i0 = g; i0 < rec_dim; i0 += kLimitLanes * kChunk) {
    float rst[kChunk];
#pragma unroll
    for (int u = 0; u < kChunk; ++u) { const int i = i0 + kLimitLanes * u; rst[u] = reset_rec[i < rec_dim ? i : rec_dim - 1]; }
#pragma unroll
    for (int u = 0; u < kChunk; ++u) {
      const int i = i0 + kLimitLanes * u;
      if (i < rec_dim) { recw[i] = rst[u]; if (obsw && i < OP) obsw[i] = rst[u]; }
    }
  }
}

constexpr int kLimitEvalThreads = 256;

__global__ void __launch_bounds__(kLimitEvalThreads) eval_limit_count_kernel(int N, int first, const unsigned char* __restrict__ done,
                                                                             const unsigned char* __restrict__ truncated, long long* __restrict__ acc) {
  const int n = blockIdx.x * kLimitEvalThreads + threadIdx.x;
  if (n >= N) return;
  long long tr = 0, term = 0;
  if (!first) { tr = acc[n]; term = acc[(size_t)N + n]; }
  const bool u = truncated[n] != 0;
  tr += u ? 1 : 0;
  term += (done[n] != 0 && !u) ? 1 : 0;
  acc[n] = tr; acc[(size_t)N + n] = term;
}

__global__ void __launch_bounds__(kLimitEvalThreads) eval_limit_reduce_kernel(int N, const long long* __restrict__ acc, mppo_eval_limit_result_t* __restrict__ out) {
  __shared__ long long part[kLimitEvalThreads][2];
  long long tr = 0, fallen = 0;
  for (int n = threadIdx.x; n < N; n += kLimitEvalThreads) {  // a fixed stride in a fixed order (integers: any order gives the same sums)
    tr += acc[n];
    fallen += acc[(size_t)N + n] > 0 ? 1 : 0;
  }
  part[threadIdx.x][0] = tr; part[threadIdx.x][1] = fallen;
  __syncthreads();
  for (int s = kLimitEvalThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) { part[threadIdx.x][0] += part[threadIdx.x + s][0]; part[threadIdx.x][1] += part[threadIdx.x + s][1]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out->truncated_episodes = part[0][0]; out->fallen_envs = part[0][1]; }
}

int32_t check_limit_cfg(const char* who, const mppo_time_limit_cfg_t* c) {
  MPPO_REQUIRE(c, "%s: null time-limit configuration", who);
  MPPO_REQUIRE(c->length >= 0, "%s: episode length %d is negative", who, c->length);
  MPPO_REQUIRE(c->rank >= 0 && c->rank < 256, "%s: rank %d (0 .. 255)", who, c->rank);
  return MPPO_OK;
}

LimitCfg limit_cfg_of(const mppo_time_limit_cfg_t& c) {
  LimitCfg l{};
  l.length = c.length; l.stagger = c.stagger != 0 ? 1 : 0; l.seed = c.seed; l.stream = kStreamLimit + ((unsigned long long)c.rank << 16);
  return l;
}

int32_t time_limit_launch(const LimitCfg& c, int N, int rec_dim, int OP, float* state, const float* reset_rec, float* obs, int obs_ld, unsigned char* done,
                          unsigned char* truncated, const mppo_env_metrics_t& met, hipStream_t stream) {
  hipLaunchKernelGGL(time_limit_kernel, dim3(cdiv(N, kLimitEnvs)), dim3(kLimitThreads), 0, stream, c, N, rec_dim, OP, state, reset_rec, obs, obs_ld, done, truncated, met);
  MPPO_CHECK_LAUNCH("time_limit_kernel");
  return MPPO_OK;
}

int32_t eval_limit_count_launch(int N, bool first, const unsigned char* done, const unsigned char* truncated, void* acc, hipStream_t stream) {
  hipLaunchKernelGGL(eval_limit_count_kernel, dim3(cdiv(N, kLimitEvalThreads)), dim3(kLimitEvalThreads), 0, stream, N, first ? 1 : 0, done, truncated,
                     static_cast<long long*>(acc));
  MPPO_CHECK_LAUNCH("eval_limit_count_kernel");
  return MPPO_OK;
}

int32_t eval_limit_reduce_launch(int N, const void* acc, mppo_eval_limit_result_t* result, hipStream_t stream) {
  hipLaunchKernelGGL(eval_limit_reduce_kernel, dim3(1), dim3(kLimitEvalThreads), 0, stream, N, static_cast<const long long*>(acc), result);
  MPPO_CHECK_LAUNCH("eval_limit_reduce_kernel");
  return MPPO_OK;
}

}  // namespace mppo

using namespace mppo;

extern "C" int32_t mppo_env_time_limit(const mppo_model_t* m, int32_t N, const mppo_time_limit_cfg_t* cfg, float* state, const float* reset_rec, float* obs, int32_t obs_ld,
                                       uint8_t* done, uint8_t* truncated, const mppo_env_metrics_t* metrics, void* stream) {
  MPPO_REQUIRE(m && state && reset_rec && done && truncated && metrics, "mppo_env_time_limit: null model / state / reset_rec / done / truncated / metrics");
  MPPO_REQUIRE(N >= 1, "mppo_env_time_limit: N = %d", N);
  MPPO_TRY(check_limit_cfg("mppo_env_time_limit", cfg));
  MPPO_REQUIRE(cfg->length >= 1, "mppo_env_time_limit: episode length 0 is \"no limit\" - there is nothing to launch");
  MPPO_REQUIRE(metrics->episode_returns && metrics->episode_lengths && metrics->returned_episode_returns && metrics->returned_episode_lengths && metrics->returned_episode,
               "mppo_env_time_limit: the metrics need episode_returns, episode_lengths, returned_episode_returns, returned_episode_lengths and returned_episode");
  MPPO_REQUIRE(!cfg->stagger || metrics->timestep, "mppo_env_time_limit: a staggered limit reads metrics->timestep");
  const ModelView& mv = model_view(m);
  MPPO_REQUIRE(!obs || obs_ld >= mv.obs_pad, "mppo_env_time_limit: obs_ld %d < padded observation width %d", obs_ld, mv.obs_pad);
  return time_limit_launch(limit_cfg_of(*cfg), N, mv.rec_dim, mv.obs_pad, state, reset_rec, obs, obs_ld, done, truncated, *metrics, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mppo_eval_limit_count(int32_t N, int32_t first, const uint8_t* done, const uint8_t* truncated, void* acc, void* stream) {
  MPPO_REQUIRE(N >= 1, "mppo_eval_limit_count: N = %d", N);
  MPPO_REQUIRE(done && truncated && acc, "mppo_eval_limit_count: null done / truncated / accumulators");
  MPPO_REQUIRE((reinterpret_cast<uintptr_t>(acc) & 7) == 0, "mppo_eval_limit_count: the accumulators must be 8-byte aligned");
  return eval_limit_count_launch(N, first != 0, done, truncated, acc, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mppo_eval_limit_reduce(int32_t N, const void* acc, mppo_eval_limit_result_t* result, void* stream) {
  MPPO_REQUIRE(N >= 1, "mppo_eval_limit_reduce: N = %d", N);
  MPPO_REQUIRE(acc && result, "mppo_eval_limit_reduce: null accumulators / result");
  MPPO_REQUIRE((reinterpret_cast<uintptr_t>(acc) & 7) == 0 && (reinterpret_cast<uintptr_t>(result) & 7) == 0, "mppo_eval_limit_reduce: accumulators and result must be 8-byte aligned");
  return eval_limit_reduce_launch(N, acc, result, static_cast<hipStream_t>(stream));
}
