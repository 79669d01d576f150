// k_eval.hip - episode statistics and trajectory rows of a policy evaluation (mppo_evaluate, evaluator.hip).
//
// The reference has no evaluation loop (minppo/infer.py:22-27 raises NotImplementedError) and no time limit (env.py:238-242 ends an episode on
// height only), so a policy that stands never finishes an episode and `returned_episode_returns` goes stale exactly when training succeeds.  The
// evaluator therefore reports two things after K steps: the episodes that ended (count, return and length statistics) and the environments that
// never fell (`survivors`, with the returns they have collected so far).
//
//   eval_accumulate_kernel  once per step, after the env step (and its masked reinit): one thread per environment folds the env kernel's OWN
//                           bookkeeping (`EnvMetrics`, env.py:183-194: returned_episode, returned_episode_returns / _lengths, episode_returns - the
//                           returns are not re-derived) and the step's reward into per-environment accumulators; the workgroups behind those copy
//                           one trajectory row, one thread per element, coalesced along the row.  Every word has one writer: no atomics.
//   eval_reduce_kernel      once at the end, ONE workgroup: thread i walks environments i, i + 256, ... in that order, an LDS tree of fixed shape
//                           combines the threads, thread 0 writes the result.  Sums in double, counts in int64, min / max exact; nothing depends on
//                           the order in which waves arrive, so the result is bitwise reproducible from run to run.
//   eval_zero_kernel        the zero noise of a deterministic evaluation (`mean + exp(log_std) * 0` is the mean): a kernel, not a memset node, so
//                           that the sequence stays capturable.
#include "eval.h"

#include <cmath>
#include <limits>

namespace mppo {

constexpr int kEvalThreads = 256;

__global__ void __launch_bounds__(kEvalThreads) eval_accumulate_kernel(int n_acc, int acc_blocks, int N, int first, const float* __restrict__ reward,
                                                                       const unsigned char* __restrict__ done, mppo_env_metrics_t met, void* __restrict__ acc_v,
                                                                       const float* __restrict__ state, int state_ld, int row_w, const float* __restrict__ action,
                                                                       int act_ld, int A, int R, float* __restrict__ traj_row) {
  if ((int)blockIdx.x < acc_blocks) {
    const int n = blockIdx.x * kEvalThreads + threadIdx.x;
    if (n >= n_acc) return;
    long long* ai = static_cast<long long*>(acc_v);
    double* ad = static_cast<double*>(acc_v);
    const size_t S = (size_t)N;
    long long episodes = 0, len_sum = 0, len_min = std::numeric_limits<long long>::max(), len_max = 0;
    double ret_sum = 0.0, ret_sumsq = 0.0, ret_min = (double)INFINITY, ret_max = -(double)INFINITY, reward_sum = 0.0;
    if (!first) {
      episodes = ai[kAccEpisodes * S + n]; len_sum = ai[kAccLenSum * S + n]; len_min = ai[kAccLenMin * S + n]; len_max = ai[kAccLenMax * S + n];
      ret_sum = ad[kAccRetSum * S + n]; ret_sumsq = ad[kAccRetSumSq * S + n]; ret_min = ad[kAccRetMin * S + n]; ret_max = ad[kAccRetMax * S + n];
      reward_sum = ad[kAccRewardSum * S + n];
    }
    if (met.returned_episode[n] != 0) {  // an episode ended at this step: its return and length as the env kernel recorded them
      const double r = (double)met.returned_episode_returns[n];
      const long long l = (long long)met.returned_episode_lengths[n];
      episodes += 1; len_sum += l;
      len_min = l < len_min ? l : len_min; len_max = l > len_max ? l : len_max;
      ret_sum += r; ret_sumsq += r * r;  // (the square of a float is exact in double)
      ret_min = r < ret_min ? r : ret_min; ret_max = r > ret_max ? r : ret_max;
    }
    reward_sum += (double)reward[n];
    ai[kAccEpisodes * S + n] = episodes; ai[kAccLenSum * S + n] = len_sum; ai[kAccLenMin * S + n] = len_min; ai[kAccLenMax * S + n] = len_max;
    ad[kAccRetSum * S + n] = ret_sum; ad[kAccRetSumSq * S + n] = ret_sumsq; ad[kAccRetMin * S + n] = ret_min; ad[kAccRetMax * S + n] = ret_max;
    ad[kAccRewardSum * S + n] = reward_sum;
    ad[kAccRunningRet * S + n] = (double)met.episode_returns[n];
    return;
  }
  // one trajectory row: element e = n * W + c of [R][W]
  const int W = row_w + A + 2;
  const size_t e = (size_t)((int)blockIdx.x - acc_blocks) * kEvalThreads + threadIdx.x;
  if (e >= (size_t)R * W) return;
  const int n = (int)(e / W), c = (int)(e % W);
  float v;
  if (c < row_w) v = state[(size_t)n * state_ld + c];
  else if (c < row_w + A) v = action ? action[(size_t)n * act_ld + (c - row_w)] : 0.f;
  else if (c == row_w + A) v = reward ? reward[n] : 0.f;
  else v = (done && done[n] != 0) ? 1.f : 0.f;
  traj_row[e] = v;
}

struct EvalPartial {
  long long episodes, len_sum, len_min, len_max, survivors;
  double ret_sum, ret_sumsq, ret_min, ret_max, reward_sum, survivor_ret_sum;
};
__device__ __forceinline__ void eval_combine(EvalPartial& a, const EvalPartial& b) {
  a.episodes += b.episodes; a.len_sum += b.len_sum; a.survivors += b.survivors;
  a.len_min = b.len_min < a.len_min ? b.len_min : a.len_min; a.len_max = b.len_max > a.len_max ? b.len_max : a.len_max;
  a.ret_sum += b.ret_sum; a.ret_sumsq += b.ret_sumsq; a.reward_sum += b.reward_sum; a.survivor_ret_sum += b.survivor_ret_sum;
  a.ret_min = b.ret_min < a.ret_min ? b.ret_min : a.ret_min; a.ret_max = b.ret_max > a.ret_max ? b.ret_max : a.ret_max;
}

__global__ void __launch_bounds__(kEvalThreads) eval_reduce_kernel(int N, int K, const void* __restrict__ acc_v, mppo_eval_result_t* __restrict__ out) {
  __shared__ EvalPartial part[kEvalThreads];
  const long long* ai = static_cast<const long long*>(acc_v);
  const double* ad = static_cast<const double*>(acc_v);
  const size_t S = (size_t)N;
  EvalPartial p;
  p.episodes = 0; p.len_sum = 0; p.len_min = std::numeric_limits<long long>::max(); p.len_max = 0; p.survivors = 0;
  p.ret_sum = 0.0; p.ret_sumsq = 0.0; p.ret_min = (double)INFINITY; p.ret_max = -(double)INFINITY; p.reward_sum = 0.0; p.survivor_ret_sum = 0.0;
  for (int n = threadIdx.x; n < N; n += kEvalThreads) {  // a fixed stride in a fixed order
    EvalPartial q;
    q.episodes = ai[kAccEpisodes * S + n]; q.len_sum = ai[kAccLenSum * S + n]; q.len_min = ai[kAccLenMin * S + n]; q.len_max = ai[kAccLenMax * S + n];
    q.ret_sum = ad[kAccRetSum * S + n]; q.ret_sumsq = ad[kAccRetSumSq * S + n]; q.ret_min = ad[kAccRetMin * S + n]; q.ret_max = ad[kAccRetMax * S + n];
    q.reward_sum = ad[kAccRewardSum * S + n];
    const bool survivor = q.episodes == 0;  // no episode of this environment ended in K steps: its running return is all it has to show
    q.survivors = survivor ? 1 : 0;
    q.survivor_ret_sum = survivor ? ad[kAccRunningRet * S + n] : 0.0;
    eval_combine(p, q);
  }
  part[threadIdx.x] = p;
  __syncthreads();
  for (int s = kEvalThreads / 2; s > 0; s >>= 1) {  // the tree's shape depends on nothing but kEvalThreads
    if ((int)threadIdx.x < s) {
      EvalPartial a = part[threadIdx.x];
      eval_combine(a, part[threadIdx.x + s]);
      part[threadIdx.x] = a;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const EvalPartial r = part[0];
    out->episodes = r.episodes; out->len_sum = r.len_sum;
    out->len_min = r.episodes > 0 ? r.len_min : 0; out->len_max = r.len_max;
    out->survivors = r.survivors; out->steps = (long long)K * (long long)N;
    out->ret_sum = r.ret_sum; out->ret_sumsq = r.ret_sumsq; out->ret_min = r.ret_min; out->ret_max = r.ret_max;
    out->survivor_ret_sum = r.survivor_ret_sum; out->reward_sum = r.reward_sum;
  }
}

__global__ void __launch_bounds__(kEvalThreads) eval_zero_kernel(float* __restrict__ p, size_t n) {
  const size_t i = (size_t)blockIdx.x * kEvalThreads + threadIdx.x;
  if (i < n) p[i] = 0.f;
}

int32_t eval_accumulate_launch(int n_acc, int N, bool first, const float* reward, const uint8_t* done, const mppo_env_metrics_t* met, void* acc, const float* state,
                               int state_ld, int row_w, const float* action, int act_ld, int A, int R, float* traj_row, hipStream_t stream) {
  const int acc_blocks = n_acc > 0 ? cdiv(n_acc, kEvalThreads) : 0;
  const int row_blocks = R > 0 ? cdiv((long)R * (row_w + A + 2), kEvalThreads) : 0;
  if (acc_blocks + row_blocks == 0) return MPPO_OK;
  mppo_env_metrics_t mm{};
  if (met) mm = *met;
  hipLaunchKernelGGL(eval_accumulate_kernel, dim3(acc_blocks + row_blocks), dim3(kEvalThreads), 0, stream, n_acc, acc_blocks, N, first ? 1 : 0, reward, done, mm, acc, state,
                     state_ld, row_w, action, act_ld, A, R, traj_row);
  MPPO_CHECK_LAUNCH("eval_accumulate_kernel");
  return MPPO_OK;
}

int32_t eval_reduce_launch(int N, int K, const void* acc, mppo_eval_result_t* result, hipStream_t stream) {
  hipLaunchKernelGGL(eval_reduce_kernel, dim3(1), dim3(kEvalThreads), 0, stream, N, K, acc, result);
  MPPO_CHECK_LAUNCH("eval_reduce_kernel");
  return MPPO_OK;
}

int32_t eval_zero_launch(float* p, size_t n, hipStream_t stream) {
  hipLaunchKernelGGL(eval_zero_kernel, dim3(cdiv((long)n, kEvalThreads)), dim3(kEvalThreads), 0, stream, p, n);
  MPPO_CHECK_LAUNCH("eval_zero_kernel");
  return MPPO_OK;
}

}  // namespace mppo

using namespace mppo;

extern "C" int32_t mppo_eval_accumulate(int32_t N, int32_t first, const float* reward, const uint8_t* done, const mppo_env_metrics_t* metrics, void* acc,
                                        const float* state, int32_t state_ld, int32_t row_w, const float* action, int32_t act_ld, int32_t A, int32_t R,
                                        float* traj_row, void* stream) {
  MPPO_REQUIRE(N >= 1, "mppo_eval_accumulate: N = %d", N);
  MPPO_REQUIRE(reward && acc && metrics, "mppo_eval_accumulate: null reward / metrics / accumulators");
  MPPO_REQUIRE(metrics->returned_episode && metrics->returned_episode_returns && metrics->returned_episode_lengths && metrics->episode_returns,
               "mppo_eval_accumulate: the metrics need returned_episode, returned_episode_returns, returned_episode_lengths and episode_returns");
  MPPO_REQUIRE((reinterpret_cast<uintptr_t>(acc) & 7) == 0, "mppo_eval_accumulate: the accumulators must be 8-byte aligned");
  MPPO_REQUIRE(R >= 0 && R <= N, "mppo_eval_accumulate: %d recorded environments of %d", R, N);
  if (R > 0) {
    MPPO_REQUIRE(traj_row && state && done, "mppo_eval_accumulate: null trajectory row / state / done with %d recorded environments", R);
    MPPO_REQUIRE(row_w >= 0 && A >= 0 && state_ld >= row_w && (A == 0 || !action || act_ld >= A), "mppo_eval_accumulate: row_w %d / state_ld %d / A %d / act_ld %d",
                 row_w, state_ld, A, act_ld);
  }
  return eval_accumulate_launch(N, N, first != 0, reward, done, metrics, acc, state, state_ld, row_w, action, act_ld, A, R, traj_row, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mppo_eval_reduce(int32_t N, int32_t K, const void* acc, mppo_eval_result_t* result, void* stream) {
  MPPO_REQUIRE(N >= 1 && K >= 0, "mppo_eval_reduce: N = %d, K = %d", N, K);
  MPPO_REQUIRE(acc && result, "mppo_eval_reduce: null accumulators / result");
  MPPO_REQUIRE((reinterpret_cast<uintptr_t>(acc) & 7) == 0 && (reinterpret_cast<uintptr_t>(result) & 7) == 0, "mppo_eval_reduce: accumulators and result must be 8-byte aligned");
  return eval_reduce_launch(N, K, acc, result, static_cast<hipStream_t>(stream));
}
