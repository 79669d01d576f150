// eval.h - the policy evaluator's statistics stages (k_eval.hip), shared with the evaluation loop (evaluator.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/minppo_hip.h"
#include "mppo_common.h"

namespace mppo {

// Per-environment accumulators: kEvalAccSlots arrays of N 8-byte words, slot-major (word n of slot k at acc[k * N + n]), one writer
// per word (the thread of environment n).  int64 slots, then double slots.
enum EvalAccSlot {
  kAccEpisodes = 0,  // int64  finished episodes
  kAccLenSum,        // int64  sum of their lengths
  kAccLenMin,        // int64  INT64_MAX while none has finished
  kAccLenMax,        // int64  0 while none has finished
  kAccRetSum,        // double sum of their returns
  kAccRetSumSq,      // double sum of the squares
  kAccRetMin,        // double +inf while none has finished
  kAccRetMax,        // double -inf while none has finished
  kAccRewardSum,     // double sum of every step's reward
  kAccRunningRet,    // double the environment's running episode_returns as of the last accumulated step
  kEvalAccSlots
};
inline size_t eval_acc_bytes(int N) { return (size_t)kEvalAccSlots * (size_t)N * 8; }

// One launch: the first cdiv(n_acc, 256) workgroups fold a step into the accumulators of environments 0 .. n_acc - 1 (n_acc = 0: none, the
// trajectory's frame 0), the rest copy one trajectory row [R][W], W = row_w + A + 2: state[n, 0:row_w] | action[n, 0:A] | reward[n] | done[n];
// action / reward / done may be null when n_acc = 0 (zeros in the row: frame 0); the accumulators read reward and the metrics, `done` is read by
// the row part only.  first: the accumulators are empty (they are written, not read).
int32_t eval_accumulate_launch(int n_acc, int N, bool first, const float* reward, const uint8_t* done, const mppo_env_metrics_t* met, void* acc, const float* state,
                               int state_ld, int row_w, const float* action, int act_ld, int A, int R, float* traj_row, hipStream_t stream);
int32_t eval_reduce_launch(int N, int K, const void* acc, mppo_eval_result_t* result, hipStream_t stream);
int32_t eval_zero_launch(float* p, size_t n, hipStream_t stream);

}  // namespace mppo
