// limit.h - the episode time limit: which environments are truncated after an env step (k_limit.hip applies it; the engine and the evaluator launch it behind
// every step when environment.episode_length > 0), and GAE's cut at a truncated sample (k_ppo.hip gae_truncated_kernel).  minppo_amd/jaxrng.py
// time_limit_first_philox restates the staggered first limit.
//
// After an env step, environment n is truncated iff its episode did not end in that step (done[n] == 0) and
//   episode_lengths[n] >= L                                                                      (the limit), or
//   stagger, timestep[n] == episode_lengths[n] and episode_lengths[n] == first_n                 (the shortened FIRST episode since the reset)
// with first_n = 1 + (w mod L), w = word 0 of philox(counter = {n, 0xFFFFFFFE, lo(S), hi(S)}, key = seed), S = "LIMIT" << 24 + (rank << 16).  Stateless: a function
// of (seed, rank, environment) alone - no word in the state record, nothing in a checkpoint.  uint32 arithmetic and one integer remainder: the host restatement is exact.
#pragma once
#include "mppo_common.h"
#include "philox.h"

namespace mppo {

constexpr unsigned long long kStreamLimit = 0x4C494D4954ull << 24;  // "LIMIT" (beside kStreamPush / kStreamReset / kStreamNoise / kStreamPerm)

struct LimitCfg {
  int length, stagger;              // L >= 1; stagger != 0: the first episode of environment n ends at first_n
  unsigned long long seed, stream;  // the key and the stream id (kStreamLimit + (rank << 16))
};

// the length of environment `env`'s first episode under stagger, 1 .. L
__host__ __device__ inline unsigned limit_first(const LimitCfg& c, unsigned env) {
  return 1u + philox4x32(env, 0xFFFFFFFEu, (unsigned)c.stream, (unsigned)(c.stream >> 32), (unsigned)c.seed, (unsigned)(c.seed >> 32)).x % (unsigned)c.length;
}

// k_limit.hip: the refusals every entry point with a time-limit configuration shares, the kernel's parameters of a configuration, the launch (rec_dim / OP: the
// model's record and padded observation widths), the evaluator's counting stage and its reduction
int32_t check_limit_cfg(const char* who, const mppo_time_limit_cfg_t* c);
LimitCfg limit_cfg_of(const mppo_time_limit_cfg_t& c);
int32_t time_limit_launch(const LimitCfg& c, int N, int rec_dim, int OP, float* state, const float* reset_rec, float* obs, int obs_ld, unsigned char* done,
                          unsigned char* truncated, const mppo_env_metrics_t& met, hipStream_t stream);
inline size_t eval_limit_acc_bytes(int N) { return (size_t)2 * (size_t)N * 8; }
int32_t eval_limit_count_launch(int N, bool first, const unsigned char* done, const unsigned char* truncated, void* acc, hipStream_t stream);
int32_t eval_limit_reduce_launch(int N, const void* acc, mppo_eval_limit_result_t* result, hipStream_t stream);
// k_ppo.hip, beside gae_kernel: GAE with the cut at truncated samples (truncated = null: gae_launch itself)
int32_t gae_truncated_launch(int T, int N, float gamma, float lam, const float* reward, const float* value, const unsigned char* done, const unsigned char* truncated,
                             const float* last_val, float* adv, float* target, hipStream_t stream);

}  // namespace mppo
