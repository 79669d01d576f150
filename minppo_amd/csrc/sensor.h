// sensor.h - sensor noise and actuation latency: the draw of the noise an observation column gets at an env step, the draw of an environment's latency, and
// what the launches of k_sensor.hip are told.  Shared by the kernels (k_sensor.hip), the engine and the evaluator; minppo_amd/jaxrng.py obs_noise_philox and
// action_delays_philox restate the two draws.
//
// Observation noise.  Stateless: a function of (seed, rank, environment, step, column) alone.  With S = "ONOIS" << 24 + (rank << 16):
//   r = philox(counter = {n, s, lo(S) + (j >> 2), hi(S)}, key = seed);  w = word j & 3 of r
//   obs[n][j] <- obs[n][j] + uniform_from_bits(w, -sigma_j, sigma_j)                       (one float32 add)
// A column whose sigma_j is not above 0 is not written, the pad columns O .. OP - 1 never.  The low 16 bits of lo(S) are free for the block index j >> 2, so
// (O + 3) / 4 <= 65536.  s: 0 for the row a reset writes, u * T + t + 1 for the row of rollout step t of update u (the evaluator's step k: k + 1), read through
// the pushes' ctr / mul / add scheme (push.h): s = (*ctr) * mul + add modulo 2^32.
//
// Actuation latency.  Environment n has the latency d_n for the whole run - a function of (seed, rank, environment) alone.  With S = "DELAY" << 24 + (rank << 16):
//   d_n = min + word 0 of philox(counter = {n, 0xFFFFFFFC, lo(S), hi(S)}, key = seed) mod (max - min + 1)
// At the k-th step of an episode (k = episode_lengths[n] before the step) the environment is given the policy's action of step k - d_n of the same episode, zeros
// while k < d_n, and the very bits of the policy's action when d_n = 0.  The history is a ring [D][N][A], D = max, indexed by the environment's own timestep[n]
// (monotonic since the reset, in every checkpoint): slot timestep mod D is written, slot (timestep - d_n) mod D is read - by the same lane, the read first, so
// d_n = D reads what the slot held before this step's action replaces it.  uint32 arithmetic and integer remainders: the host restatements are exact.
#pragma once
#include "mppo_common.h"
#include "philox.h"
#include "threefry.h"

namespace mppo {

constexpr unsigned long long kStreamObsNoise = 0x4F4E4F4953ull << 24;  // "ONOIS" (beside kStreamDomain / kStreamLimit / kStreamPush / kStreamReset)
constexpr unsigned long long kStreamDelay = 0x44454C4159ull << 24;     // "DELAY"
constexpr unsigned kDelayCounter = 0xFFFFFFFCu;                         // word 1 of the counter (0xFFFFFFFD .. F: the domain's, the limit's, the pushes')
constexpr int kMaxActionDelay = 16;                                     // the deepest ring (the engine's region "action_hist" has that many slots)

struct ObsNoiseDraw {
  unsigned long long seed, stream;  // the key and the stream id (kStreamObsNoise + (rank << 16))
};

// the four words of block `blk` (columns 4 blk .. 4 blk + 3) of environment `env` at step `step`
__host__ __device__ inline U4 obs_noise_block(const ObsNoiseDraw& p, unsigned env, unsigned step, unsigned blk) {
  return philox4x32(env, step, (unsigned)p.stream + blk, (unsigned)(p.stream >> 32), (unsigned)p.seed, (unsigned)(p.seed >> 32));
}

struct DelayDraw {
  int dmin, dmax;                   // 0 <= dmin <= dmax <= kMaxActionDelay
  unsigned long long seed, stream;  // the key and the stream id (kStreamDelay + (rank << 16))
};

__host__ __device__ inline int delay_draw(const DelayDraw& p, unsigned env) {
  const unsigned w = philox4x32(env, kDelayCounter, (unsigned)p.stream, (unsigned)(p.stream >> 32), (unsigned)p.seed, (unsigned)(p.seed >> 32)).x;
  return p.dmin + (int)(w % (unsigned)(p.dmax - p.dmin + 1));
}

// k_sensor.hip: the refusals every entry point with one of the two configurations shares, the draws' parameters of a configuration, the launches
int32_t check_obs_noise_cfg(const char* who, const mppo_obs_noise_cfg_t* c);
int32_t check_obs_noise_scale(const char* who, const float* scale, int O);  // a HOST vector: no negative (or NaN) entry, (O + 3) / 4 <= 65536
int32_t check_action_delay_cfg(const char* who, const mppo_action_delay_cfg_t* c);
ObsNoiseDraw obs_noise_draw_of(const mppo_obs_noise_cfg_t& c);
DelayDraw delay_draw_of(const mppo_action_delay_cfg_t& c);
// sigma: [4 ceil(O / 4)] device floats (the pad entries are read, never used)
int32_t obs_noise_launch(const ObsNoiseDraw& p, int N, int O, float* obs, int obs_ld, const float* sigma, const int* ctr, int mul, int add, hipStream_t stream);
int32_t action_delay_fill_launch(const DelayDraw& p, int N, int* delay, hipStream_t stream);
int32_t action_delay_launch(int N, int A, int D, const int* delay, const int* timestep, const int* episode_lengths, const float* action, int act_ld, float* hist,
                            float* applied, int applied_ld, hipStream_t stream);

}  // namespace mppo
