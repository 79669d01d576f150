// push.h - random pushes: the draw of the external wrench an environment gets at an env step.  Shared by the environment kernel (k_physics.hip: drawn in
// the step's launch, no array) and the fill kernel (k_push.hip: the same draw written out as [N][6]); minppo_amd/jaxrng.py push_wrench_philox restates it.
//
// Stateless: a function of (seed, rank, environment, step) alone - no word in the state record, nothing in a checkpoint.  With S = "PUSH" << 24 + (rank << 16):
//   phase_n = word 0 of philox(counter = {n, 0xFFFFFFFF, lo(S), hi(S)}, key = seed) mod interval
//   environment n is pushed at step s iff (s + phase_n) mod interval < duration; its window is k = (s + phase_n) / interval  (both sums modulo 2^32)
//   fx, fy  = uniform_from_bits(word 0 / word 1 of philox({n, k, lo(S), hi(S)}, seed), -force, force);  fz = 0, torque = 0
// so every environment is pushed on `duration` of any `interval` consecutive steps, out of phase with its neighbours, by a horizontal force uniform on a
// square that stays what it is for the whole window (an auto-reset inside the window does not end it).  Only the multiply / add / clamp of uniform_from_bits
// and one integer remainder: the host restatement is exact.
#pragma once
#include "mppo_common.h"
#include "philox.h"
#include "threefry.h"

namespace mppo {

constexpr unsigned long long kStreamPush = 0x50555348ull << 24;  // "PUSH" (beside kStreamReset / kStreamNoise / kStreamPerm)

struct PushDraw {
  float force;                      // F > 0 (0: no draw)
  int interval, duration;           // I >= 1, 1 <= D <= I, in env steps
  unsigned long long seed, stream;  // the key and the stream id (kStreamPush + (rank << 16))
};

// the force (fx, fy) on environment `env` at step `step`; false (and exact zeros) when it is not pushed there
__host__ __device__ inline bool push_draw(const PushDraw& p, unsigned env, unsigned step, float* fx, float* fy) {
  const unsigned s0 = (unsigned)p.stream, s1 = (unsigned)(p.stream >> 32), k0 = (unsigned)p.seed, k1 = (unsigned)(p.seed >> 32);
  const unsigned I = (unsigned)p.interval;
  const unsigned phase = philox4x32(env, 0xFFFFFFFFu, s0, s1, k0, k1).x % I;
  const unsigned at = step + phase;
  *fx = 0.f; *fy = 0.f;
  if (at % I >= (unsigned)p.duration) return false;
  const U4 r = philox4x32(env, at / I, s0, s1, k0, k1);
  *fx = uniform_from_bits(r.x, -p.force, p.force);
  *fy = uniform_from_bits(r.y, -p.force, p.force);
  return true;
}

// what a step launch is told about its wrench (env_model.hip env_step_push_ws): given as an array, or drawn in the kernel at step (*ctr) * mul + add
struct EnvPush {
  int body;
  const float* xfrc;  // [N][6] device, force then torque; null: drawn (draw.force > 0) or none
  PushDraw draw;
  const int* ctr;     // a word in device memory (null: 0)
  int mul, add;
};

struct EnvDomain;  // domrand.h: the table of a randomised launch (table null: none)
// env_model.hip: the refusals every entry point with a push configuration shares, the draw's parameters of a configuration, the pushed step launch
int32_t check_push_cfg(const char* who, const mppo_push_cfg_t* p);
int32_t check_push_body(const char* who, const mppo_model_t* m, int32_t body);
PushDraw push_draw_of(const mppo_push_cfg_t& p);
int32_t env_step_push_ws(const mppo_model_t* m, int32_t N, int32_t n_frames, const mppo_reward_cfg_t* rc, float* state, const float* reset_rec, const float* action,
                         int32_t act_ld, float* obs, int32_t obs_ld, float* reward, uint8_t* done, const mppo_env_metrics_t* metrics, const EnvPush& push, float* ws,
                         size_t ws_bytes, hipStream_t stream, const EnvDomain& dom);
// k_push.hip: the draw written out, xfrc [N][6] of step (*ctr) * mul + add
int32_t push_fill_launch(const PushDraw& p, int N, const int* ctr, int mul, int add, float* xfrc, hipStream_t stream);

}  // namespace mppo
