// env_sequence.h - the environment's two launch sequences (env_sequence.hip): what follows a reset, and one step with every optional stage in its place.  The engine's
// rollout and reset (engine.hip) and the evaluator (evaluator.hip) enqueue their environments through these two functions and nothing else; what differs between
// the callers - whose counter drives the draws, where a step's rows go, whether the normalisation collects sums - is a value in the two structs below.
#pragma once
#include "env_launch.h"
#include "limit.h"
#include "obsnorm.h"
#include "sensor.h"

namespace mppo {

// What is fixed for a run: the environments' buffers, the identity of the draws, and every option (each at "off" as initialised: not one launch more)
struct EnvRun {
  const mppo_model_t* model = nullptr;
  int N = 0, n_frames = 1;
  mppo_reward_cfg_t rc{};
  float *state = nullptr, *reset_rec = nullptr;  // [N][rec_dim], [rec_dim]
  mppo_env_metrics_t met{};
  float* ws = nullptr;                           // the out-of-LDS matrices of a large robot (model_scratch_bytes; null: none needed)
  size_t ws_bytes = 0;
  // the draws that depend on the step read its index as (*counter) * counter_mul + add, `add` following from EnvStep::t (counter null: 0 - the index is `add`)
  const int* counter = nullptr;
  int counter_mul = 0;
  // reset noise (0: every environment restarts from the one constant reset record) and the stream it is drawn from
  float reset_noise = 0.f;
  int rng_impl = 0, rank = 0;
  uint64_t seed = 0;
  // random pushes (force 0: the unpushed step); ctr / mul / add are the sequence's to fill in
  EnvPush push{};
  // episode time limit (length 0: none)
  LimitCfg limit{};
  // domain randomisation (table null: none)
  EnvDomain domain{};
  // sensor noise: sigma [OP] device floats, pad columns 0
  bool obs_noise = false;
  ObsNoiseDraw noise_draw{};
  float* obs_noise_scale = nullptr;
  // actuation latency (dmax 0: off - the step reads EnvStep::action): the ring [kMaxActionDelay][N][A], what the step launch is given [N][A], the latency table [N]
  DelayDraw delay{};
  float *action_hist = nullptr, *action_applied = nullptr;
  int* action_delay = nullptr;
  // observation normalisation (table null: off): [2][norm_ld] mean32 | inv_std32
  const float* norm_table = nullptr;
  int norm_ld = 0;
  float norm_clip = 0.f;
};

// What changes from step to step (the reset reads obs, reward, done and reset_key alone)
struct EnvStep {
  const float* action = nullptr;         // [N][A] the policy's
  float* obs = nullptr;                  // [N][obs_ld] the rows this step (or the reset) writes
  int obs_ld = 0;
  float* reward = nullptr;               // [N]  (the reset: may be null)
  unsigned char* done = nullptr;         // [N]  (the reset: may be null)
  unsigned char* truncated = nullptr;    // [N]  under a time limit
  double* norm_partials = nullptr;       // the normalisation's sums of this step's raw rows (obs_norm_partial_doubles; null: not collected)
  const unsigned* reset_key = nullptr;   // the reset noise's threefry key of this step, two device words (null under Philox)
  int t = 0;                             // the step's index within its rollout
};

// env_reset_ws -> [reset noise, event 0] -> [sensor noise, step 0] -> [an empty latency ring, the latency table]
int32_t env_sequence_reset(const EnvRun& r, const EnvStep& b, hipStream_t stream);
// [latency] -> step -> [time limit] -> [restart of the ended episodes] -> [sensor noise] -> [normalisation]
int32_t env_sequence_step(const EnvRun& r, const EnvStep& b, hipStream_t stream);

}  // namespace mppo
