// env_launch.h - the model handle's launch helpers (env_model.hip): what the engine, the evaluator and the stages that take a model call to enqueue the environment
// kernel with the out-of-LDS matrices in a region of their own (`ws`; null: the handle's own allocation, grown on demand - not inside a stream capture).
#pragma once
#include "model_view.h"
#include "mppo_common.h"
#include "push.h"
#include "domrand.h"

namespace mppo {

const ModelView& model_view(const mppo_model* m);
// bytes of global memory the environment kernel needs beside the state for N environments (0 for a robot whose matrices fit LDS)
size_t model_scratch_bytes(const mppo_model* m, int N);

int32_t env_reset_ws(const mppo_model_t* m, int32_t N, float* state, float* reset_rec, float* obs, int32_t obs_ld, float* reward, uint8_t* done, const mppo_env_metrics_t* metrics,
                     float* ws, size_t ws_bytes, hipStream_t stream, const EnvDomain& dom);
// the reset from randomised states over the environments `mask` names (null: all of them); event = (*counter) * counter_mul + counter_add (counter null: 0)
int32_t env_reinit_ws(const mppo_model_t* m, int32_t N, float* state, float* obs, int32_t obs_ld, const uint8_t* mask, float scale, int32_t rng_impl, uint64_t seed,
                      int32_t rank, const uint32_t* key2, const int32_t* counter, int32_t counter_mul, int32_t counter_add, float* ws, size_t ws_bytes, hipStream_t stream,
                      const EnvDomain& dom);
// the step: under an external wrench (push.xfrc given, or drawn in the kernel when push.draw.force > 0; EnvPush{}: the unpushed step) and a randomisation table
// (EnvDomain{}: none - the launch runs the kernels it always ran)
int32_t env_step_push_ws(const mppo_model_t* m, int32_t N, int32_t n_frames, const mppo_reward_cfg_t* rc, float* state, const float* reset_rec, const float* action,
                         int32_t act_ld, float* obs, int32_t obs_ld, float* reward, uint8_t* done, const mppo_env_metrics_t* metrics, const EnvPush& push, float* ws,
                         size_t ws_bytes, hipStream_t stream, const EnvDomain& dom);

}  // namespace mppo
