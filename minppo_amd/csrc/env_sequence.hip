// env_sequence.hip - the environment's launch sequences (env_sequence.h): the ORDER of the optional stages around a reset and a step, decided once for the engine's
// rollout and the evaluator, which must agree bit for bit (tests/test_evaluate.py and the options' tests hold them to it).  Launches only - no allocation, no
// synchronisation, no blocking copy: both sequences can be captured into a hipGraph.  An option that is off adds no launch and changes no argument.
#include "env_sequence.h"

namespace mppo {

int32_t env_sequence_reset(const EnvRun& r, const EnvStep& b, hipStream_t s) {
  const ModelView& mv = model_view(r.model);
  // the plain reset makes the noise-free reset record and the zeroed metrics (train.py:142-144); reward / done are the step's to write
  MPPO_TRY(env_reset_ws(r.model, r.N, r.state, r.reset_rec, b.obs, b.obs_ld, b.reward, b.done, &r.met, r.ws, r.ws_bytes, s, r.domain));
  // reset noise: every environment then starts from a state of its own - event 0 of the Philox stream, the reset key for threefry (no counter word: the event is 0)
  if (r.reset_noise > 0.f)
    MPPO_TRY(env_reinit_ws(r.model, r.N, r.state, b.obs, b.obs_ld, nullptr, r.reset_noise, r.rng_impl, r.seed, r.rank, b.reset_key, nullptr, 0, 0, r.ws, r.ws_bytes, s, r.domain));
  // sensor noise: the row the reset wrote is step 0 of the noise's stream (the state records stay exact); it stays raw under observation normalisation
  if (r.obs_noise) MPPO_TRY(obs_noise_launch(r.noise_draw, r.N, mv.obs_dim, b.obs, b.obs_ld, r.obs_noise_scale, nullptr, 0, 0, s));
  // actuation latency: an empty ring, and the table of every environment's latency (a function of seed and rank: a resumed run has the same robots)
  if (r.delay.dmax > 0) {
    MPPO_CHECK_HIP(hipMemsetAsync(r.action_hist, 0, (size_t)kMaxActionDelay * r.N * mv.nu * 4, s));
    MPPO_TRY(action_delay_fill_launch(r.delay, r.N, r.action_delay, s));
  }
  return MPPO_OK;
}

int32_t env_sequence_step(const EnvRun& r, const EnvStep& b, hipStream_t s) {
  const ModelView& mv = model_view(r.model);
  const int N = r.N, A = mv.nu, O = mv.obs_dim;
  // actuation latency: the policy's action goes into the ring, the step is given the one its environment's latency ago (zeros at an episode's start); the caller's
  // trajectory keeps the policy's own action and log_prob - what PPO's ratio refers to.  Off: the step reads the policy's action as it always did
  const float* act = b.action;
  if (r.delay.dmax > 0) {
    MPPO_TRY(action_delay_launch(N, A, r.delay.dmax, r.action_delay, r.met.timestep, r.met.episode_lengths, b.action, A, r.action_hist, r.action_applied, A, s));
    act = r.action_applied;
  }
  // random pushes: the wrench of step (*counter) * mul + t is drawn inside the step's launch - a replayed graph draws fresh ones; off: the plain step (train.py:165)
  EnvPush push = r.push;
  push.ctr = r.counter; push.mul = r.counter_mul; push.add = b.t;
  MPPO_TRY(env_step_push_ws(r.model, N, r.n_frames, &r.rc, r.state, r.reset_rec, act, A, b.obs, b.obs_ld, b.reward, b.done, &r.met, push, r.ws, r.ws_bytes, s, r.domain));
  // episode time limit: the environments that have reached it are truncated - flags, metrics, the reset record - as the step's epilogue ends an episode;
  // `done` then includes them, so the masked restart below takes them too
  if (r.limit.length > 0)
    MPPO_TRY(time_limit_launch(r.limit, N, mv.rec_dim, mv.obs_pad, r.state, r.reset_rec, b.obs, b.obs_ld, b.done, b.truncated, r.met, s));
  // reset noise: the environments whose episode ended at this step restart from a randomised state (event ... + 1 + t) instead of the constant record the step
  // kernel gave them (env.py:166,179-180) - one masked launch of the reset kernel over `done`; a workgroup without an ended episode leaves at once.
  // Domain randomisation forces the launch, at scale 0 when reset noise is off: the one shared reset record is another robot's, so every restart goes through the
  // reset kernel with the environment's own row
  if (r.reset_noise > 0.f || r.domain.table)
    MPPO_TRY(env_reinit_ws(r.model, N, r.state, b.obs, b.obs_ld, b.done, r.reset_noise, r.rng_impl, r.seed, r.rank, b.reset_key, r.counter, r.counter_mul, 1 + b.t, r.ws,
                           r.ws_bytes, s, r.domain));
  // sensor noise BEHIND the restart, so that restarted environments' rows get it too: the noise of step ... + t + 1 (0 is the reset's).  What is stored is what the
  // next forward, the critic's bootstrap, the learn phase and the normalisation's statistics read
  if (r.obs_noise) MPPO_TRY(obs_noise_launch(r.noise_draw, N, O, b.obs, b.obs_ld, r.obs_noise_scale, r.counter, r.counter_mul, b.t + 1, s));
  // observation normalisation LAST, so that its raw sums include the noise: the new rows are stored normalised with the run's table (the next forward and the learn
  // phase read them so); their raw values go into this step's partial sums first, where the caller collects them (the state rows are raw throughout)
  if (r.norm_table) MPPO_TRY(obs_norm_apply_launch(N, O, b.obs, b.obs_ld, r.norm_table, r.norm_ld, r.norm_clip, b.norm_partials, s));
  return MPPO_OK;
}

}  // namespace mppo
