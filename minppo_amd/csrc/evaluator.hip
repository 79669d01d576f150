// evaluator.hip - mppo_evaluate: K steps of N environments under a trained policy as ONE call, with episode statistics and an optional joint
// trajectory.  What it replaces in the reference: nothing - minppo/infer.py:22-27 raises NotImplementedError; the loop below is the rollout of
// train.py:150-179 without the learner, under the mean action (deterministic) or a sample of the engine's Philox stream.
//
// The sequence is a composition of the library's own entry points, so that a caller could write it themselves and get the same bits
// (tests/test_evaluate.py does): mppo_env_reset, [mppo_env_reinit], then per step [mppo_normal_fill], mppo_policy_forward, mppo_env_step,
// [mppo_env_time_limit], [mppo_env_reinit over done], and the two stages of k_eval.hip (under an episode time limit also the two of k_limit.hip).  Launches only: no allocation, no synchronisation, no blocking copy - every
// buffer is a region of the caller's workspace (a large robot's out-of-LDS matrices included), so the call can be captured into a hipGraph.
#include "eval.h"
#include "model_view.h"
#include "obsnorm.h"
#include "ppo_layout.h"
#include "push.h"
#include "limit.h"
#include "domrand.h"
#include "sensor.h"

namespace mppo {
const ModelView& model_view(const mppo_model* m);
size_t model_scratch_bytes(const mppo_model* m, int N);
int32_t env_step_ws(const mppo_model_t* m, int32_t N, int32_t n_frames, const mppo_reward_cfg_t* rc, float* state, const float* reset_rec, const float* action,
                    int32_t act_ld, float* obs, int32_t obs_ld, float* reward, uint8_t* done, const mppo_env_metrics_t* metrics, float* ws, size_t ws_bytes, hipStream_t stream);
int32_t env_reset_ws(const mppo_model_t* m, int32_t N, float* state, float* reset_rec, float* obs, int32_t obs_ld, float* reward, uint8_t* done, const mppo_env_metrics_t* metrics,
                     float* ws, size_t ws_bytes, hipStream_t stream, const EnvDomain& dom);
int32_t env_reinit_ws(const mppo_model_t* m, int32_t N, float* state, float* obs, int32_t obs_ld, const uint8_t* mask, float scale, int32_t rng_impl, uint64_t seed,
                      int32_t rank, const uint32_t* key2, const int32_t* counter, int32_t counter_mul, int32_t counter_add, float* ws, size_t ws_bytes, hipStream_t stream,
                      const EnvDomain& dom);

struct EvalWs {
  float *state, *reset_rec, *obs, *action, *log_prob, *value, *noise, *reward, *fwd_ws, *env_ws;
  unsigned char* done;
  mppo_env_metrics_t met;
  void* acc;
  size_t env_ws_bytes, total;
  // behind mppo_eval_ws_bytes' regions (carve_eval's `limit`): the time limit's flags and the two counters per environment
  unsigned char* truncated;
  void* limit_acc;
  // behind those (carve_eval's `domain`): the domain randomisation's table [N][4]
  float* domain;
  // behind that (carve_eval's `sensors`): the latency's ring [D][N][A], D = kMaxActionDelay, the applied actions [N][A], the latency table [N], the noise's sigma [OP]
  float *action_hist, *action_applied, *obs_noise_scale;
  int* action_delay;
};

// the regions of the workspace, each on a 256-byte boundary (base = null: sizes only)
static EvalWs carve_eval(const mppo_model* m, const mppo_net_t& net, int N, unsigned char* base, bool limit = false, bool domain = false, bool sensors = false) {
  const ModelView& mv = model_view(m);
  EvalWs w{};
  size_t off = 0;
  auto take = [&](size_t bytes) -> unsigned char* {
    off = align_up(off, 256);
    unsigned char* p = base ? base + off : nullptr;
    off += bytes;
    return p;
  };
  const size_t n = (size_t)N;
  w.state = (float*)take(n * mv.rec_dim * 4);
  w.reset_rec = (float*)take((size_t)mv.rec_dim * 4);
  w.obs = (float*)take(n * mv.obs_pad * 4);
  w.action = (float*)take(n * net.A * 4);
  w.log_prob = (float*)take(n * 4);
  w.value = (float*)take(n * 4);
  w.noise = (float*)take(n * net.A * 4);
  w.reward = (float*)take(n * 4);
  w.done = take(n);
  w.met.episode_returns = (float*)take(n * 4);
  w.met.episode_lengths = (int32_t*)take(n * 4);
  w.met.returned_episode_returns = (float*)take(n * 4);
  w.met.returned_episode_lengths = (int32_t*)take(n * 4);
  w.met.timestep = (int32_t*)take(n * 4);
  w.met.returned_episode = (uint8_t*)take(n);
  w.acc = take(eval_acc_bytes(N));
  w.fwd_ws = (float*)take(fwd_bufs_floats(net, N) * 4);
  w.env_ws_bytes = model_scratch_bytes(m, N);
  w.env_ws = w.env_ws_bytes ? (float*)take(w.env_ws_bytes) : nullptr;
  if (limit) { w.truncated = take(n); w.limit_acc = take(eval_limit_acc_bytes(N)); }
  if (domain) w.domain = (float*)take(n * 16);
  if (sensors) {
    w.action_hist = (float*)take((size_t)kMaxActionDelay * n * net.A * 4);
    w.action_applied = (float*)take(n * net.A * 4);
    w.action_delay = (int*)take(n * 4);
    w.obs_noise_scale = (float*)take((size_t)mv.obs_pad * 4);
  }
  w.total = align_up(off, 256);
  return w;
}

static int32_t check_eval(const char* who, const mppo_model_t* m, const mppo_net_t* net, const mppo_eval_cfg_t* c) {
  MPPO_REQUIRE(m && net && c, "%s: null model / net / cfg", who);
  MPPO_REQUIRE(c->N >= 1, "%s: N = %d environments", who, c->N);
  MPPO_REQUIRE(c->K >= 1, "%s: K = %d steps", who, c->K);
  MPPO_REQUIRE(c->n_frames >= 1, "%s: n_frames = %d", who, c->n_frames);
  MPPO_REQUIRE(c->record_envs >= 0 && c->record_envs <= c->N, "%s: record_envs = %d of N = %d environments", who, c->record_envs, c->N);
  MPPO_REQUIRE(c->reset_noise_scale >= 0.f, "%s: reset_noise_scale %g is negative (or not a number)", who, (double)c->reset_noise_scale);
  const ModelView& mv = model_view(m);
  MPPO_REQUIRE(mv.nq >= 3, "%s: the environment reads qpos[2] as the height (env.py:239); nq = %d", who, mv.nq);
  MPPO_REQUIRE(net->O == mv.obs_dim && net->OP == mv.obs_pad, "%s: net O/OP (%d/%d) do not match the model's observation (%d/%d)", who, net->O, net->OP, mv.obs_dim, mv.obs_pad);
  MPPO_REQUIRE(net->A == mv.nu, "%s: net A = %d but the model has %d actuators", who, net->A, mv.nu);
  MPPO_REQUIRE(net->A >= 1 && net->A <= 63 && net->H >= 4 && net->H % 4 == 0, "%s: unsupported A / H (1 <= A <= 63, H a multiple of 4)", who);
  MPPO_REQUIRE(net->num_layers >= 0 && net->num_layers <= kMaxHidden, "%s: num_layers = %d (1 .. %d hidden layers, 0 = 2)", who, net->num_layers, kMaxHidden);
  MPPO_REQUIRE(!net->bf16 || (net_layers(*net) == 2 && net->H % 32 == 0 && net->H <= 256 && net->A <= 32),
               "%s: bf16 products need the fused kernels (two hidden layers, hidden size a multiple of 32 up to 256, at most 32 actuators)", who);
  return MPPO_OK;
}

}  // namespace mppo

using namespace mppo;

extern "C" size_t mppo_eval_ws_bytes(const mppo_model_t* m, const mppo_net_t* net, const mppo_eval_cfg_t* cfg) {
  if (check_eval("mppo_eval_ws_bytes", m, net, cfg) != MPPO_OK) return 0;
  return carve_eval(m, *net, cfg->N, nullptr).total;
}

// obs_table (may be null: the plain evaluation, not one launch more): [2][O] mean32 | inv_std32 of a policy trained on normalised observations
static int32_t evaluate_impl(const char* who, const mppo_model_t* m, const mppo_net_t* net, const float* params, const mppo_eval_cfg_t* cfg, void* ws, size_t ws_bytes,
                             const float* obs_table, float clip, const mppo_push_cfg_t* push, mppo_eval_result_t* result, float* traj, void* stream,
                             bool limit_ws = false, int32_t episode_length = 0, mppo_eval_limit_result_t* extra = nullptr, bool domain_ws = false,
                             const mppo_domain_cfg_t* domain = nullptr, bool sensors_ws = false, const float* noise_scale = nullptr,
                             const mppo_action_delay_cfg_t* delay = nullptr, float* traj_applied = nullptr) {
  MPPO_TRY(check_eval(who, m, net, cfg));
  // sensor noise (a HOST vector [O]; null or all zero: the evaluation without it, launch for launch) and actuation latency (null or 0 / 0: likewise): rank 0 under
  // the evaluation's seed, the noise of step k's row at index k + 1 (0: the reset's), under `deterministic` too
  MPPO_TRY(check_obs_noise_scale(who, noise_scale, net->O));
  bool noisy_obs = false;
  if (noise_scale) for (int j = 0; j < net->O; ++j) noisy_obs = noisy_obs || noise_scale[j] > 0.f;
  mppo_obs_noise_cfg_t nc{};
  nc.seed = cfg->seed;
  const ObsNoiseDraw nd = obs_noise_draw_of(nc);
  DelayDraw dd{};
  if (delay) {
    mppo_action_delay_cfg_t dc = *delay;
    dc.rank = 0; dc.seed = cfg->seed;
    MPPO_TRY(check_action_delay_cfg(who, &dc));
    if (dc.max > 0) dd = delay_draw_of(dc);
  }
  const bool delayed = dd.dmax > 0;
  // domain randomisation (may be null, or every range at its identity: the evaluation without it, launch for launch): the table is drawn once, from the evaluation's
  // seed as rank 0, and every reset, step and re-initialisation launch reads it
  mppo_domain_cfg_t dc{};
  bool randomised = false;
  if (domain) {
    dc = *domain;
    dc.rank = 0; dc.seed = cfg->seed;
    randomised = domain_cfg_on(dc);
    MPPO_TRY(check_domain_cfg(who, randomised ? m : nullptr, &dc));
  }
  // episode time limit (0: none - launch for launch the evaluation without one): no stagger, rank 0, the evaluation's seed (which the unstaggered test does not read)
  MPPO_REQUIRE(episode_length >= 0, "%s: episode length %d is negative", who, episode_length);
  MPPO_REQUIRE(episode_length == 0 || (extra && (reinterpret_cast<uintptr_t>(extra) & 7) == 0), "%s: the time limit's result must be given, 8-byte aligned", who);
  LimitCfg lim{};
  if (episode_length > 0) {
    mppo_time_limit_cfg_t lc{};
    lc.length = episode_length; lc.seed = cfg->seed;
    lim = limit_cfg_of(lc);
  }
  // random pushes (may be null, or of force 0: the unpushed evaluation, launch for launch): drawn inside the step's kernel at step t of rank 0 under the evaluation's seed
  EnvPush ep{};
  if (push) {
    MPPO_TRY(check_push_cfg(who, push));
    if (push->force > 0.f) {
      MPPO_TRY(check_push_body(who, m, push->body));
      mppo_push_cfg_t pc = *push;
      pc.rank = 0; pc.seed = cfg->seed;  // (rank 0: within the stream id's eight bits whatever the configuration held)
      ep.body = pc.body; ep.draw = push_draw_of(pc); ep.mul = 0;
    }
  }
  MPPO_REQUIRE(params && ws && result, "%s: null params / workspace / result", who);
  MPPO_REQUIRE(traj || cfg->record_envs == 0, "%s: null trajectory with record_envs = %d", who, cfg->record_envs);
  MPPO_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "%s: the workspace must be 256-byte aligned", who);
  MPPO_REQUIRE((reinterpret_cast<uintptr_t>(result) & 7) == 0, "%s: the result must be 8-byte aligned", who);
  MPPO_REQUIRE(clip >= 0.f, "%s: clip %g is negative (or not a number)", who, (double)clip);
  const mppo_eval_cfg_t& c = *cfg;
  const int N = c.N, K = c.K, R = c.record_envs, A = net->A;
  const EvalWs w = carve_eval(m, *net, N, static_cast<unsigned char*>(ws), limit_ws, domain_ws, sensors_ws);
  MPPO_REQUIRE(ws_bytes >= w.total, "%s: workspace %zu < %zu bytes (%s)", who, ws_bytes, w.total,
               sensors_ws ? "mppo_eval_sensors_ws_bytes" : domain_ws ? "mppo_eval_domain_ws_bytes" : limit_ws ? "mppo_eval_limit_ws_bytes" : "mppo_eval_ws_bytes");
  const EnvDomain dom = randomised ? EnvDomain{w.domain, dc.mass_body} : EnvDomain{};
  hipStream_t s = static_cast<hipStream_t>(stream);
  const ModelView& mv = model_view(m);
  const int OP = mv.obs_pad, row_w = mv.nq + mv.nv;
  const size_t frame = (size_t)R * (row_w + A + 2);
  const bool noisy_reset = c.reset_noise_scale > 0.f;
  const FwdBufs fb = carve_fwd(*net, N, w.fwd_ws);

  if (randomised) MPPO_TRY(domain_fill_launch(dc, N, w.domain, s));
  // the reset zeroes the metrics; reward / done are the step's to write
  MPPO_TRY(env_reset_ws(m, N, w.state, w.reset_rec, w.obs, OP, w.reward, w.done, &w.met, w.env_ws, w.env_ws_bytes, s, dom));
  if (noisy_reset)  // event 0 of the reset noise's Philox stream: every environment starts from a state of its own
    MPPO_TRY(env_reinit_ws(m, N, w.state, w.obs, OP, nullptr, c.reset_noise_scale, 0, c.seed, 0, nullptr, nullptr, 1, 0, w.env_ws, w.env_ws_bytes, s, dom));
  if (noisy_obs) {  // the sigma table into the workspace (pad columns 0; the one host-to-device copy of this call), then the reset's row: step 0
    MPPO_CHECK_HIP(hipMemsetAsync(w.obs_noise_scale, 0, (size_t)OP * 4, s));
    MPPO_CHECK_HIP(hipMemcpyAsync(w.obs_noise_scale, noise_scale, (size_t)net->O * 4, hipMemcpyHostToDevice, s));
    MPPO_TRY(obs_noise_launch(nd, N, net->O, w.obs, OP, w.obs_noise_scale, nullptr, 0, 0, s));
  }
  if (delayed) {  // an empty ring, every environment's latency; frame 0 of the applied actions' trajectory is zero as the action columns of frame 0 are
    MPPO_CHECK_HIP(hipMemsetAsync(w.action_hist, 0, (size_t)kMaxActionDelay * N * A * 4, s));
    MPPO_TRY(action_delay_fill_launch(dd, N, w.action_delay, s));
    if (traj_applied && R > 0) MPPO_CHECK_HIP(hipMemsetAsync(traj_applied, 0, (size_t)R * A * 4, s));
  }
  if (c.deterministic) MPPO_TRY(eval_zero_launch(w.noise, (size_t)N * A, s));
  // frame 0: the initial states, the action / reward / done columns zero
  MPPO_TRY(eval_accumulate_launch(0, N, true, nullptr, nullptr, nullptr, nullptr, w.state, mv.rec_dim, row_w, nullptr, A, A, R, traj, s));
  for (int t = 0; t < K; ++t) {
    if (!c.deterministic) MPPO_TRY(normal_fill_ctr(c.seed, (unsigned long long)t, nullptr, (size_t)N * A, w.noise, s));
    MPPO_TRY(policy_forward(*net, params, N, w.obs, OP, fb, w.noise, w.action, w.log_prob, w.value, nullptr, s));
    ep.add = t;
    const float* act = w.action;
    if (delayed) {  // the step is given the action of its environment's latency ago; the trajectory's action columns stay the policy's
      MPPO_TRY(action_delay_launch(N, A, dd.dmax, w.action_delay, w.met.timestep, w.met.episode_lengths, w.action, A, w.action_hist, w.action_applied, A, s));
      act = w.action_applied;
      if (traj_applied && R > 0)  // (the first R rows of the dense [N][A] buffer: one contiguous block)
        MPPO_CHECK_HIP(hipMemcpyAsync(traj_applied + (size_t)(t + 1) * R * A, w.action_applied, (size_t)R * A * 4, hipMemcpyDeviceToDevice, s));
    }
    MPPO_TRY(env_step_push_ws(m, N, c.n_frames, &c.reward, w.state, w.reset_rec, act, A, w.obs, OP, w.reward, w.done, &w.met, ep, w.env_ws, w.env_ws_bytes, s, dom));
    if (lim.length > 0)  // the environments that have reached the limit are truncated: done, the metrics and the reset record as the step ends an episode
      MPPO_TRY(time_limit_launch(lim, N, mv.rec_dim, OP, w.state, w.reset_rec, w.obs, OP, w.done, w.truncated, w.met, s));
    // the environments whose episode ended restart from a randomised state (event t + 1), as in the engine's rollout; under domain randomisation every restart
    // goes through the reset kernel with the environment's own row (the one shared reset record is another robot's), at scale 0 without reset noise
    if (noisy_reset || randomised)
      MPPO_TRY(env_reinit_ws(m, N, w.state, w.obs, OP, w.done, c.reset_noise_scale, 0, c.seed, 0, nullptr, nullptr, 1, t + 1, w.env_ws, w.env_ws_bytes, s, dom));
    if (noisy_obs) MPPO_TRY(obs_noise_launch(nd, N, net->O, w.obs, OP, w.obs_noise_scale, nullptr, 0, t + 1, s));  // (restarted environments' rows included)
    if (obs_table)  // the next forward reads what the policy was trained on; the observation after the reset stays raw, as in the engine (the state rows are raw throughout)
      MPPO_TRY(obs_norm_apply_launch(N, net->O, w.obs, OP, obs_table, net->O, clip, nullptr, s));
    MPPO_TRY(eval_accumulate_launch(N, N, t == 0, w.reward, w.done, &w.met, w.acc, w.state, mv.rec_dim, row_w, w.action, A, A, R,
                                    R > 0 ? traj + (size_t)(t + 1) * frame : nullptr, s));
    if (lim.length > 0) MPPO_TRY(eval_limit_count_launch(N, t == 0, w.done, w.truncated, w.limit_acc, s));
  }
  if (lim.length > 0) MPPO_TRY(eval_limit_reduce_launch(N, w.limit_acc, extra, s));
  return eval_reduce_launch(N, K, w.acc, result, s);
}

extern "C" int32_t mppo_evaluate(const mppo_model_t* m, const mppo_net_t* net, const float* params, const mppo_eval_cfg_t* cfg, void* ws, size_t ws_bytes,
                                 mppo_eval_result_t* result, float* traj, void* stream) {
  return evaluate_impl("mppo_evaluate", m, net, params, cfg, ws, ws_bytes, nullptr, 0.f, nullptr, result, traj, stream);
}

extern "C" int32_t mppo_evaluate_obs_norm(const mppo_model_t* m, const mppo_net_t* net, const float* params, const mppo_eval_cfg_t* cfg, void* ws, size_t ws_bytes,
                                          const float* obs_table, float clip, mppo_eval_result_t* result, float* traj, void* stream) {
  return evaluate_impl("mppo_evaluate_obs_norm", m, net, params, cfg, ws, ws_bytes, obs_table, clip, nullptr, result, traj, stream);
}

extern "C" int32_t mppo_evaluate_push(const mppo_model_t* m, const mppo_net_t* net, const float* params, const mppo_eval_cfg_t* cfg, void* ws, size_t ws_bytes,
                                      const float* obs_table, float clip, const mppo_push_cfg_t* push, mppo_eval_result_t* result, float* traj, void* stream) {
  return evaluate_impl("mppo_evaluate_push", m, net, params, cfg, ws, ws_bytes, obs_table, clip, push, result, traj, stream);
}

extern "C" size_t mppo_eval_limit_ws_bytes(const mppo_model_t* m, const mppo_net_t* net, const mppo_eval_cfg_t* cfg) {
  if (check_eval("mppo_eval_limit_ws_bytes", m, net, cfg) != MPPO_OK) return 0;
  return carve_eval(m, *net, cfg->N, nullptr, true).total;
}

extern "C" int32_t mppo_evaluate_limit(const mppo_model_t* m, const mppo_net_t* net, const float* params, const mppo_eval_cfg_t* cfg, void* ws, size_t ws_bytes,
                                       const float* obs_table, float clip, const mppo_push_cfg_t* push, int32_t episode_length, mppo_eval_result_t* result,
                                       mppo_eval_limit_result_t* extra, float* traj, void* stream) {
  return evaluate_impl("mppo_evaluate_limit", m, net, params, cfg, ws, ws_bytes, obs_table, clip, push, result, traj, stream, true, episode_length, extra);
}

extern "C" size_t mppo_eval_domain_ws_bytes(const mppo_model_t* m, const mppo_net_t* net, const mppo_eval_cfg_t* cfg) {
  if (check_eval("mppo_eval_domain_ws_bytes", m, net, cfg) != MPPO_OK) return 0;
  return carve_eval(m, *net, cfg->N, nullptr, true, true).total;
}

extern "C" int32_t mppo_evaluate_domain(const mppo_model_t* m, const mppo_net_t* net, const float* params, const mppo_eval_cfg_t* cfg, void* ws, size_t ws_bytes,
                                        const float* obs_table, float clip, const mppo_push_cfg_t* push, int32_t episode_length, const mppo_domain_cfg_t* domain,
                                        mppo_eval_result_t* result, mppo_eval_limit_result_t* extra, float* traj, void* stream) {
  return evaluate_impl("mppo_evaluate_domain", m, net, params, cfg, ws, ws_bytes, obs_table, clip, push, result, traj, stream, true, episode_length, extra, true, domain);
}

extern "C" size_t mppo_eval_sensors_ws_bytes(const mppo_model_t* m, const mppo_net_t* net, const mppo_eval_cfg_t* cfg) {
  if (check_eval("mppo_eval_sensors_ws_bytes", m, net, cfg) != MPPO_OK) return 0;
  return carve_eval(m, *net, cfg->N, nullptr, true, true, true).total;
}

extern "C" int32_t mppo_evaluate_sensors(const mppo_model_t* m, const mppo_net_t* net, const float* params, const mppo_eval_cfg_t* cfg, void* ws, size_t ws_bytes,
                                         const float* obs_table, float clip, const mppo_push_cfg_t* push, int32_t episode_length, const mppo_domain_cfg_t* domain,
                                         const float* obs_noise_scale, const mppo_action_delay_cfg_t* delay, mppo_eval_result_t* result,
                                         mppo_eval_limit_result_t* extra, float* traj, float* traj_applied, void* stream) {
  return evaluate_impl("mppo_evaluate_sensors", m, net, params, cfg, ws, ws_bytes, obs_table, clip, push, result, traj, stream, true, episode_length, extra, true, domain,
                       true, obs_noise_scale, delay, traj_applied);
}
