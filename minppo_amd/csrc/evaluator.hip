// evaluator.hip - mppo_evaluate: K steps of N environments under a trained policy as ONE call, with episode statistics and an optional joint
// trajectory.  What it replaces in the reference: nothing - minppo/infer.py:22-27 raises NotImplementedError; the loop below is the rollout of
// train.py:150-179 without the learner, under the mean action (deterministic) or a sample of the engine's Philox stream.
//
// The sequence is a composition of the library's own entry points, so that a caller could write it themselves and get the same bits
// (tests/test_evaluate.py does): mppo_env_reset, [mppo_env_reinit], then per step [mppo_normal_fill], mppo_policy_forward, mppo_env_step,
// [mppo_env_time_limit], [mppo_env_reinit over done], and the two stages of k_eval.hip (under an episode time limit also the two of k_limit.hip).  The environment's part
// of it - the reset with what follows it, the step with its optional stages - is env_sequence.hip's, shared with the engine's rollout.  Launches only: no allocation,
// no synchronisation, no blocking copy - every buffer is a region of the caller's workspace (a large robot's out-of-LDS matrices included), so the call can be
// captured into a hipGraph.
#include "eval.h"
#include "env_sequence.h"
#include "ppo_layout.h"

namespace mppo {

// The workspace layouts, each the one before it plus regions behind: which one an entry point promises (its mppo_eval*_ws_bytes, by that name in the refusal)
enum EvalLayout { kEvalPlain, kEvalLimit, kEvalDomain, kEvalSensors };
static const char* const kEvalWsBytesName[] = {"mppo_eval_ws_bytes", "mppo_eval_limit_ws_bytes", "mppo_eval_domain_ws_bytes", "mppo_eval_sensors_ws_bytes"};

// What an entry point has beside the plain evaluation's arguments, in the order the entry points grew (each lists the members up to its last one); everything at
// its default: mppo_evaluate, launch for launch
struct EvalOptions {
  EvalLayout layout = kEvalPlain;
  const float* obs_table = nullptr;  // [2][O] mean32 | inv_std32 of a policy trained on normalised observations (device memory)
  float clip = 0.f;
  const mppo_push_cfg_t* push = nullptr;
  int32_t episode_length = 0;        // > 0: the time limit, and `extra` its result
  mppo_eval_limit_result_t* extra = nullptr;
  const mppo_domain_cfg_t* domain = nullptr;
  const float* noise_scale = nullptr;  // a HOST vector [O]
  const mppo_action_delay_cfg_t* delay = nullptr;
  float* traj_applied = nullptr;     // [K + 1][R][A] the applied actions under a latency (may be null)
};

struct EvalWs {
  float *state, *reset_rec, *obs, *action, *log_prob, *value, *noise, *reward, *fwd_ws, *env_ws;
  unsigned char* done;
  mppo_env_metrics_t met;
  void* acc;
  size_t env_ws_bytes, total;
  // behind mppo_eval_ws_bytes' regions (kEvalLimit): the time limit's flags and the two counters per environment
  unsigned char* truncated;
  void* limit_acc;
  // behind those (kEvalDomain): the domain randomisation's table [N][4]
  float* domain;
  // behind that (kEvalSensors): the latency's ring [D][N][A], D = kMaxActionDelay, the applied actions [N][A], the latency table [N], the noise's sigma [OP]
  float *action_hist, *action_applied, *obs_noise_scale;
  int* action_delay;
};

// the regions of the workspace, each on a 256-byte boundary (base = null: sizes only)
static EvalWs carve_eval(const mppo_model* m, const mppo_net_t& net, int N, unsigned char* base, EvalLayout layout) {
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
  if (layout >= kEvalLimit) { w.truncated = take(n); w.limit_acc = take(eval_limit_acc_bytes(N)); }
  if (layout >= kEvalDomain) w.domain = (float*)take(n * 16);
  if (layout >= kEvalSensors) {
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
  return check_net(who, *net, mv, "num_layers", "bf16 products need the fused kernels (two hidden layers, hidden size a multiple of 32 up to 256, at most 32 actuators)");
}

static size_t eval_ws_bytes(EvalLayout layout, const mppo_model_t* m, const mppo_net_t* net, const mppo_eval_cfg_t* cfg) {
  if (check_eval(kEvalWsBytesName[layout], m, net, cfg) != MPPO_OK) return 0;
  return carve_eval(m, *net, cfg->N, nullptr, layout).total;
}

// Every draw is rank 0's under the evaluation's seed at step t itself (no counter word); an option that is null or at its identity: the evaluation without it,
// launch for launch
static int32_t evaluate_impl(const char* who, const mppo_model_t* m, const mppo_net_t* net, const float* params, const mppo_eval_cfg_t* cfg, void* ws, size_t ws_bytes,
                             const EvalOptions& o, mppo_eval_result_t* result, float* traj, void* stream) {
  MPPO_TRY(check_eval(who, m, net, cfg));
  const mppo_eval_cfg_t& c = *cfg;
  EnvRun run;
  run.model = m; run.N = c.N; run.n_frames = c.n_frames; run.rc = c.reward;
  run.reset_noise = c.reset_noise_scale; run.seed = c.seed;
  // sensor noise (a HOST vector [O]; all zero: off) and actuation latency (0 / 0: off): the noise of step k's row at index k + 1 (0: the reset's), under
  // `deterministic` too
  MPPO_TRY(check_obs_noise_scale(who, o.noise_scale, net->O));
  if (o.noise_scale) for (int j = 0; j < net->O; ++j) run.obs_noise = run.obs_noise || o.noise_scale[j] > 0.f;
  mppo_obs_noise_cfg_t nc{};
  nc.seed = c.seed;
  run.noise_draw = obs_noise_draw_of(nc);
  if (o.delay) {
    mppo_action_delay_cfg_t dc = *o.delay;
    dc.rank = 0; dc.seed = c.seed;
    MPPO_TRY(check_action_delay_cfg(who, &dc));
    if (dc.max > 0) run.delay = delay_draw_of(dc);
  }
  // domain randomisation: the table is drawn once and every reset, step and re-initialisation launch reads it
  mppo_domain_cfg_t dc{};
  bool randomised = false;
  if (o.domain) {
    dc = *o.domain;
    dc.rank = 0; dc.seed = c.seed;
    randomised = domain_cfg_on(dc);
    MPPO_TRY(check_domain_cfg(who, randomised ? m : nullptr, &dc));
  }
  // episode time limit (0: none): no stagger (the unstaggered test does not read the seed)
  MPPO_REQUIRE(o.episode_length >= 0, "%s: episode length %d is negative", who, o.episode_length);
  MPPO_REQUIRE(o.episode_length == 0 || (o.extra && (reinterpret_cast<uintptr_t>(o.extra) & 7) == 0), "%s: the time limit's result must be given, 8-byte aligned", who);
  if (o.episode_length > 0) {
    mppo_time_limit_cfg_t lc{};
    lc.length = o.episode_length; lc.seed = c.seed;
    run.limit = limit_cfg_of(lc);
  }
  const bool limited = run.limit.length > 0;
  // random pushes (force 0: off): drawn inside the step's kernel
  if (o.push) {
    MPPO_TRY(check_push_cfg(who, o.push));
    if (o.push->force > 0.f) {
      MPPO_TRY(check_push_body(who, m, o.push->body));
      mppo_push_cfg_t pc = *o.push;
      pc.rank = 0; pc.seed = c.seed;  // (rank 0: within the stream id's eight bits whatever the configuration held)
      run.push.body = pc.body; run.push.draw = push_draw_of(pc);
    }
  }
  MPPO_REQUIRE(params && ws && result, "%s: null params / workspace / result", who);
  MPPO_REQUIRE(traj || c.record_envs == 0, "%s: null trajectory with record_envs = %d", who, c.record_envs);
  MPPO_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "%s: the workspace must be 256-byte aligned", who);
  MPPO_REQUIRE((reinterpret_cast<uintptr_t>(result) & 7) == 0, "%s: the result must be 8-byte aligned", who);
  MPPO_REQUIRE(o.clip >= 0.f, "%s: clip %g is negative (or not a number)", who, (double)o.clip);
  const int N = c.N, K = c.K, R = c.record_envs, A = net->A;
  const EvalWs w = carve_eval(m, *net, N, static_cast<unsigned char*>(ws), o.layout);
  MPPO_REQUIRE(ws_bytes >= w.total, "%s: workspace %zu < %zu bytes (%s)", who, ws_bytes, w.total, kEvalWsBytesName[o.layout]);
  run.state = w.state; run.reset_rec = w.reset_rec; run.met = w.met; run.ws = w.env_ws; run.ws_bytes = w.env_ws_bytes;
  if (randomised) run.domain = EnvDomain{w.domain, dc.mass_body};
  run.obs_noise_scale = w.obs_noise_scale;
  run.action_hist = w.action_hist; run.action_applied = w.action_applied; run.action_delay = w.action_delay;
  // the next forward reads what the policy was trained on; the observation after the reset stays raw, as in the engine (the state rows are raw throughout)
  run.norm_table = o.obs_table; run.norm_ld = net->O; run.norm_clip = o.clip;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const ModelView& mv = model_view(m);
  const int OP = mv.obs_pad, row_w = mv.nq + mv.nv;
  const size_t frame = (size_t)R * (row_w + A + 2);
  const FwdBufs fb = carve_fwd(*net, N, w.fwd_ws);
  // every step's rows are written in place: the one observation buffer, the step's reward / done / truncated
  EnvStep st;
  st.action = w.action; st.obs = w.obs; st.obs_ld = OP; st.reward = w.reward; st.done = w.done; st.truncated = w.truncated;

  if (randomised) MPPO_TRY(domain_fill_launch(dc, N, w.domain, s));
  if (run.obs_noise) {  // the sigma table into the workspace (pad columns 0; the one host-to-device copy of this call)
    MPPO_CHECK_HIP(hipMemsetAsync(w.obs_noise_scale, 0, (size_t)OP * 4, s));
    MPPO_CHECK_HIP(hipMemcpyAsync(w.obs_noise_scale, o.noise_scale, (size_t)net->O * 4, hipMemcpyHostToDevice, s));
  }
  MPPO_TRY(env_sequence_reset(run, st, s));
  const bool applied = run.delay.dmax > 0 && o.traj_applied && R > 0;
  // frame 0 of the applied actions' trajectory is zero as the action columns of frame 0 are
  if (applied) MPPO_CHECK_HIP(hipMemsetAsync(o.traj_applied, 0, (size_t)R * A * 4, s));
  if (c.deterministic) MPPO_TRY(eval_zero_launch(w.noise, (size_t)N * A, s));
  // frame 0: the initial states, the action / reward / done columns zero
  MPPO_TRY(eval_accumulate_launch(0, N, true, nullptr, nullptr, nullptr, nullptr, w.state, mv.rec_dim, row_w, nullptr, A, A, R, traj, s));
  for (int t = 0; t < K; ++t) {
    if (!c.deterministic) MPPO_TRY(normal_fill_ctr(c.seed, (unsigned long long)t, nullptr, (size_t)N * A, w.noise, s));
    MPPO_TRY(policy_forward(*net, params, N, w.obs, OP, fb, w.noise, w.action, w.log_prob, w.value, nullptr, s));
    st.t = t;
    MPPO_TRY(env_sequence_step(run, st, s));
    // what the step was given under a latency (nothing writes the buffer before the next step); the trajectory's action columns stay the policy's
    if (applied)  // (the first R rows of the dense [N][A] buffer: one contiguous block)
      MPPO_CHECK_HIP(hipMemcpyAsync(o.traj_applied + (size_t)(t + 1) * R * A, w.action_applied, (size_t)R * A * 4, hipMemcpyDeviceToDevice, s));
    MPPO_TRY(eval_accumulate_launch(N, N, t == 0, w.reward, w.done, &w.met, w.acc, w.state, mv.rec_dim, row_w, w.action, A, A, R,
                                    R > 0 ? traj + (size_t)(t + 1) * frame : nullptr, s));
    if (limited) MPPO_TRY(eval_limit_count_launch(N, t == 0, w.done, w.truncated, w.limit_acc, s));
  }
  if (limited) MPPO_TRY(eval_limit_reduce_launch(N, w.limit_acc, o.extra, s));
  return eval_reduce_launch(N, K, w.acc, result, s);
}

}  // namespace mppo

using namespace mppo;

extern "C" size_t mppo_eval_ws_bytes(const mppo_model_t* m, const mppo_net_t* net, const mppo_eval_cfg_t* cfg) { return eval_ws_bytes(kEvalPlain, m, net, cfg); }

extern "C" int32_t mppo_evaluate(const mppo_model_t* m, const mppo_net_t* net, const float* params, const mppo_eval_cfg_t* cfg, void* ws, size_t ws_bytes,
                                 mppo_eval_result_t* result, float* traj, void* stream) {
  return evaluate_impl("mppo_evaluate", m, net, params, cfg, ws, ws_bytes, EvalOptions{}, result, traj, stream);
}

extern "C" int32_t mppo_evaluate_obs_norm(const mppo_model_t* m, const mppo_net_t* net, const float* params, const mppo_eval_cfg_t* cfg, void* ws, size_t ws_bytes,
                                          const float* obs_table, float clip, mppo_eval_result_t* result, float* traj, void* stream) {
  return evaluate_impl("mppo_evaluate_obs_norm", m, net, params, cfg, ws, ws_bytes, EvalOptions{kEvalPlain, obs_table, clip}, result, traj, stream);
}

extern "C" int32_t mppo_evaluate_push(const mppo_model_t* m, const mppo_net_t* net, const float* params, const mppo_eval_cfg_t* cfg, void* ws, size_t ws_bytes,
                                      const float* obs_table, float clip, const mppo_push_cfg_t* push, mppo_eval_result_t* result, float* traj, void* stream) {
  return evaluate_impl("mppo_evaluate_push", m, net, params, cfg, ws, ws_bytes, EvalOptions{kEvalPlain, obs_table, clip, push}, result, traj, stream);
}

extern "C" size_t mppo_eval_limit_ws_bytes(const mppo_model_t* m, const mppo_net_t* net, const mppo_eval_cfg_t* cfg) { return eval_ws_bytes(kEvalLimit, m, net, cfg); }

extern "C" int32_t mppo_evaluate_limit(const mppo_model_t* m, const mppo_net_t* net, const float* params, const mppo_eval_cfg_t* cfg, void* ws, size_t ws_bytes,
                                       const float* obs_table, float clip, const mppo_push_cfg_t* push, int32_t episode_length, mppo_eval_result_t* result,
                                       mppo_eval_limit_result_t* extra, float* traj, void* stream) {
  const EvalOptions o{kEvalLimit, obs_table, clip, push, episode_length, extra};
  return evaluate_impl("mppo_evaluate_limit", m, net, params, cfg, ws, ws_bytes, o, result, traj, stream);
}

extern "C" size_t mppo_eval_domain_ws_bytes(const mppo_model_t* m, const mppo_net_t* net, const mppo_eval_cfg_t* cfg) { return eval_ws_bytes(kEvalDomain, m, net, cfg); }

extern "C" int32_t mppo_evaluate_domain(const mppo_model_t* m, const mppo_net_t* net, const float* params, const mppo_eval_cfg_t* cfg, void* ws, size_t ws_bytes,
                                        const float* obs_table, float clip, const mppo_push_cfg_t* push, int32_t episode_length, const mppo_domain_cfg_t* domain,
                                        mppo_eval_result_t* result, mppo_eval_limit_result_t* extra, float* traj, void* stream) {
  const EvalOptions o{kEvalDomain, obs_table, clip, push, episode_length, extra, domain};
  return evaluate_impl("mppo_evaluate_domain", m, net, params, cfg, ws, ws_bytes, o, result, traj, stream);
}

extern "C" size_t mppo_eval_sensors_ws_bytes(const mppo_model_t* m, const mppo_net_t* net, const mppo_eval_cfg_t* cfg) { return eval_ws_bytes(kEvalSensors, m, net, cfg); }

extern "C" int32_t mppo_evaluate_sensors(const mppo_model_t* m, const mppo_net_t* net, const float* params, const mppo_eval_cfg_t* cfg, void* ws, size_t ws_bytes,
                                         const float* obs_table, float clip, const mppo_push_cfg_t* push, int32_t episode_length, const mppo_domain_cfg_t* domain,
                                         const float* obs_noise_scale, const mppo_action_delay_cfg_t* delay, mppo_eval_result_t* result,
                                         mppo_eval_limit_result_t* extra, float* traj, float* traj_applied, void* stream) {
  const EvalOptions o{kEvalSensors, obs_table, clip, push, episode_length, extra, domain, obs_noise_scale, delay, traj_applied};
  return evaluate_impl("mppo_evaluate_sensors", m, net, params, cfg, ws, ws_bytes, o, result, traj, stream);
}
