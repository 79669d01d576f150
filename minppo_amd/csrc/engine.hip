// engine.hip — one PPO `_update_step` (reference minppo/train.py:146-283) as a single C call.
//
// The reference is ONE jitted XLA program; here the same dependency chain is a fixed sequence of
// kernel launches enqueued from C++ on the caller's stream (about 1.3k launches per update at the
// default 4 epochs x 32 minibatches), optionally captured once into a hipGraph and replayed, so
// that Python is out of the loop.  All buffers live in one caller-owned HBM arena whose layout is
// fixed at creation time (so the captured graph stays valid; with several ranks the RCCL calls are captured too); dynamic quantities the graph must
// not bake in (Adam step index, RNG stream position) live in the arena's `count` words and are
// advanced by a kernel at the end of every update.
//
// Multi-GPU (one process per GPU): environments shard across ranks, parameters are replicated.
// Per optimizer step the flat gradient [P] is sum-all-reduced with RCCL on the same stream; per
// update the [E*M*2] float64 advantage sums are all-reduced once, so that every rank normalises
// with the statistics of the global minibatch.  Rows are weighted 1/(mb*world).
#include <wave_ops.h>

#include "mppo_common.h"
#include "model_view.h"
#include "ppo_layout.h"
#include "platform.h"
#include "peer.h"
#include "obsnorm.h"
#include "rewnorm.h"
#include "push.h"
#include "domrand.h"
#include "limit.h"
#include "sensor.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

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

// end of an update: the Adam step index and the update index move on; `zero` (optional): words another kernel of the update wants back
// at zero before its next use (the bucket counters of the two-launch permutation, k_perm.hip).  The LAST of those words is that form's
// overflow mark (a bucket received more values than it has slots: the epoch's index array is then not a permutation); before it is zeroed
// it is made sticky in count[3], which the host reads at its next synchronisation (Trainer.check_status): an update that trained on a
// spoilt permutation never passes silently (round-4 advisor; unreachable short of a 22-sigma event for B <= 131072, but no longer unguarded)
__global__ void advance_counters_kernel(int* count, int opt_steps, int* zero = nullptr, int nzero = 0) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    if (opt_steps > 0) { count[0] += opt_steps; count[1] += 1; }
    if (nzero > 0 && zero[nzero - 1] != 0) count[3] = 1;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nzero; i += blockDim.x) zero[i] = 0;
}

// Per-update rollout statistics: the device-side reduction of what the reference returns as the full [T,N] history of
// `EnvMetrics` (env.py:183-194 -> Memory.info, train.py:170,283).  One workgroup of 1024 threads; thread n walks its
// environments through the T steps, replaying the episode bookkeeping of env.py:183-190 from the rollout's own reward /
// done arrays (carry-in = the environments' episode_returns / episode_lengths as they stood BEFORE the rollout, copied
// by the engine), and the block reduces in a fixed order in float64: bit-reproducible, no atomics.
//   out[0] sum of rewards            out[1] number of done steps (= returned episodes)
//   out[2] sum over done steps of returned_episode_returns      out[3] ... of returned_episode_lengths
//   out[4] = out[2]/out[1], out[5] = out[3]/out[1] (0 when no episode ended)    out[6], out[7] = 0
//   (under an episode time limit - rollout_stats_limit_kernel, whose `done` includes the truncations: out[6] = number of truncated steps)
constexpr int kStatsThreads = 1024;
template <bool kLimit>
__device__ __forceinline__ void rollout_stats_body(int T, int N, const float* __restrict__ reward, const unsigned char* __restrict__ done,
                                                   const unsigned char* __restrict__ truncated, const float* __restrict__ ret_in, const int* __restrict__ len_in,
                                                   float* __restrict__ out) {
  __shared__ double red[kStatsThreads / 64][5];
  double sr = 0.0, sd = 0.0, sret = 0.0, slen = 0.0, str = 0.0;
  for (int n = threadIdx.x; n < N; n += kStatsThreads) {
    float ret = ret_in[n];
    int len = len_in[n];
    // the T steps in chunks of eight whose loads are all requested before the first is consumed (the bookkeeping is a dependent chain, the
    // loads are not: one trip to memory per chunk instead of one per step - 16 -> see DESIGN.md 3.6)
    for (int t0 = 0; t0 < T; t0 += 8) {
      float r8[8];
      unsigned char d8[8], u8[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int t = t0 + u < T ? t0 + u : T - 1;
        r8[u] = reward[(size_t)t * N + n];
        d8[u] = done[(size_t)t * N + n];
        if (kLimit) u8[u] = truncated[(size_t)t * N + n];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (t0 + u < T) {
          const float r = r8[u];
          const bool d = d8[u] != 0;
          ret += r; len += 1;                       // new_episode_return / new_episode_length (env.py:183-184)
          sr += (double)r;
          if (d) { sd += 1.0; sret += (double)ret; slen += (double)len; ret = 0.f; len = 0; }  // env.py:187-190
          if (kLimit) str += u8[u] != 0 ? 1.0 : 0.0;
        }
      }
    }
  }
  sr = wave_sum_f64(sr); sd = wave_sum_f64(sd); sret = wave_sum_f64(sret); slen = wave_sum_f64(slen);
  if (kLimit) str = wave_sum_f64(str);
  if ((threadIdx.x & 63) == 0) { double* q = red[threadIdx.x >> 6]; q[0] = sr; q[1] = sd; q[2] = sret; q[3] = slen; q[4] = str; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int w = 0; w < kStatsThreads / 64; ++w) for (int k = 0; k < 5; ++k) a[k] += red[w][k];
    for (int k = 0; k < 4; ++k) out[k] = (float)a[k];
    out[4] = a[1] > 0.0 ? (float)(a[2] / a[1]) : 0.f;
    out[5] = a[1] > 0.0 ? (float)(a[3] / a[1]) : 0.f;
    out[6] = kLimit ? (float)a[4] : 0.f; out[7] = 0.f;
  }
}
__global__ void __launch_bounds__(kStatsThreads) rollout_stats_kernel(int T, int N, const float* __restrict__ reward, const unsigned char* __restrict__ done,
                                                                      const float* __restrict__ ret_in, const int* __restrict__ len_in, float* __restrict__ out) {
  rollout_stats_body<false>(T, N, reward, done, nullptr, ret_in, len_in, out);
}
__global__ void __launch_bounds__(kStatsThreads) rollout_stats_limit_kernel(int T, int N, const float* __restrict__ reward, const unsigned char* __restrict__ done,
                                                                            const unsigned char* __restrict__ truncated, const float* __restrict__ ret_in,
                                                                            const int* __restrict__ len_in, float* __restrict__ out) {
  rollout_stats_body<true>(T, N, reward, done, truncated, ret_in, len_in, out);
}

struct Region { std::string name; size_t off, bytes; };
}  // namespace mppo

struct mppo_engine {
  const mppo_model* model;
  mppo_engine_cfg_t cfg;
  mppo::ModelView mv;
  unsigned char* arena;
  size_t arena_bytes;
  std::vector<mppo::Region> regions;
  int N, T, B, mb, M, E, O, OP, A, H, P;
  float *params, *adam_m, *adam_v, *grad;
  int* count;
  float *state, *reset_rec, *obs, *action, *value, *reward, *log_prob, *last_val, *adv, *target, *noise, *adv_stats, *losses, *stats;
  unsigned char* done;
  int* perm;
  double* adv_sums;
  mppo_env_metrics_t met;
  float *fwd_ws, *grad_ws, *adam_ws;
  float* stat_ret_in;
  int* stat_len_in;
  unsigned* jax_rng;  // [2] carried key | [T][2] action keys | [E][rounds][2] sort keys (rng_impl = 1)
  int jax_rounds;
  void* perm_ws;
  size_t perm_ws_bytes;
  float* env_ws;
  size_t env_ws_bytes;
  mppo::Comm* comm;
  mppo::PeerComm* peer;  // the ranks' peer-to-peer exchange (peer.h); takes precedence over `comm` once connected
  mppo::GraphExec* graph;
  bool graph_failed, was_reset, graph_agreed;
  float* flag_ws;        // one float of the arena: the ranks' agreement on the graph capture (RCCL path)
  // reset noise (mppo_engine_set_reset_noise; 0: every environment restarts from the one constant reset record, nothing below is used)
  float reset_noise;
  unsigned* reset_rng;   // [T][2] this update's step keys (train.py:163) | [2] the reset key (train.py:142): the threefry stream's keys (rng_impl = 1)
  bool prepared;         // an update has been prepared (captured or not): the launch sequence is fixed
  // observation normalisation (mppo_engine_set_obs_norm; off: nothing below is used and no launch is added)
  bool obs_norm;
  float obs_norm_clip, obs_norm_eps;
  double* obs_norm_stats;     // [1 + 2 O] count | mean | M2
  float* obs_norm_table;      // [2][OP] mean32 | inv_std32: what this update's rollout applies
  double* obs_norm_partials;  // [T][G][2][O] the apply launches' sums of this update
  // reward scaling (mppo_engine_set_reward_norm; off: nothing below is used and no launch is added)
  bool reward_norm;
  float reward_norm_clip, reward_norm_eps;
  double* reward_norm_stats;     // [3] count | mean | M2 of the discounted return
  float* reward_norm_table;      // [2] mean32 | inv_std32: the scale this update's rollout applies
  float* reward_norm_carry;      // [N] the discounted return carried from one update to the next
  double* reward_norm_partials;  // [G][2] the apply launch's sums of this update
  float* reward_scaled;          // [T][N] what GAE reads; "reward" stays raw
  // both of them on several ranks: the ranks' sums of this update, gathered - [world][2][O] for the observations, behind them [world][2] for the returns
  double* norm_slots;
  // random pushes (mppo_engine_set_push; body 0: off - the rollout's step launches are the unpushed ones)
  mppo::EnvPush push;
  // episode time limit (mppo_engine_set_time_limit; length 0: off - no launch is added, GAE and the statistics are the plain ones)
  mppo::LimitCfg limit;
  unsigned char* truncated;  // [T][N] the samples the limit cut
  // domain randomisation (mppo_engine_set_domain; table null: off - every launch and every argument is what it was).  The table [N][4] is the engine's own
  // allocation, not a region of the arena: it is a function of (seed, rank) alone, so a checkpoint does not carry it and the arena's layout is what it always was
  mppo::EnvDomain domain;
  // sensor noise and actuation latency (mppo_engine_set_obs_noise / _set_action_delay; off: nothing below is used, no launch is added and the step reads action[t])
  bool obs_noise;
  mppo::ObsNoiseDraw noise_draw;
  float* obs_noise_scale;  // [OP] the per-column half-widths, pad columns 0
  mppo::DelayDraw delay;   // dmax 0: off
  float* action_hist;      // [kMaxActionDelay][N][A] the ring of the policy's past actions (the first dmax slots are used)
  float* action_applied;   // [N][A] what the step launch is given
  int* action_delay;       // [N] the latency table
};

namespace mppo {

static size_t layout(mppo_engine* e, bool assign) {
  size_t off = 0;
  e->regions.clear();
  auto take = [&](const char* name, size_t bytes) -> unsigned char* {
    off = align_up(off, 256);
    e->regions.push_back({name, off, bytes});
    unsigned char* p = assign ? e->arena + off : nullptr;
    off += bytes;
    return p;
  };
  const size_t N = e->N, T = e->T, B = e->B, A = e->A, OP = e->OP, P = e->P, EM = (size_t)e->E * e->M;
  const mppo_net_t& net = e->cfg.net;
  e->params = (float*)take("params", P * 4);
  e->adam_m = (float*)take("adam_m", P * 4);
  e->adam_v = (float*)take("adam_v", P * 4);
  e->grad = (float*)take("grad", P * 4);
  e->count = (int*)take("count", 4 * 4);
  e->state = (float*)take("state", N * e->mv.rec_dim * 4);
  e->reset_rec = (float*)take("reset_rec", (size_t)e->mv.rec_dim * 4);
  e->obs = (float*)take("obs", (T + 1) * N * OP * 4);
  e->action = (float*)take("action", T * N * A * 4);
  e->value = (float*)take("value", (B + N) * 4);  // [T][N] + the bootstrap values behind them (region "last_val" below): one critic launch can write both
  e->reward = (float*)take("reward", B * 4);
  e->log_prob = (float*)take("log_prob", B * 4);
  e->done = (unsigned char*)take("done", B);
  e->last_val = assign ? e->value + B : nullptr;
  for (Region& r : e->regions) if (r.name == "value") { r.bytes = B * 4; e->regions.push_back({"last_val", r.off + B * 4, N * 4}); break; }  // (two names for the two parts)
  e->adv = (float*)take("adv", B * 4);
  e->target = (float*)take("target", B * 4);
  e->noise = (float*)take("noise", T * N * A * 4);
  e->perm = (int*)take("perm", (size_t)e->E * B * 4);
  e->adv_sums = (double*)take("adv_sums", EM * 2 * 8);
  e->adv_stats = (float*)take("adv_stats", EM * 2 * 4);
  e->losses = (float*)take("losses", EM * 4 * 4);
  e->stats = (float*)take("rollout_stats", 8 * 4);
  e->stat_ret_in = (float*)take("stats_carry_returns", N * 4);
  e->stat_len_in = (int*)take("stats_carry_lengths", N * 4);
  e->met.episode_returns = (float*)take("episode_returns", N * 4);
  e->met.episode_lengths = (int32_t*)take("episode_lengths", N * 4);
  e->met.returned_episode_returns = (float*)take("returned_episode_returns", N * 4);
  e->met.returned_episode_lengths = (int32_t*)take("returned_episode_lengths", N * 4);
  e->met.timestep = (int32_t*)take("timestep", N * 4);
  e->met.returned_episode = (uint8_t*)take("returned_episode", N);
  e->fwd_ws = (float*)take("fwd_ws", fwd_bufs_floats(net, (int)N) * 4);
  e->grad_ws = (float*)take("grad_ws", grad_bufs_floats(net, e->mb) * 4);
  e->adam_ws = (float*)take("adam_ws", mppo_adam_ws_bytes(P));
  e->flag_ws = (float*)take("comm_flag", 256);
  e->jax_rounds = threefry_rounds((int)B);
  e->jax_rng = (unsigned*)take("jax_rng", (2 + 2 * T + 2 * (size_t)e->E * e->jax_rounds) * 4);
  e->perm_ws_bytes = mppo_permutation_ws_bytes((int)B);
  if (permutation_batch_ws_bytes((int)B, e->E) > e->perm_ws_bytes) e->perm_ws_bytes = permutation_batch_ws_bytes((int)B, e->E);  // all epochs in one sort
  e->perm_ws = take("perm_ws", e->perm_ws_bytes);
  // a large robot's mass matrices and contact Jacobians, one record per environment (k_physics.hip; nothing for the robots whose working set fits LDS)
  e->env_ws_bytes = model_scratch_bytes(e->model, (int)N);
  e->env_ws = e->env_ws_bytes ? (float*)take("env_scratch", e->env_ws_bytes) : nullptr;
  // the keys of the reset noise's threefry stream: behind everything else, so that every other region is where it was ("jax_rng" keeps its size and meaning)
  e->reset_rng = (unsigned*)take("reset_rng", (2 * T + 2) * 4);
  // observation normalisation: behind those again, present whether or not the option is on
  e->obs_norm_stats = (double*)take("obs_norm_stats", (1 + 2 * (size_t)e->O) * 8);
  e->obs_norm_table = (float*)take("obs_norm_table", 2 * OP * 4);
  e->obs_norm_partials = (double*)take("obs_norm_partials", T * obs_norm_partial_doubles((int)N, e->O) * 8);
  // reward scaling: behind those again, present whether or not the option is on
  e->reward_norm_stats = (double*)take("reward_norm_stats", 3 * 8);
  e->reward_norm_table = (float*)take("reward_norm_table", 2 * 4);
  e->reward_norm_carry = (float*)take("reward_norm_carry", N * 4);
  e->reward_norm_partials = (double*)take("reward_norm_partials", (size_t)reward_norm_partials((int)N) * 2 * 8);
  e->reward_scaled = (float*)take("reward_scaled", B * 4);
  // the episode time limit's flags: behind those again, present whether or not a limit is set
  e->truncated = (unsigned char*)take("truncated", B);
  // actuation latency and sensor noise: behind those again, present whether or not the options are on
  e->action_hist = (float*)take("action_hist", (size_t)kMaxActionDelay * N * A * 4);
  e->action_applied = (float*)take("action_applied", N * A * 4);
  e->action_delay = (int*)take("action_delay", N * 4);
  e->obs_noise_scale = (float*)take("obs_noise_scale", OP * 4);
  // the normalisations across ranks: behind those again, present whatever the options and the rank count are (one rank never touches it)
  e->norm_slots = (double*)take("norm_slots", (size_t)e->cfg.world_size * 2 * ((size_t)e->O + 1) * 8);
  return align_up(off, 256);
}

static int32_t validate_cfg(const mppo_model* m, const mppo_engine_cfg_t* c) {
  MPPO_REQUIRE(m && c, "engine: null model / cfg");
  const ModelView& mv = model_view(m);
  MPPO_REQUIRE(c->num_envs >= 1 && c->num_steps >= 1 && c->num_minibatches >= 1 && c->update_epochs >= 1 && c->n_frames >= 1, "engine: non-positive size in cfg");
  MPPO_REQUIRE(c->world_size >= 1 && c->rank >= 0 && c->rank < c->world_size, "engine: bad rank %d / world %d", c->rank, c->world_size);
  const long B = (long)c->num_envs * c->num_steps;
  // the reference raises ValueError here (train.py:253-255)
  MPPO_REQUIRE(B <= permutation_max_samples(), "engine: %ld samples per rank and update (num_envs x num_steps); the minibatch permutations take at most %d", B, permutation_max_samples());
  MPPO_REQUIRE(B % c->num_minibatches == 0, "`batch_size` must be equal to `num_steps * num_envs` (num_envs*num_steps = %ld is not divisible by num_minibatches = %d)", B,
               c->num_minibatches);
  MPPO_REQUIRE(c->net.O == mv.obs_dim && c->net.OP == mv.obs_pad, "engine: net O/OP (%d/%d) do not match the model's observation (%d/%d)", c->net.O, c->net.OP,
               mv.obs_dim, mv.obs_pad);
  MPPO_REQUIRE(c->net.A == mv.nu, "engine: net A = %d but the model has %d actuators", c->net.A, mv.nu);
  // (up to 32 action dimensions take the fused kernels, 33 .. 63 the layer-wise path: fused_supported, k_fused.hip)
  MPPO_REQUIRE(c->net.A >= 1 && c->net.A <= 63 && c->net.H >= 4 && c->net.H % 4 == 0, "engine: unsupported A / H (1 <= A <= 63, H a multiple of 4)");
  MPPO_REQUIRE(c->net.num_layers >= 0 && c->net.num_layers <= kMaxHidden, "engine: model.num_layers = %d (1 .. %d hidden layers)", c->net.num_layers, kMaxHidden);
  // bf16-in / f32-accumulate products exist in the fused kernels (two hidden layers, H a multiple of 32 up to 256); the layer-wise path is float only
  MPPO_REQUIRE(!c->net.bf16 || (net_layers(c->net) == 2 && c->net.H % 32 == 0 && c->net.H <= 256 && c->net.A <= 32),
               "engine: training.mlp_dtype=bf16 needs the fused kernels (model.num_layers = 2, hidden_size a multiple of 32 up to 256, at most 32 actuators)");
  MPPO_REQUIRE(c->num_updates >= 1, "engine: num_updates must be >= 1 (total_timesteps too small)");
  MPPO_REQUIRE(c->rng_impl == 0 || c->rng_impl == 1, "engine: rng_impl %d (0 philox, 1 threefry)", c->rng_impl);
  MPPO_REQUIRE(c->rng_impl == 0 || c->world_size == 1, "engine: the threefry streams follow the reference's single-device key plumbing (world_size must be 1)");
  return MPPO_OK;
}

static void fill_dims(mppo_engine* e) {
  const mppo_engine_cfg_t& c = e->cfg;
  e->N = c.num_envs; e->T = c.num_steps; e->B = e->N * e->T; e->M = c.num_minibatches; e->E = c.update_epochs; e->mb = e->B / e->M;
  e->O = c.net.O; e->OP = c.net.OP; e->A = c.net.A; e->H = c.net.H; e->P = param_layout(c.net).total;
}

constexpr unsigned long long kStreamNoise = 0x4E4F495345ull << 24;  // "NOISE"
constexpr unsigned long long kStreamPerm = 0x5045524Dull << 24;     // "PERM"
// ("RESET" << 24, kStreamReset: the reset noise's stream, drawn inside the environment kernel - k_physics.hip)

// The reset noise's event counter (Philox stream): event 0 is mppo_engine_reset, step t of update u is event u * T + 1 + t, with u read on the device from
// count[1] - the update index that advance_counters_kernel moves on at the end of every update, so a replayed graph draws fresh values at every step.


static bool shadow_enabled() {  // MPPO_NO_SHADOW=1: A/B switch for measurements
  static const bool no_shadow = [] { const char* v = MPPO_EXPERIMENT_ENV("MPPO_NO_SHADOW"); return v && v[0] == '1'; }();
  return !no_shadow;
}

static bool pregather_enabled() {  // MPPO_NO_PREGATHER=1: A/B switch for measurements
  static const bool off = [] { const char* v = MPPO_EXPERIMENT_ENV("MPPO_NO_PREGATHER"); return v && v[0] == '1'; }();
  return !off;
}

// What carries this engine's collectives: the ranks' hipIpc-mapped exchange buffers (peer.h) once connected, else the RCCL communicator.
// MPPO_FORCE_COMM=1 runs the collectives also at world size 1 (identity all-reduce): hardware check of the RCCL path
struct Transport { bool peer, comm; };
static Transport transport_of(const mppo_engine* e) {
  const char* fc = getenv("MPPO_FORCE_COMM");
  const bool force_comm = fc && fc[0] == '1';
  const bool peer = peer_connected(e->peer);
  return Transport{peer, !peer && (e->cfg.world_size > 1 || (force_comm && e->comm))};
}

static int32_t do_rollout(mppo_engine* e, hipStream_t s) {
  const mppo_engine_cfg_t& c = e->cfg;
  const size_t N = e->N, OP = e->OP, A = e->A;
  // episode bookkeeping as it stands before the rollout: carry-in of the statistics kernel at the end
  MPPO_CHECK_HIP(hipMemcpyAsync(e->stat_ret_in, e->met.episode_returns, N * 4, hipMemcpyDeviceToDevice, s));
  MPPO_CHECK_HIP(hipMemcpyAsync(e->stat_len_in, e->met.episode_lengths, N * 4, hipMemcpyDeviceToDevice, s));
  if (!c.external_random) {
    if (c.rng_impl == 1) {
      // the reference's key plumbing (train.py:158,163,252): this update's action keys and sort keys from the carried key,
      // then one jax.random.normal(action_rng, (N, A)) per env step (what `pi.sample(seed=action_rng)` draws)
      MPPO_TRY(threefry_chain(e->jax_rng, e->T, e->E, e->jax_rounds, e->jax_rng + 2, e->jax_rng + 2 + 2 * e->T, e->reset_noise > 0.f ? e->reset_rng : nullptr, s));
      for (int t = 0; t < e->T; ++t) MPPO_TRY(threefry_normal(e->jax_rng + 2 + 2 * t, N * A, e->noise + (size_t)t * N * A, s));
    } else {
      MPPO_TRY(normal_fill_ctr(c.seed, kStreamNoise + ((unsigned long long)c.rank << 16), e->count + 1, (size_t)e->T * N * A, e->noise, s));
    }
  }
  FwdBufs fb = carve_fwd(c.net, e->N, e->fwd_ws);
  if (c.net.bf16 && shadow_enabled() && fused_rollout_supported(c.net, e->obs, e->OP)) {
    // bf16 network: the rollout forwards read the bf16 fragment copies of the gradient workspace too; they are rebuilt here (the
    // parameters may have been written from outside since the last update) and nothing changes the parameters before the learn phase
    const GradBufs gb = carve_grad(c.net, e->mb, e->grad_ws);
    MPPO_TRY(shadow_refresh(c.net, e->params, gb, s));
    fb.frag = gb.frag; fb.frag_net_stride = gb.frag_net_stride;
  }
  // (measurement, -DMPPO_EXPERIMENTS: MPPO_DEFER_CRITIC=1 takes the critic off the rollout's launches - actor-only rollout forwards, one critic launch before GAE)
  static const char* defer_env = MPPO_EXPERIMENT_ENV("MPPO_DEFER_CRITIC");
  const bool defer_critic = defer_env && defer_env[0] == '1' && fused_rollout_supported(c.net, e->obs, e->OP);
  for (int t = 0; t < e->T; ++t) {
    const float* obs_t = e->obs + (size_t)t * N * OP;
    MPPO_TRY(policy_forward(c.net, e->params, e->N, obs_t, e->OP, fb, e->noise + t * N * A, e->action + t * N * A, e->log_prob + t * N,
                            defer_critic ? nullptr : e->value + (size_t)t * N, nullptr, s));                          // train.py:157-160
    // (random pushes: the wrench of step u * T + t, u the device's update index, is drawn inside this launch - a replayed graph draws fresh ones; off: the plain step)
    EnvPush push = e->push;
    push.add = t;
    // actuation latency: the policy's action goes into the ring, the step is given the one its environment's latency ago (zeros at an episode's start); the
    // trajectory keeps the policy's own action and log_prob - what PPO's ratio refers to.  Off: the step reads action[t] as it always did
    const float* act_t = e->action + t * N * A;
    if (e->delay.dmax > 0) {
      MPPO_TRY(action_delay_launch(e->N, e->A, e->delay.dmax, e->action_delay, e->met.timestep, e->met.episode_lengths, act_t, e->A, e->action_hist, e->action_applied,
                                   e->A, s));
      act_t = e->action_applied;
    }
    MPPO_TRY(env_step_push_ws(e->model, e->N, c.n_frames, &c.reward, e->state, e->reset_rec, act_t, e->A, e->obs + (size_t)(t + 1) * N * OP,
                              e->OP, e->reward + t * N, e->done + t * N, &e->met, push, e->env_ws, e->env_ws_bytes, static_cast<hipStream_t>(s), e->domain));            // :165
    // episode time limit: the environments that have reached it are truncated - flags, metrics, the reset record - as the step's epilogue ends an episode;
    // done[t] then includes them, so the masked reinit below restarts them too and the reward scaling's carry restarts behind them
    if (e->limit.length > 0)
      MPPO_TRY(time_limit_launch(e->limit, e->N, e->mv.rec_dim, e->OP, e->state, e->reset_rec, e->obs + (size_t)(t + 1) * N * OP, e->OP, e->done + t * N,
                                 e->truncated + t * N, e->met, s));
    // reset noise: the environments whose episode ended at this step restart from a randomised state instead of the constant record the step kernel
    // gave them (env.py:166,179-180) - one masked launch of the reset kernel over done[t]; a workgroup without an ended episode leaves at once
    // (domain randomisation: the one shared reset record is another robot's - every restart goes through the reset kernel with the environment's own row,
    // at scale 0 when reset noise is off)
    if (e->reset_noise > 0.f || e->domain.table)
      MPPO_TRY(env_reinit_ws(e->model, e->N, e->state, e->obs + (size_t)(t + 1) * N * OP, e->OP, e->done + t * N, e->reset_noise, c.rng_impl, c.seed, c.rank,
                             e->reset_rng + 2 * t, e->count + 1, e->T, 1 + t, e->env_ws, e->env_ws_bytes, s, e->domain));
    // sensor noise: the new rows - restarted environments' included - get the noise of step u * T + t + 1, u the device's update index; what is stored is what
    // the next forward, the critic's bootstrap, the learn phase and the normalisation's statistics read
    if (e->obs_noise)
      MPPO_TRY(obs_noise_launch(e->noise_draw, e->N, e->O, e->obs + (size_t)(t + 1) * N * OP, e->OP, e->obs_noise_scale, e->count + 1, e->T, t + 1, s));
    // observation normalisation: the new rows are stored normalised with this update's table (the next forward and the learn phase read them so);
    // their raw values go into this step's partial sums first
    if (e->obs_norm)
      MPPO_TRY(obs_norm_apply_launch(e->N, e->O, e->obs + (size_t)(t + 1) * N * OP, e->OP, e->obs_norm_table, e->OP, e->obs_norm_clip,
                                     e->obs_norm_partials + (size_t)t * obs_norm_partial_doubles(e->N, e->O), s));
  }
  if (defer_critic)  // value[t] of all T steps and the bootstrap value in ONE critic launch over the [T + 1][N] observation rows (nothing before GAE reads them)
    MPPO_TRY(policy_forward(c.net, e->params, (e->T + 1) * e->N, e->obs, e->OP, fb, nullptr, nullptr, nullptr, e->value, nullptr, s));
  else
    MPPO_TRY(policy_forward(c.net, e->params, e->N, e->obs + (size_t)e->T * N * OP, e->OP, fb, nullptr, nullptr, nullptr, e->last_val, nullptr, s));  // train.py:182
  // reward scaling: GAE reads the rewards divided by the return deviation collected through the previous update (the scale is frozen within an update);
  // the statistics kernel below, the metrics and the history go on reading the raw rewards
  if (e->reward_norm)
    MPPO_TRY(reward_norm_apply_launch(e->T, e->N, c.gamma, e->reward, e->done, e->reward_norm_carry, e->reward_norm_table, e->reward_norm_clip, e->reward_scaled,
                                      e->reward_norm_partials, s));
  // (under a time limit the scan is cut at the truncated samples and the statistics count them; without one: the plain launches)
  MPPO_TRY(gae_truncated_launch(e->T, e->N, c.gamma, c.gae_lambda, e->reward_norm ? e->reward_scaled : e->reward, e->value, e->done,
                                e->limit.length > 0 ? e->truncated : nullptr, e->last_val, e->adv, e->target, s));
  if (e->limit.length > 0)
    hipLaunchKernelGGL(rollout_stats_limit_kernel, dim3(1), dim3(kStatsThreads), 0, s, e->T, e->N, e->reward, e->done, e->truncated, e->stat_ret_in, e->stat_len_in, e->stats);
  else
    hipLaunchKernelGGL(rollout_stats_kernel, dim3(1), dim3(kStatsThreads), 0, s, e->T, e->N, e->reward, e->done, e->stat_ret_in, e->stat_len_in, e->stats);
  MPPO_CHECK_LAUNCH("rollout_stats_kernel");
  const Transport tp = transport_of(e);
  if ((e->obs_norm || e->reward_norm) && (tp.peer || tp.comm)) {
    // Several ranks (or MPPO_FORCE_COMM=1 at one: the gather as the identity): every rank adds its own partials in index order into its slot, the slots are
    // gathered - ONE exchange per update for both options, on the transport the learn phase uses - and the update kernel adds them in rank order and merges
    // k = T N G rows.  Every rank started from the same statistics and table and merges the same bytes: statistics and tables stay replicas.
    const int G = c.world_size;
    double* const obs_slots = e->norm_slots;
    double* const rew_slots = e->norm_slots + (size_t)G * 2 * e->O;
    if (e->obs_norm) MPPO_TRY(obs_norm_rank_sums_launch(e->O, e->T * obs_norm_partials(e->N), e->obs_norm_partials, c.rank, G, obs_slots, s));
    if (e->reward_norm) MPPO_TRY(obs_norm_rank_sums_launch(1, reward_norm_partials(e->N), e->reward_norm_partials, c.rank, G, rew_slots, s));
    if (tp.peer) {
      if (e->obs_norm) MPPO_TRY(peer_gather_f64(e->peer, obs_slots, 2 * e->O, (size_t)G * 2 * e->O, e->reward_norm ? 2 : 0, s));
      else MPPO_TRY(peer_gather_f64(e->peer, rew_slots, 2, 0, 0, s));
    } else {  // a sum in which every foreign term is +0.0: a gather, whatever order the library adds in
      double* const first = e->obs_norm ? obs_slots : rew_slots;
      MPPO_TRY(comm_allreduce_f64(e->comm, first, (size_t)G * 2 * ((e->obs_norm ? (size_t)e->O : 0) + (e->reward_norm ? 1 : 0)), s));
    }
    const long long rows = (long long)e->T * e->N * G;
    if (e->obs_norm) MPPO_TRY(obs_norm_update_launch(e->O, G, rows, obs_slots, e->obs_norm_stats, e->obs_norm_eps, e->obs_norm_table, e->OP, s));
    if (e->reward_norm) MPPO_TRY(obs_norm_update_launch(1, G, rows, rew_slots, e->reward_norm_stats, e->reward_norm_eps, e->reward_norm_table, 1, s));
    return MPPO_OK;
  }
  if (e->obs_norm)  // the T steps' rows join the running statistics; the table is rewritten for the next update (nothing of this one applies it any more)
    MPPO_TRY(obs_norm_update_launch(e->O, e->T * obs_norm_partials(e->N), (long long)e->T * e->N, e->obs_norm_partials, e->obs_norm_stats, e->obs_norm_eps, e->obs_norm_table,
                                    e->OP, s));
  if (e->reward_norm)  // this update's T N returns join the running statistics; the scale is rewritten for the next update
    MPPO_TRY(obs_norm_update_launch(1, reward_norm_partials(e->N), (long long)e->T * e->N, e->reward_norm_partials, e->reward_norm_stats, e->reward_norm_eps,
                                    e->reward_norm_table, 1, s));
  return MPPO_OK;
}

static int32_t do_learn(mppo_engine* e, hipStream_t s) {
  const mppo_engine_cfg_t& c = e->cfg;
  const int EM = e->E * e->M;
  if (!c.external_random) {
    if (c.rng_impl == 1) {
      for (int ep = 0; ep < e->E; ++ep)
        MPPO_TRY(threefry_permutation(e->jax_rng + 2 + 2 * e->T + 2 * ep * e->jax_rounds, e->jax_rounds, e->B, e->perm + (size_t)ep * e->B, e->perm_ws,
                                      e->perm_ws_bytes, s));                                                          // train.py:258 with JAX's keys
    } else {
      // train.py:258 for all E epochs at once (one sort: k_perm.hip); stream ids kStreamPerm + (rank << 16) + ep as before
      MPPO_TRY(permutation_batch_ctr(c.seed, kStreamPerm + ((unsigned long long)c.rank << 16), e->count + 1, e->B, e->E, e->perm, e->perm_ws, e->perm_ws_bytes, s));
    }
  }
  MPPO_TRY(mppo_adv_sums(e->adv, e->perm, EM, e->mb, e->adv_sums, s));
  const Transport tp = transport_of(e);
  const bool use_peer = tp.peer;  // gradients travel through the ranks' hipIpc-mapped exchange buffers (peer.h)
  const bool use_comm = tp.comm;
  if (use_peer) MPPO_TRY(peer_allreduce_f64(e->peer, e->adv_sums, (size_t)EM * 2, s));
  if (use_comm) MPPO_TRY(comm_allreduce_f64(e->comm, e->adv_sums, (size_t)EM * 2, s));
  MPPO_TRY(mppo_adv_stats_finalize(e->adv_sums, EM, (double)e->mb * c.world_size, e->adv_stats, s));
  mppo_batch_t batch;
  batch.obs = e->obs; batch.obs_ld = e->OP; batch.action = e->action; batch.act_ld = e->A; batch.value = e->value; batch.log_prob = e->log_prob;
  batch.adv = e->adv; batch.target = e->target;
  GradBufs gb = carve_grad(c.net, e->mb, e->grad_ws);
  // W2^T shadow copies for the backward row pass: rebuilt from the parameters once per update (they may have been written from
  // outside: upload, checkpoint), then kept current by every Adam step of the update
  static const char* nofuse = MPPO_EXPERIMENT_ENV("MPPO_NO_FUSED");
  const bool fused_path = fused_supported(c.net, batch) && !(nofuse && nofuse[0] == '1');
  const bool use_shadow = fused_supported(c.net, batch) && shadow_enabled();
  ShadowRef shadow = make_shadow_ref(c.net, gb);
  if (use_shadow) {
    MPPO_TRY(shadow_refresh(c.net, e->params, gb, s));
    gb.w2t_valid = true;
  }
  // the row pass of step st gathers the observation rows of step st + 1 beside its own work (k_fused.hip, XPre); the first
  // step's rows are gathered here
  const bool use_pre = use_shadow && pregather_enabled();
  if (use_pre) MPPO_TRY(fused_gather_rows(c.net, batch, e->perm, e->mb, gb.xmb, s));
  const float inv_count = 1.f / ((float)e->mb * (float)c.world_size);
  mppo_adam_cfg_t ac = c.adam;
  ac.sched_div = e->mb * c.world_size * e->E;  // minibatch_size * update_epochs of the GLOBAL batch (train.py:94,100)
  ac.num_updates = c.num_updates;
  for (int ep = 0; ep < e->E; ++ep) {
    for (int k = 0; k < e->M; ++k) {
      const int st = ep * e->M + k;
      const bool single = !use_comm && !use_peer;  // then the reduce kernel's sums of squares are those of the final gradient
      XPre pre{(st & 1) ? gb.xmb2 : gb.xmb, (st & 1) ? gb.xmb : gb.xmb2,
               st + 1 < EM ? e->perm + (size_t)((st + 1) / e->M) * e->B + (size_t)((st + 1) % e->M) * e->mb : nullptr};
      const int* idx = e->perm + (size_t)ep * e->B + (size_t)k * e->mb;
      if (use_peer) {
        // the local gradient goes straight into this rank's exchange buffer (the weight-gradient launch signals the peers; the
        // layer-wise path's gradient is copied there by a publish kernel), and the Adam launch reduces this rank's slice,
        // broadcasts it, waits for the others' and applies the update: the same three launches as on one GPU
        const PeerStep ps = peer_step(e->peer, st);
        if (fused_path) {
          MPPO_TRY(minibatch_grad(c.net, e->params, batch, idx, e->mb, e->adv_stats + 2 * st, inv_count, c.loss, peer_pub(e->peer), e->losses + 4 * st, nullptr, gb, s,
                                  use_pre ? &pre : nullptr, &ps));
        } else {
          MPPO_TRY(minibatch_grad(c.net, e->params, batch, idx, e->mb, e->adv_stats + 2 * st, inv_count, c.loss, e->grad, e->losses + 4 * st, nullptr, gb, s, nullptr));
          MPPO_TRY(peer_publish(e->peer, e->grad, (size_t)e->P, st, s));
        }
        MPPO_TRY(clip_adam((size_t)e->P, e->params, e->adam_m, e->adam_v, peer_red(e->peer), e->count, st, ac, const_cast<float*>(peer_red(e->peer)) + e->P, true, s,
                           use_shadow ? &shadow : nullptr, &ps));
        continue;
      }
      MPPO_TRY(minibatch_grad(c.net, e->params, batch, idx, e->mb, e->adv_stats + 2 * st, inv_count, c.loss, e->grad,
                              e->losses + 4 * st, single ? e->adam_ws : nullptr, gb, s, use_pre ? &pre : nullptr));  // train.py:246-247
      if (!single) MPPO_TRY(comm_allreduce_f32(e->comm, e->grad, (size_t)e->P, s));
      MPPO_TRY(clip_adam((size_t)e->P, e->params, e->adam_m, e->adam_v, e->grad, e->count, st, ac, e->adam_ws, single, s, use_shadow ? &shadow : nullptr));  // train.py:248
#ifdef MPPO_EXPERIMENTS
      static const int extra = [] { const char* v = getenv("MPPO_EXTRA_LAUNCHES"); return v ? atoi(v) : 0; }();  // timing experiment: what does ONE more trivial launch cost here?
      for (int x = 0; x < extra; ++x) hipLaunchKernelGGL(advance_counters_kernel, dim3(1), dim3(64), 0, s, e->count, 0, (int*)nullptr, 0);
#endif
    }
  }
  if (use_peer) MPPO_TRY(peer_advance(e->peer, EM, s));
  int* perm_cnt = nullptr;
  int perm_ncnt = 0;
  if (!c.external_random && c.rng_impl != 1) permutation_batch_counters(e->B, e->E, e->perm_ws, e->perm_ws_bytes, &perm_cnt, &perm_ncnt);
  hipLaunchKernelGGL(advance_counters_kernel, dim3(1), dim3(256), 0, s, e->count, EM, perm_cnt, perm_ncnt);
  MPPO_CHECK_LAUNCH("advance_counters_kernel");
  // carry last_obs into slot 0 of the next rollout (RunnerState.last_obs, train.py:174,279)
  MPPO_CHECK_HIP(hipMemcpyAsync(e->obs, e->obs + (size_t)e->T * e->N * e->OP, (size_t)e->N * e->OP * 4, hipMemcpyDeviceToDevice, s));
  return MPPO_OK;
}

}  // namespace mppo

using namespace mppo;

extern "C" int32_t mppo_engine_arena_bytes(const mppo_model_t* m, const mppo_engine_cfg_t* cfg, size_t* out) {
  MPPO_TRY(validate_cfg(m, cfg));
  MPPO_REQUIRE(out, "mppo_engine_arena_bytes: null out");
  mppo_engine tmp{};
  tmp.model = m; tmp.cfg = *cfg; tmp.mv = model_view(m);
  fill_dims(&tmp);
  *out = layout(&tmp, false);
  return MPPO_OK;
}

extern "C" int32_t mppo_engine_create(const mppo_model_t* m, const mppo_engine_cfg_t* cfg, void* arena, size_t arena_bytes, mppo_engine_t** out) {
  MPPO_TRY(validate_cfg(m, cfg));
  MPPO_REQUIRE(arena && out, "mppo_engine_create: null arena / out");
  MPPO_REQUIRE((reinterpret_cast<uintptr_t>(arena) & 255) == 0, "mppo_engine_create: arena must be 256-byte aligned");
  mppo_engine* e = new mppo_engine();
  e->model = m; e->cfg = *cfg; e->mv = model_view(m);
  e->arena = static_cast<unsigned char*>(arena);
  e->arena_bytes = arena_bytes;
  fill_dims(e);
  const size_t need = layout(e, true);
  if (arena_bytes < need) { delete e; return fail(MPPO_ENOMEM, "mppo_engine_create: arena %zu < %zu bytes", arena_bytes, need); }
  e->comm = nullptr; e->peer = nullptr; e->graph = nullptr; e->graph_failed = false; e->was_reset = false; e->graph_agreed = false;
  e->reset_noise = 0.f; e->prepared = false;
  e->obs_norm = false; e->obs_norm_clip = 0.f; e->obs_norm_eps = 0.f;
  e->reward_norm = false; e->reward_norm_clip = 0.f; e->reward_norm_eps = 0.f;
  e->push = EnvPush{};
  e->limit = LimitCfg{};
  e->domain = EnvDomain{};
  e->obs_noise = false; e->noise_draw = ObsNoiseDraw{}; e->delay = DelayDraw{};
  *out = e;
  return MPPO_OK;
}

extern "C" int32_t mppo_engine_destroy(mppo_engine_t* e) {
  if (!e) return MPPO_OK;
  if (e->graph) graph_destroy(e->graph);
  if (e->comm) comm_destroy(e->comm);
  if (e->peer) peer_destroy(e->peer);
  if (e->domain.table) (void)hipFree(const_cast<float*>(e->domain.table));
  delete e;
  return MPPO_OK;
}

extern "C" int32_t mppo_engine_region(const mppo_engine_t* e, const char* name, size_t* offset, size_t* nbytes) {
  MPPO_REQUIRE(e && name && offset && nbytes, "mppo_engine_region: null argument");
  for (const Region& r : e->regions)
    if (r.name == name) { *offset = r.off; *nbytes = r.bytes; return MPPO_OK; }
  return fail(MPPO_EINVAL, "mppo_engine_region: no region named '%s'", name);
}

extern "C" int32_t mppo_comm_unique_id(void* id128) {
  MPPO_REQUIRE(id128, "mppo_comm_unique_id: null");
  return comm_unique_id(id128);
}

extern "C" int32_t mppo_engine_comm_init(mppo_engine_t* e, const void* id128) {
  MPPO_REQUIRE(e && id128, "mppo_engine_comm_init: null argument");
  MPPO_REQUIRE(!e->comm, "mppo_engine_comm_init: communicator already initialised");
  MPPO_TRY(comm_create(id128, e->cfg.rank, e->cfg.world_size, &e->comm));
  // one eager all-reduce of each kind now (scratch regions of the arena, overwritten before they are read): RCCL sets up
  // its channels and buffers on the first call, which must not happen inside a stream capture
  MPPO_CHECK_HIP(hipMemsetAsync(e->grad, 0, (size_t)e->P * 4, nullptr));
  MPPO_CHECK_HIP(hipMemsetAsync(e->adv_sums, 0, (size_t)e->E * e->M * 2 * 8, nullptr));
  MPPO_TRY(comm_allreduce_f32(e->comm, e->grad, (size_t)e->P, nullptr));
  MPPO_TRY(comm_allreduce_f64(e->comm, e->adv_sums, (size_t)e->E * e->M * 2, nullptr));
  MPPO_CHECK_HIP(hipStreamSynchronize(nullptr));
  return MPPO_OK;
}

extern "C" int32_t mppo_engine_reset(mppo_engine_t* e, void* stream) {
  MPPO_REQUIRE(e, "mppo_engine_reset: null engine");
  hipStream_t s = static_cast<hipStream_t>(stream);
  MPPO_CHECK_HIP(hipMemsetAsync(e->count, 0, 16, s));
  MPPO_CHECK_HIP(hipMemsetAsync(e->adam_m, 0, (size_t)e->P * 4, s));
  MPPO_CHECK_HIP(hipMemsetAsync(e->adam_v, 0, (size_t)e->P * 4, s));
  MPPO_CHECK_HIP(hipMemsetAsync(e->obs, 0, (size_t)(e->T + 1) * e->N * e->OP * 4, s));
  MPPO_TRY(permutation_batch_prepare(e->B, e->E, e->perm_ws, e->perm_ws_bytes, s));
  MPPO_TRY(env_reset_ws(e->model, e->N, e->state, e->reset_rec, e->obs, e->OP, nullptr, nullptr, &e->met, e->env_ws, e->env_ws_bytes, static_cast<hipStream_t>(s), e->domain));  // train.py:142-144
  // reset noise: the plain reset above made the noise-free reset record and the zeroed metrics; every environment then starts from a state of its own
  // (event 0 of the Philox stream; the reset key behind the step keys of region "reset_rng" for threefry: the caller writes it before this call)
  if (e->reset_noise > 0.f)
    MPPO_TRY(env_reinit_ws(e->model, e->N, e->state, e->obs, e->OP, nullptr, e->reset_noise, e->cfg.rng_impl, e->cfg.seed, e->cfg.rank, e->reset_rng + 2 * e->T, nullptr, 0, 0,
                           e->env_ws, e->env_ws_bytes, s, e->domain));
  // sensor noise: the row the reset wrote is step 0 of the noise's stream (the state records stay exact)
  if (e->obs_noise) MPPO_TRY(obs_noise_launch(e->noise_draw, e->N, e->O, e->obs, e->OP, e->obs_noise_scale, nullptr, 0, 0, s));
  // actuation latency: an empty ring, and the table of every environment's latency (a function of seed and rank: a resumed run has the same robots)
  if (e->delay.dmax > 0) {
    MPPO_CHECK_HIP(hipMemsetAsync(e->action_hist, 0, (size_t)kMaxActionDelay * e->N * e->A * 4, s));
    MPPO_TRY(action_delay_fill_launch(e->delay, e->N, e->action_delay, s));
  }
  if (e->obs_norm) {  // nothing counted, the identity table (pad columns included); obs[0] above stays raw
    MPPO_CHECK_HIP(hipMemsetAsync(e->obs_norm_stats, 0, (1 + 2 * (size_t)e->O) * 8, s));
    MPPO_TRY(obs_norm_update_launch(e->O, 0, 0, nullptr, e->obs_norm_stats, e->obs_norm_eps, e->obs_norm_table, e->OP, s));
  }
  if (e->reward_norm) {  // nothing counted, no return carried, the identity table: the first update's rewards are multiplied by 1
    MPPO_CHECK_HIP(hipMemsetAsync(e->reward_norm_stats, 0, 3 * 8, s));
    MPPO_CHECK_HIP(hipMemsetAsync(e->reward_norm_carry, 0, (size_t)e->N * 4, s));
    MPPO_TRY(obs_norm_update_launch(1, 0, 0, nullptr, e->reward_norm_stats, e->reward_norm_eps, e->reward_norm_table, 1, s));
  }
  e->was_reset = true;
  return MPPO_OK;
}

extern "C" int32_t mppo_engine_set_obs_norm(mppo_engine_t* e, int32_t enabled, float clip, float eps) {
  MPPO_REQUIRE(e, "mppo_engine_set_obs_norm: null engine");
  MPPO_REQUIRE(clip >= 0.f && eps >= 0.f, "mppo_engine_set_obs_norm: clip %g / eps %g is negative (or not a number)", (double)clip, (double)eps);
  MPPO_REQUIRE(!enabled || e->cfg.world_size == 1 || e->comm || peer_connected(e->peer), "mppo_engine_set_obs_norm: world_size = %d ranks - the running statistics are "
               "gathered over the ranks' transport once per update: connect it first (mppo_engine_peer_connect or mppo_engine_comm_init), then enable the option", e->cfg.world_size);
  if (e->graph || e->prepared)
    return fail(MPPO_ESTATE, "mppo_engine_set_obs_norm: the update has been prepared already (its launch sequence is fixed, a captured graph holds it): "
                             "call it before mppo_engine_reset, mppo_engine_prepare and the first mppo_engine_update");
  if (e->was_reset)
    return fail(MPPO_ESTATE, "mppo_engine_set_obs_norm: mppo_engine_reset has run already (it zeroes the statistics and writes the identity table): call it before the reset");
  e->obs_norm = enabled != 0;
  e->obs_norm_clip = clip;
  e->obs_norm_eps = eps;
  return MPPO_OK;
}

extern "C" int32_t mppo_engine_set_reward_norm(mppo_engine_t* e, int32_t enabled, float clip, float eps) {
  MPPO_REQUIRE(e, "mppo_engine_set_reward_norm: null engine");
  MPPO_REQUIRE(clip >= 0.f && eps >= 0.f, "mppo_engine_set_reward_norm: clip %g / eps %g is negative (or not a number)", (double)clip, (double)eps);
  MPPO_REQUIRE(!enabled || e->cfg.world_size == 1 || e->comm || peer_connected(e->peer), "mppo_engine_set_reward_norm: world_size = %d ranks - the running statistics are "
               "gathered over the ranks' transport once per update: connect it first (mppo_engine_peer_connect or mppo_engine_comm_init), then enable the option", e->cfg.world_size);
  if (e->graph || e->prepared)
    return fail(MPPO_ESTATE, "mppo_engine_set_reward_norm: the update has been prepared already (its launch sequence is fixed, a captured graph holds it): "
                             "call it before mppo_engine_reset, mppo_engine_prepare and the first mppo_engine_update");
  if (e->was_reset)
    return fail(MPPO_ESTATE, "mppo_engine_set_reward_norm: mppo_engine_reset has run already (it zeroes the statistics and the carry and writes the identity table): "
                             "call it before the reset");
  e->reward_norm = enabled != 0;
  e->reward_norm_clip = clip;
  e->reward_norm_eps = eps;
  return MPPO_OK;
}

extern "C" int32_t mppo_engine_set_reset_noise(mppo_engine_t* e, float scale) {
  MPPO_REQUIRE(e, "mppo_engine_set_reset_noise: null engine");
  MPPO_REQUIRE(scale >= 0.f, "mppo_engine_set_reset_noise: scale %g is negative (or not a number)", (double)scale);
  if (e->graph || e->prepared)
    return fail(MPPO_ESTATE, "mppo_engine_set_reset_noise: the update has been prepared already (its launch sequence is fixed, a captured graph holds it): "
                             "set the scale before mppo_engine_prepare and the first mppo_engine_update");
  if (e->was_reset && scale != e->reset_noise)
    return fail(MPPO_ESTATE, "mppo_engine_set_reset_noise: mppo_engine_reset has run already (the environments hold the initial states of scale %g): set the scale before it",
                (double)e->reset_noise);
  e->reset_noise = scale;
  return MPPO_OK;
}

extern "C" int32_t mppo_engine_set_push(mppo_engine_t* e, const mppo_push_cfg_t* push) {
  MPPO_REQUIRE(e, "mppo_engine_set_push: null engine");
  if (push) MPPO_TRY(check_push_cfg("mppo_engine_set_push", push));
  const bool on = push && push->force > 0.f;
  if (on) MPPO_TRY(check_push_body("mppo_engine_set_push", e->model, push->body));
  if (e->graph || e->prepared)
    return fail(MPPO_ESTATE, "mppo_engine_set_push: the update has been prepared already (its launch sequence is fixed, a captured graph holds it): "
                             "set the pushes before mppo_engine_prepare and the first mppo_engine_update");
  if (e->was_reset)
    return fail(MPPO_ESTATE, "mppo_engine_set_push: mppo_engine_reset has run already: set the pushes before it");
  e->push = EnvPush{};
  if (on) {
    mppo_push_cfg_t pc = *push;
    pc.seed = e->cfg.seed; pc.rank = e->cfg.rank;  // (the engine's own: one stream per rank, as the action noise and the reset noise have)
    MPPO_TRY(check_push_cfg("mppo_engine_set_push", &pc));  // (the rank that is used - the engine configuration's - fits the stream id's eight bits)
    e->push.body = pc.body; e->push.draw = push_draw_of(pc); e->push.ctr = e->count + 1; e->push.mul = e->T;
  }
  return MPPO_OK;
}

extern "C" int32_t mppo_engine_set_domain(mppo_engine_t* e, const mppo_domain_cfg_t* domain) {
  MPPO_REQUIRE(e, "mppo_engine_set_domain: null engine");
  mppo_domain_cfg_t dc{};
  bool on = false;
  if (domain) {
    dc = *domain;
    dc.seed = e->cfg.seed; dc.rank = e->cfg.rank;  // (the engine's own: one stream per rank, as the pushes and the reset noise have; nothing crosses ranks)
    on = domain_cfg_on(dc);
    MPPO_TRY(check_domain_cfg("mppo_engine_set_domain", on ? e->model : nullptr, &dc));
  }
  if (e->graph || e->prepared)
    return fail(MPPO_ESTATE, "mppo_engine_set_domain: the update has been prepared already (its launch sequence is fixed, a captured graph holds it): "
                             "set the randomisation before mppo_engine_prepare and the first mppo_engine_update");
  if (e->was_reset)
    return fail(MPPO_ESTATE, "mppo_engine_set_domain: mppo_engine_reset has run already (the environments hold the initial states of the robots they were): set the randomisation before it");
  // the table lives on the device the arena is on, whatever the calling thread's current device is (restored on the way out)
  int cur = -1, dev = -1;
#ifndef MPPO_EMU
  {
    hipPointerAttribute_t attr{};
    MPPO_CHECK_HIP(hipGetDevice(&cur));
    MPPO_CHECK_HIP(hipPointerGetAttributes(&attr, e->arena));
    dev = attr.device;
    if (dev != cur) MPPO_CHECK_HIP(hipSetDevice(dev));
  }
#endif
  auto back = [&](int32_t rc) {
#ifndef MPPO_EMU
    if (dev != cur && cur >= 0) (void)hipSetDevice(cur);
#endif
    return rc;
  };
  if (e->domain.table) {
    if (hipDeviceSynchronize() != hipSuccess) return back(fail(MPPO_EHIP, "mppo_engine_set_domain: the device does not synchronise"));
    (void)hipFree(const_cast<float*>(e->domain.table));
  }
  e->domain = EnvDomain{};
  if (on) {
    float* table = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&table), (size_t)e->N * 16) != hipSuccess) return back(fail(MPPO_EHIP, "mppo_engine_set_domain: no device memory for the table of %d environments", e->N));
    int32_t rc = domain_fill_launch(dc, e->N, table, nullptr);
    if (rc == MPPO_OK && hipStreamSynchronize(nullptr) != hipSuccess) rc = fail(MPPO_EHIP, "mppo_engine_set_domain: the fill launch failed");
    if (rc != MPPO_OK) { (void)hipFree(table); return back(rc); }
    e->domain = EnvDomain{table, dc.mass_body};
  }
  return back(MPPO_OK);
}

extern "C" int32_t mppo_engine_set_time_limit(mppo_engine_t* e, int32_t length, int32_t stagger) {
  MPPO_REQUIRE(e, "mppo_engine_set_time_limit: null engine");
  mppo_time_limit_cfg_t lc{};
  lc.length = length; lc.stagger = stagger != 0 ? 1 : 0; lc.seed = e->cfg.seed;
  lc.rank = length > 0 ? e->cfg.rank : 0;  // (the engine's own: one stream per rank, as the pushes have; it fits the stream id's eight bits or the limit is refused)
  MPPO_TRY(check_limit_cfg("mppo_engine_set_time_limit", &lc));
  if (e->graph || e->prepared)
    return fail(MPPO_ESTATE, "mppo_engine_set_time_limit: the update has been prepared already (its launch sequence is fixed, a captured graph holds it): "
                             "set the limit before mppo_engine_prepare and the first mppo_engine_update");
  if (e->was_reset)
    return fail(MPPO_ESTATE, "mppo_engine_set_time_limit: mppo_engine_reset has run already: set the limit before it");
  e->limit = LimitCfg{};
  if (length > 0) e->limit = limit_cfg_of(lc);
  return MPPO_OK;
}

extern "C" int32_t mppo_engine_set_obs_noise(mppo_engine_t* e, const float* scale) {
  MPPO_REQUIRE(e, "mppo_engine_set_obs_noise: null engine");
  MPPO_TRY(check_obs_noise_scale("mppo_engine_set_obs_noise", scale, e->O));
  bool on = false;
  if (scale) for (int j = 0; j < e->O; ++j) on = on || scale[j] > 0.f;
  mppo_obs_noise_cfg_t nc{};
  nc.seed = e->cfg.seed; nc.rank = on ? e->cfg.rank : 0;  // (the engine's own: one stream per rank, as the pushes have; it fits the stream id's eight bits or the noise is refused)
  MPPO_TRY(check_obs_noise_cfg("mppo_engine_set_obs_noise", &nc));
  if (e->graph || e->prepared)
    return fail(MPPO_ESTATE, "mppo_engine_set_obs_noise: the update has been prepared already (its launch sequence is fixed, a captured graph holds it): "
                             "set the noise before mppo_engine_prepare and the first mppo_engine_update");
  if (e->was_reset)
    return fail(MPPO_ESTATE, "mppo_engine_set_obs_noise: mppo_engine_reset has run already (the observation it wrote has its noise or has none): set the noise before it");
  e->obs_noise = false;
  if (on) {  // the table into its region (pad columns 0), before anything is enqueued
    std::vector<float> table((size_t)e->OP, 0.f);
    for (int j = 0; j < e->O; ++j) table[j] = scale[j];
    MPPO_CHECK_HIP(hipMemcpy(e->obs_noise_scale, table.data(), (size_t)e->OP * 4, hipMemcpyHostToDevice));
    e->obs_noise = true;
    e->noise_draw = obs_noise_draw_of(nc);
  }
  return MPPO_OK;
}

extern "C" int32_t mppo_engine_set_action_delay(mppo_engine_t* e, int32_t dmin, int32_t dmax) {
  MPPO_REQUIRE(e, "mppo_engine_set_action_delay: null engine");
  mppo_action_delay_cfg_t dc{};
  dc.min = dmin; dc.max = dmax; dc.seed = e->cfg.seed;
  dc.rank = dmax > 0 ? e->cfg.rank : 0;  // (the engine's own, as above)
  MPPO_TRY(check_action_delay_cfg("mppo_engine_set_action_delay", &dc));
  if (e->graph || e->prepared)
    return fail(MPPO_ESTATE, "mppo_engine_set_action_delay: the update has been prepared already (its launch sequence is fixed, a captured graph holds it): "
                             "set the latency before mppo_engine_prepare and the first mppo_engine_update");
  if (e->was_reset)
    return fail(MPPO_ESTATE, "mppo_engine_set_action_delay: mppo_engine_reset has run already (it empties the ring and writes the latency table): set the latency before it");
  e->delay = DelayDraw{};
  if (dmax > 0) e->delay = delay_draw_of(dc);
  return MPPO_OK;
}

static int32_t require_ready(mppo_engine_t* e, bool needs_comm) {
  MPPO_REQUIRE(e, "null engine");
  if (!e->was_reset) return fail(MPPO_ESTATE, "engine: call mppo_engine_reset before stepping");
  if (needs_comm && e->cfg.world_size > 1 && !e->comm && !peer_connected(e->peer))
    return fail(MPPO_ESTATE, "engine: world_size = %d but neither mppo_engine_comm_init nor mppo_engine_peer_connect was called", e->cfg.world_size);
  return MPPO_OK;
}

extern "C" int32_t mppo_engine_rollout(mppo_engine_t* e, void* stream) {
  // environments are independent: the rollout needs no communication - except for the normalisations' running statistics, which are those of all ranks
  MPPO_TRY(require_ready(e, e && (e->obs_norm || e->reward_norm)));
  return do_rollout(e, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mppo_engine_learn(mppo_engine_t* e, void* stream) {
  MPPO_TRY(require_ready(e, true));
  return do_learn(e, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mppo_engine_graph_active(const mppo_engine_t* e, int32_t* out) {
  MPPO_REQUIRE(e && out, "mppo_engine_graph_active: null argument");
  *out = e->graph ? 1 : 0;
  return MPPO_OK;
}

// RCCL path, first update of several ranks: the ranks agree on whether they replay a graph.  A capture that failed on ONE rank would
// leave that rank launching eagerly while the others replay captured collectives; so every rank contributes its outcome to one eager
// all-reduce and all of them fall back to eager launches if any capture failed.  (The peer-to-peer path needs no such agreement:
// its exchange is made of ordinary kernels and flags, the same whether a rank replays or launches them.)
static int32_t agree_on_graph(mppo_engine_t* e, hipStream_t s) {
  const float mine = e->graph ? 0.f : 1.f;
  MPPO_CHECK_HIP(hipMemcpyAsync(e->flag_ws, &mine, 4, hipMemcpyHostToDevice, s));
  MPPO_TRY(comm_allreduce_f32(e->comm, e->flag_ws, 1, s));
  float sum = 0.f;
  MPPO_CHECK_HIP(hipMemcpyAsync(&sum, e->flag_ws, 4, hipMemcpyDeviceToHost, s));
  MPPO_CHECK_HIP(hipStreamSynchronize(s));
  if (sum != 0.f && e->graph) { graph_destroy(e->graph); e->graph = nullptr; }
  if (sum != 0.f) e->graph_failed = true;
  e->graph_agreed = true;
  return MPPO_OK;
}

static int32_t prepare_update(mppo_engine_t* e, hipStream_t s, bool* replay) {
  e->prepared = true;
  // RCCL path: the all-reduces are captured into the graph together with the kernels only on request (MPPO_GRAPH_COMM=1; it has never
  // run on more than one GPU), by default several ranks with an RCCL communicator launch eagerly.  The peer-to-peer path is captured
  // like any sequence of kernels.
  const char* gc = getenv("MPPO_GRAPH_COMM");  // (read at every call: a process may hold engines of both kinds)
  const bool graph_comm = gc && gc[0] == '1';
  const bool with_peer = peer_connected(e->peer);
  const bool with_comm = !with_peer && (e->cfg.world_size > 1 || e->comm);
  const bool want_graph = e->cfg.use_graph && !e->graph_failed && s != nullptr && (!with_comm || graph_comm);
  if (want_graph) {
    if (!e->graph) {
      // capture once; every pointer and size in the sequence is fixed by the arena layout
      if (graph_begin(s, with_comm) == MPPO_OK) {
        int32_t r = do_rollout(e, s);
        if (r == MPPO_OK) r = do_learn(e, s);
        const int32_t r2 = graph_end(s, &e->graph);
        if (r != MPPO_OK || r2 != MPPO_OK) { e->graph = nullptr; e->graph_failed = true; }
      } else {
        e->graph_failed = true;
      }
      if (with_comm && e->cfg.world_size > 1 && !e->graph_agreed) MPPO_TRY(agree_on_graph(e, s));
    }
  }
  *replay = want_graph && e->graph;
  return MPPO_OK;
}

extern "C" int32_t mppo_engine_update(mppo_engine_t* e, void* stream) {
  MPPO_TRY(require_ready(e, true));
  hipStream_t s = static_cast<hipStream_t>(stream);
  bool replay = false;
  MPPO_TRY(prepare_update(e, s, &replay));
  if (replay) return graph_launch(e->graph, s);
  MPPO_TRY(do_rollout(e, s));
  return do_learn(e, s);
}

// Everything mppo_engine_update does BEFORE it enqueues work: the one-time capture of the update into a hipGraph (which also loads
// the kernels' code objects).  With several ranks the caller puts a host-side barrier between this call and the first update, so
// that the ranks start their first exchange within milliseconds of each other instead of a capture time apart.
extern "C" int32_t mppo_engine_prepare(mppo_engine_t* e, void* stream) {
  MPPO_TRY(require_ready(e, true));
  bool replay = false;
  return prepare_update(e, static_cast<hipStream_t>(stream), &replay);
}

// ---- peer-to-peer gradient exchange (peer.h): every rank exports its exchange buffer, the caller gathers the 64-byte handles of all
// ranks (rank order) and hands them to every rank; a host-side barrier between the last connect and the first update is the caller's.
extern "C" int32_t mppo_engine_peer_export(mppo_engine_t* e, void* handle64) {
  MPPO_REQUIRE(e && handle64, "mppo_engine_peer_export: null argument");
  MPPO_REQUIRE(!e->peer, "mppo_engine_peer_export: already exported");
  MPPO_REQUIRE(e->cfg.world_size >= 2, "mppo_engine_peer_export: one rank has nobody to exchange with");
  const size_t adv = (size_t)e->E * e->M * 2;
  // (the self-test sums four values; the gather's region holds one rank's sums of both normalisations, whether or not they are on: the order of this call and
  // mppo_engine_set_*_norm does not matter)
  return peer_create(e->cfg.rank, e->cfg.world_size, (size_t)e->P, adv < 4 ? 4 : adv, 2 * ((size_t)e->O + 1), &e->peer, handle64);
}

extern "C" int32_t mppo_engine_peer_connect(mppo_engine_t* e, const void* handles, int32_t shared_device) {
  MPPO_REQUIRE(e && handles && e->peer, "mppo_engine_peer_connect: call mppo_engine_peer_export first");
  MPPO_REQUIRE(!e->graph, "mppo_engine_peer_connect: the update has been captured already");
  return peer_connect(e->peer, handles, shared_device);
}

// Everything the gradient path depends on, once, on known inputs, before anything depends on it:
//  1. the once-per-update all-reduce of the advantage sums: every rank publishes (rank + 1) four times, waits for the peers' values and
//     adds them in rank order (scalar system-scope stores / loads, the adv_done flags);
//  1b. the once-per-update gather of the normalisations' sums, in the engine's shape: slot r = (r + 1) c(i); every rank checks every slot EXACTLY (the gat_done
//     flags, the gather's own epoch and region);
//  2. ONE full optimizer step's exchange in the form the engine will launch it (fused / split / shared): a known local gradient
//     g_r[i] = (r + 1) c(i), c(i) a multiple of 1/256, goes into `pub` through the publish kernel (16-byte system-scope stores, the
//     arrival counter, the wg_done flags), then clip_adam<PEER> on SCRATCH parameters and moments: phase A pulls this rank's slice of
//     every rank's `pub`, reduces, pushes it into every rank's `red` with its sums of squares and raises red_done; phase B waits for
//     all pieces and applies Adam.  Checked on every rank: red == c(i) G (G + 1) / 2 EXACTLY for all i, the sums of squares, and the
//     scratch first moment (what phase B read).
// *ok = 0: a wait ran into its time limit or a value is wrong (the mapping was made but stores from / to a peer do not arrive, or arrive
// out of order): the caller drops the exchange on all ranks and continues on RCCL (Trainer.init_comm).
__host__ __device__ static inline float selftest_pattern(size_t i) { return (float)((int)(((unsigned)i * 2654435761u) >> 24) - 128) / 256.f; }

// the soak behind the first, fully checked exchange (below): step after step a known local gradient (rank + 1) f c(i), f = 1 .. 4 changing with
// the step, goes through the exchange in the form the engine will launch it, and every element of the reduced gradient this rank reads is
// compared ON THE DEVICE with its exact value f c(i) G (G + 1) / 2 (multiples of 1/256: every partial sum is exact, whatever the order)
__global__ void selftest_fill_kernel(float* __restrict__ g, size_t P, float rank1, float f) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += (size_t)gridDim.x * blockDim.x) g[i] = rank1 * f * selftest_pattern(i);
}
__global__ void selftest_check_kernel(const float* __restrict__ red_pairs, size_t P, float tri, float f, int* __restrict__ bad) {
  int n = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += (size_t)gridDim.x * blockDim.x) n += (int)(sys_load_f32(red_pairs + 2 * i) != tri * f * selftest_pattern(i));
  if (n) atomicAdd(bad, n);
}

extern "C" int32_t mppo_engine_peer_selftest(mppo_engine_t* e, void* stream, int32_t* ok) {
  MPPO_REQUIRE(e && ok && peer_connected(e->peer), "mppo_engine_peer_selftest: no connected exchange");
  MPPO_REQUIRE(!e->graph, "mppo_engine_peer_selftest: the update has been captured already");
#ifndef MPPO_EMU
  // Engines of ONE process wait for each other inside this call (every rank's self-test kernels poll the peers' flags): on the legacy
  // default stream - which synchronises with every other blocking stream of the process - the ranks would serialise, every wait would
  // run into its limit and the job would fall back to RCCL without anybody having said why (round-4 advisor).  Refused instead.
  MPPO_REQUIRE(!peer_has_local(e->peer) || (stream != nullptr && stream != static_cast<void*>(hipStreamLegacy)),
               "mppo_engine_peer_selftest: a peer engine lives in this process - every engine needs a stream of its own (not the default stream), "
               "and its self-test a thread of its own");
#endif
  *ok = 0;
  const int G = e->cfg.world_size;
  const size_t P = (size_t)e->P;
  double host[4], *dev = nullptr;
  for (double& x : host) x = (double)(e->cfg.rank + 1);
  float* scratch = nullptr;  // g | p | m | v, [P] each
  MPPO_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&dev), sizeof(host)));
  hipError_t he = hipMalloc(reinterpret_cast<void**>(&scratch), 4 * P * sizeof(float));
  if (he != hipSuccess) { (void)hipFree(dev); return fail(MPPO_EHIP, "mppo_engine_peer_selftest: %s", hipGetErrorString(he)); }
  std::vector<float> g(P), red(2 * (P + kSqSlots)), m1(P);  // red: (value, epoch) pairs as they travel (peer.h)
  for (size_t i = 0; i < P; ++i) g[i] = (float)(e->cfg.rank + 1) * selftest_pattern(i);
  int32_t rc = MPPO_OK, timed_out = 0;
  int soak_bad = 0;
  // exchanges of the soak: 2 000 by default (about 50 ms on distinct GPUs); MPPO_PEER_SOAK=<n> overrides, 0 = the single checked exchange only
#ifdef MPPO_EMU
  int soak = 6;  // (emulated ranks are slow)
#else
  int soak = 2000;
#endif
  if (const char* sv = getenv("MPPO_PEER_SOAK")) soak = atoi(sv) < 0 ? 0 : atoi(sv);
  // the gather of the normalisations' sums in the shape the engine launches it ([G][2 O] and [G][2] slots): slot r = (r + 1) c(i), every other slot a
  // value no rank publishes until its owner's bits arrive
  const int gn0 = 2 * e->O, gn1 = 2;
  const size_t goff1 = (size_t)G * gn0;
  auto gslot = [&](int q, int i) -> size_t { return i < gn0 ? (size_t)q * gn0 + i : goff1 + (size_t)q * gn1 + (i - gn0); };
  std::vector<double> gat((size_t)G * (gn0 + gn1), -7.0);
  for (int i = 0; i < gn0 + gn1; ++i) gat[gslot(e->cfg.rank, i)] = (double)(e->cfg.rank + 1) * (double)selftest_pattern((size_t)i);
  double* gdev = nullptr;
  he = hipMalloc(reinterpret_cast<void**>(&gdev), gat.size() * sizeof(double));
  if (he != hipSuccess) { (void)hipFree(dev); (void)hipFree(scratch); return fail(MPPO_EHIP, "mppo_engine_peer_selftest: %s", hipGetErrorString(he)); }
  he = hipMemcpy(gdev, gat.data(), gat.size() * sizeof(double), hipMemcpyHostToDevice);
  if (he == hipSuccess) he = hipMemcpy(dev, host, sizeof(host), hipMemcpyHostToDevice);
  if (he == hipSuccess) he = hipMemcpy(scratch, g.data(), P * sizeof(float), hipMemcpyHostToDevice);
  if (he == hipSuccess) he = hipMemset(scratch + P, 0, 3 * P * sizeof(float));
  mppo_adam_cfg_t ac = e->cfg.adam;
  ac.anneal = 0; ac.sched_div = 1; ac.num_updates = 1;
  // on the CALLER's stream (the one its updates will run on): several engines of one process (one per GPU, or ranks sharing a GPU in the
  // tests) run their self-tests at the same time and each one's kernels wait for the others' - streams they shared would block them all.
  // (A stream created here costs more than it looks: measured on a GPU shared by two rank processes, one extra stream per process
  // - even destroyed again - slowed every later update from 11.7 to 27.8 ms.)
  hipStream_t st = static_cast<hipStream_t>(stream);
  // the self-test answers in milliseconds when the transport works; when it does not, ten seconds are enough to say so (the run-time limit
  // of a wait, MPPO_PEER_TIMEOUT_MS, is sized for host-side skew between ranks in the middle of a job: a minute by default)
  const unsigned long long limit_ms = peer_set_limit_ms(e->peer, 0.0);
#ifndef MPPO_EMU  // (emulated ranks are slow and share the host's cores: they keep the run-time limit)
  if (limit_ms > 10000ull) peer_set_limit_ms(e->peer, 10000.0);
#endif
  if (he == hipSuccess) {
    rc = peer_allreduce_f64(e->peer, dev, 4, st);
    if (rc == MPPO_OK) rc = peer_gather_f64(e->peer, gdev, gn0, goff1, gn1, st);
    const PeerStep ps = peer_step(e->peer, 0);
    if (rc == MPPO_OK) rc = peer_publish(e->peer, scratch, P, 0, st);
    if (rc == MPPO_OK)
      rc = clip_adam(P, scratch + P, scratch + 2 * P, scratch + 3 * P, peer_red(e->peer), e->count, 0, ac, const_cast<float*>(peer_red(e->peer)) + P, true, st, nullptr, &ps);
    if (rc == MPPO_OK) rc = peer_advance(e->peer, 1, st);
    if (rc == MPPO_OK) rc = peer_status(e->peer, &timed_out, nullptr);  // synchronises
    if (rc == MPPO_OK) he = hipMemcpy(host, dev, sizeof(host), hipMemcpyDeviceToHost);
    if (rc == MPPO_OK && he == hipSuccess) he = hipMemcpy(gat.data(), gdev, gat.size() * sizeof(double), hipMemcpyDeviceToHost);
    if (rc == MPPO_OK && he == hipSuccess) he = hipMemcpy(red.data(),peer_red(e->peer), 2 * (P + kSqSlots) * sizeof(float), hipMemcpyDeviceToHost);
    if (rc == MPPO_OK && he == hipSuccess) he = hipMemcpy(m1.data(), scratch + 2 * P, P * sizeof(float), hipMemcpyDeviceToHost);
    // ---- the soak (round 6): ONE exchange on known values finds a transport that carries no stores; it does not find a pair torn or a store
    // reordered once in 10^5.  `soak` more exchanges follow back to back at the rate of training (no host in between), every element checked
    // on the device; every rank runs the same number (the ranks wait for each other inside every step).
    if (rc == MPPO_OK && he == hipSuccess && !timed_out && soak > 0) {
      he = hipMemsetAsync(dev, 0, sizeof(int), st);
      for (int sidx = 0; sidx < soak && rc == MPPO_OK && he == hipSuccess; ++sidx) {
        const float f = (float)(1 + (sidx & 3));
        hipLaunchKernelGGL(selftest_fill_kernel, dim3(256), dim3(256), 0, st, scratch, P, (float)(e->cfg.rank + 1), f);
        const PeerStep ps2 = peer_step(e->peer, 0);
        rc = peer_publish(e->peer, scratch, P, 0, st);
        if (rc == MPPO_OK)
          rc = clip_adam(P, scratch + P, scratch + 2 * P, scratch + 3 * P, peer_red(e->peer), e->count, 0, ac, const_cast<float*>(peer_red(e->peer)) + P, true, st, nullptr, &ps2);
        if (rc == MPPO_OK) {
          hipLaunchKernelGGL(selftest_check_kernel, dim3(256), dim3(256), 0, st, peer_red(e->peer), P, 0.5f * (float)G * (float)(G + 1), f, reinterpret_cast<int*>(dev));
          he = hipGetLastError();
        }
        if (rc == MPPO_OK) rc = peer_advance(e->peer, 1, st);
      }
      if (rc == MPPO_OK && he == hipSuccess) rc = peer_status(e->peer, &timed_out, nullptr);  // synchronises
      if (rc == MPPO_OK && he == hipSuccess) he = hipMemcpy(&soak_bad, dev, sizeof(int), hipMemcpyDeviceToHost);
    }
  }
  peer_set_limit_ms(e->peer, (double)limit_ms);
  (void)hipFree(dev);
  (void)hipFree(gdev);
  (void)hipFree(scratch);
  if (he != hipSuccess) return fail(MPPO_EHIP, "mppo_engine_peer_selftest: %s", hipGetErrorString(he));
  if (rc != MPPO_OK) return rc;
  bool good = !timed_out;
  for (int q = 0; q < G && good; ++q)  // the gather: every rank's slot, bit for bit what its owner published
    for (int i = 0; i < gn0 + gn1 && good; ++i) good = gat[gslot(q, i)] == (double)(q + 1) * (double)selftest_pattern((size_t)i);
  if (timed_out)  // say WHY the job is about to continue on RCCL: a wait ran into the self-test's limit, as opposed to a wrong value
    fprintf(stderr, "[minppo_amd] warning: rank %d: the peer exchange's connect-time self-test timed out (%d wait(s) gave up after %llu ms) - a peer did not "
                    "answer in time (a rank that started late, ranks serialised on a shared stream, or a mapping that carries no stores); the caller falls back to RCCL\n",
            e->cfg.rank, (int)timed_out, (unsigned long long)(limit_ms > 10000ull ? 10000ull : limit_ms));
  for (double x : host) good = good && x == 0.5 * G * (G + 1);
  const float tri = 0.5f * (float)G * (float)(G + 1);
  double ss = 0.0, ss_dev = 0.0;
  for (size_t i = 0; i < P && good; ++i) {
    const float want = tri * selftest_pattern(i);  // (multiples of 1/256 below 2^24: every partial sum is exact in float32)
    good = red[2 * i] == want;
    ss += (double)want * (double)want;
  }
  for (int k = 0; k < kSqSlots; ++k) ss_dev += (double)red[2 * (P + k)];
  good = good && fabs(ss_dev - ss) <= 1e-4 * ss + 1e-12;
  // phase B: first moment of the scratch state = (1 - b1) * clip scale * reduced gradient
  const double norm = sqrt(ss), scale = norm < (double)ac.max_grad_norm ? 1.0 : (double)ac.max_grad_norm / norm;
  for (size_t i = 0; i < P && good; ++i) {
    const double want = (1.0 - (double)ac.b1) * scale * (double)tri * (double)selftest_pattern(i);
    good = fabs((double)m1[i] - want) <= 1e-4 * fabs(want) + 1e-12;
  }
  if (good && soak_bad != 0) {
    fprintf(stderr, "[minppo_amd] warning: rank %d: the peer exchange passed its first checked step and then delivered %d wrong value(s) in %d more exchanges "
                    "(a torn or reordered store); the caller falls back to RCCL\n", e->cfg.rank, soak_bad, soak);
    good = false;
  }
  *ok = good ? 1 : 0;
  return MPPO_OK;
}

extern "C" int32_t mppo_engine_peer_latency(mppo_engine_t* e, int32_t other_rank, int32_t iters, int32_t initiator, void* stream, double* one_way_us) {
  MPPO_REQUIRE(e && peer_connected(e->peer), "mppo_engine_peer_latency: no connected exchange");
  return peer_latency(e->peer, other_rank, iters, initiator, static_cast<hipStream_t>(stream), one_way_us);
}

// drops the exchange (a self-test failed on some rank): the engine is back to "no transport", mppo_engine_comm_init may follow
extern "C" int32_t mppo_engine_peer_disable(mppo_engine_t* e) {
  MPPO_REQUIRE(e, "mppo_engine_peer_disable: null argument");
  MPPO_REQUIRE(!e->graph, "mppo_engine_peer_disable: the update has been captured already");
  peer_destroy(e->peer);
  e->peer = nullptr;
  return MPPO_OK;
}

extern "C" int32_t mppo_engine_comm_mode(const mppo_engine_t* e, int32_t* out) {
  MPPO_REQUIRE(e && out, "mppo_engine_comm_mode: null argument");
  *out = peer_connected(e->peer) ? 2 + peer_mode(e->peer) : (e->comm ? 1 : 0);
  return MPPO_OK;
}

extern "C" int32_t mppo_engine_peer_status(const mppo_engine_t* e, int32_t* timed_out, int32_t* info8) {
  MPPO_REQUIRE(e && timed_out, "mppo_engine_peer_status: null argument");
  *timed_out = 0;
  if (info8) for (int k = 0; k < 8; ++k) info8[k] = 0;
  if (!e->peer) return MPPO_OK;
  return peer_status(e->peer, timed_out, info8);
}
