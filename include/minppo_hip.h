/*
 * minppo_hip.h — C ABI of libminppo_hip.so, the MI355X (gfx950) engine behind the
 * minppo train / env surface.
 *
 * The reference (kscalelabs/minppo @ 2024-10-16) exposes NO FFI / plugin interface: its hot
 * path is one jitted JAX program reached through plain Python callables.  The
 * entry points below are therefore the boundary a maintainer would bind (ctypes / cffi ABI
 * mode) to replace the stages of that program; each one cites the
 * reference lines it replaces.  All paths are relative to /root/reference/.
 *
 * Conventions
 *   - every function returns 0 (MPPO_OK) or a negative MPPO_E* code; the message of the last
 *     failure on the calling thread is returned by mppo_last_error().
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  No function
 *     allocates device memory, synchronises the host with the device or touches the default
 *     stream behind the caller's back, unless stated.  Device pointers are owned by the caller
 *     (torch tensors) and must outlive the enqueued work.
 *   - all device arrays are float32 unless stated; matrices are row-major.
 *   - flat parameter vector layout (P = 2(O*H + H + H*H + H) + H*A + 2A + H + 1 parameters):
 *       actor : W1[O,H] b1[H] W2[H,H] b2[H] W3[H,A] b3[A]  log_std[A]
 *       critic: W1[O,H] b1[H] W2[H,H] b2[H] W3[H,1] b3[1]
 *     (`kernel [in,out]`, `bias [out]`: the Flax layout of train.py:63,68; two hidden layers,
 *     config.py:53.)  Every tensor starts at the next multiple of 4 floats (16 bytes), whatever
 *     A is; the alignment words in between hold zeros in the parameter, gradient and moment
 *     vectors.  mppo_param_count() is the length including them.
 *   - trajectories are time-major [T,N,...]; flat sample index = t*N + n (train.py:260).
 *   - observation rows are padded to OP = round_up(O, 4) floats (pad = 0) so that every row
 *     starts 16-byte aligned.
 */
#ifndef MINPPO_HIP_H
#define MINPPO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPPO_OK 0
#define MPPO_EINVAL (-1)   /* bad argument / shape the kernels do not support            */
#define MPPO_EHIP (-2)     /* a HIP runtime call failed (message has hipGetErrorString)   */
#define MPPO_EMODEL (-3)   /* malformed model blob                                        */
#define MPPO_ESTATE (-4)   /* call order violated (e.g. update before reset)              */
#define MPPO_ENCCL (-5)    /* an RCCL call failed                                         */
#define MPPO_ENOMEM (-6)   /* caller-provided workspace too small                         */

#define MPPO_ABI_VERSION 7  /* 7: mppo_model_attach_kernel (an environment kernel compiled for the robot at run time); 6: mppo_model_scratch_bytes (a large robot's matrices in global memory); 5: mppo_minibatch_rows_per_workgroup; a bf16 network's fragment copies are tile-major (4: mppo_engine_peer_selftest runs on the caller's stream) */

const char* mppo_last_error(void);
int32_t mppo_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * Robot model.  Replaces `load_mjcf_model` + `mjcf.load_model` + the solver override
 * (minppo/env.py:27-50, 94-100): the host compiles an MJCF-like description into one
 * little-endian blob of 4-byte words (minppo_amd/model.py: _to_blob documents the layout);
 * the same bytes must be resident in device memory at `dev_blob` for the model's lifetime.
 * ---------------------------------------------------------------------------------------- */
typedef struct mppo_model mppo_model_t;

typedef struct mppo_model_dims {
  int32_t nq, nv, nu, nbody, njnt, ncon, nlimit, nefc;
  int32_t obs_dim;      /* O  = nq + 2 nv + 16 (nbody-1)     (env.py:245-253, include_c_vals) */
  int32_t obs_pad;      /* OP = round_up(O, 4)                                                */
  int32_t rec_dim;      /* floats per env in the persistent state record                      */
  int32_t lds_bytes;    /* dynamic LDS of one env_step workgroup                              */
  float timestep;
} mppo_model_dims_t;

int32_t mppo_model_open(const void* host_blob, size_t nbytes, const void* dev_blob, mppo_model_t** out);
int32_t mppo_model_close(mppo_model_t* m);
int32_t mppo_model_get_dims(const mppo_model_t* m, mppo_model_dims_t* out);
/* *out = 1 when this model's dimensions match one of the environment-kernel instantiations compiled for fixed dimensions
 * (csrc/spec_dims.inc, written by `python -m minppo_amd.build`; MPPO_SPECIALIZE=robot.xml[,...] adds models), 0 when it runs the
 * run-time-sized kernel.  Same results either way; the fixed-size kernel is faster (env_kernel). */
int32_t mppo_model_is_specialized(const mppo_model_t* m, int32_t* out);
/* Attaches a gfx950 code object that holds the environment kernel compiled for exactly this robot's dimensions - the build-time
 * MPPO_SPECIALIZE at run time, for a robot the library was not built for (`minppo_amd/jit.py` makes one: hipcc, device side only, of
 * csrc/k_physics.hip with a one-robot list, cached by the hash of the kernel sources and the dimensions).  What it replaces in the
 * reference: `jax.jit` of the environment step (env.py:123,147 `@partial(jax.jit, ...)` on reset / step, train.py:133,138,306: XLA
 * compiles them for the loaded robot's shapes at start-up).  `names[0..2]`: the symbols of the kernel's three modes (reset, step, probe) - their mangled names must
 * spell this model's dimensions (the step's and the probe's instantiations under an external wrench, mppo_env_step_xfrc below, are looked up in the same object
 * under those two names with the mode's digit 1 / 2 replaced by 3 / 4: an object without them is refused); `regchol_max_nv`: the MPPO_REGCHOL_MAX_NV the object was compiled with (48 by default: its LDS layout
 * follows from it).  The object must carry the library's `mppo_env_kernel_tag` (argument-struct sizes, blob version).  Before it is
 * used, a reset and four steps of 24 environments must equal the run-time-sized kernel's bit for bit on this device.  *used = 1: the
 * model now runs the attached kernel (mppo_model_is_specialized reports 2); *used = 0 with MPPO_OK: it does not - the library has an
 * instantiation for this robot already, MPPO_ENV_GENERIC / MPPO_ENV_SPILL are set, the robot is too large for four environments per
 * wave, or the kernel failed the comparison (a message on stderr) - and the model is as it was.  Call before the model is handed to an
 * engine (mppo_model_get_dims().lds_bytes and mppo_model_scratch_bytes change with the kernel). */
int32_t mppo_model_attach_kernel(mppo_model_t* m, const void* image, size_t nbytes, const char* const* names, int32_t regchol_max_nv, int32_t* used);
/* Bytes of global memory the environment kernel uses beside the state for N environments: 0 for a robot whose per-environment working set
 * fits LDS four waves to a CU; a larger robot (about 30 dofs / 20 contact slots and up) keeps its mass matrix and contact Jacobian in
 * per-environment records there (L2 / Infinity-Cache resident).  mppo_env_reset / mppo_env_step / mppo_physics_forward
 * allocate them on demand inside the handle (hipMalloc, grown when N grows, freed by mppo_model_close; not during a stream capture, and
 * one stream at a time may launch through such a handle); an engine takes them from its arena (mppo_engine_arena_bytes includes them). */
int32_t mppo_model_scratch_bytes(const mppo_model_t* m, int32_t N, size_t* out);

/* Reward / termination constants read by compute_reward and is_done (env.py:199-242,
 * config.py:36-48). */
typedef struct mppo_reward_cfg {
  float height_min_z, height_max_z;
  float exp_coefficient, subtraction_factor, max_diff_norm;
  float w_ctrl_cost, w_original_pos, w_is_healthy, w_velocity;
} mppo_reward_cfg_t;

/* Per-env episode bookkeeping, `EnvMetrics` (env.py:53-59), structure-of-arrays, each [N]. */
typedef struct mppo_env_metrics {
  float* episode_returns;
  int32_t* episode_lengths;
  float* returned_episode_returns;
  int32_t* returned_episode_lengths;
  int32_t* timestep;
  uint8_t* returned_episode;
} mppo_env_metrics_t;

/* Persistent per-env record, [N, rec_dim] floats:
 *   [0,O)        the observation of this state: qpos, qvel, cinert[1:], cvel[1:], qfrc_actuator
 *                (derived fields are those of the forward pass that produced the state, env.py:245-261)
 *   [OP,OP+nv)   qacc_warmstart
 *   OP+nv        subtree_com[1].x  (env.py:222-223)     OP+nv+1  time
 * `reset_rec` [rec_dim] is the constant reset state (reset_noise_scale = 0, env.py:87,115-121).
 *
 * mppo_env_reset : `HumanoidEnv.reset` vmapped over N (env.py:124-145; train.py:133-143):
 *                  pipeline_init at qpos0 / zero velocity / zero ctrl, zero metrics, obs [N,OP].
 * mppo_env_step  : `HumanoidEnv.step` vmapped over N (env.py:148-196; train.py:138-140,165):
 *                  n_frames x mjx.step, pre-step observation, reward, done (height or NaN),
 *                  auto-reset, metrics.  action is [N, act_ld] with nu valid columns. */
int32_t mppo_env_reset(const mppo_model_t* m, int32_t N, float* state, float* reset_rec, float* obs, int32_t obs_ld,
                       float* reward, uint8_t* done, const mppo_env_metrics_t* metrics, void* stream);
int32_t mppo_env_step(const mppo_model_t* m, int32_t N, int32_t n_frames, const mppo_reward_cfg_t* rc, float* state,
                      const float* reset_rec, const float* action, int32_t act_ld, float* obs, int32_t obs_ld,
                      float* reward, uint8_t* done, const mppo_env_metrics_t* metrics, void* stream);
/* mppo_env_reinit : `_get_reset_state` with reset_noise_scale = `scale` > 0 (env.py:115-121) for the environments `mask` names ([N] bytes in
 *                   device memory, non-zero: reset; NULL: every environment): qpos = qpos0 + U(-scale, scale) on all nq words (quaternion words
 *                   too, left unnormalised as MJX leaves them), qvel = U(-scale, scale), ctrl = 0, warm start 0, then pipeline_init's one forward
 *                   pass.  Writes the state rows and (obs may be NULL) the observation rows of those environments and nothing else: after a
 *                   mppo_env_step with mask = its `done` it turns the step's constant-record restarts into the reference's randomised ones.  A
 *                   workgroup without a masked-in environment leaves before it loads the model.  scale = 0: the plain reset's rows.
 *                   The noise is drawn inside the kernel, per environment and element, from one of two streams:
 *   rng_impl 1      the reference's threefry tree: key_n = split(K, N)[n]; r1, r2 = split(key_n); uniform(r1, (nq,)), uniform(r2, (nv,))
 *                   (train.py:135,164; env.py:116-119; conventions of minppo_amd/jaxrng.py), K = key2[0..1] in DEVICE memory: the reset key
 *                   (train.py:142) or a step key (train.py:163).  seed / rank / counter are not read.
 *   rng_impl 2      the same with the environments' keys given: key2 = [N][2] words, key_n = key2[n] (the `step_rngs` of train.py:164)
 *   rng_impl 0      the engine's Philox4x32-10: element i (0 .. nq - 1: qpos, then qvel) of environment n at event c is word i & 3 of
 *                   philox(counter = {n, c, lo(S + (i >> 2)), hi(S)}, key = seed) with S = ("RESET" << 24) + (rank << 16) and the event
 *                   c = (counter ? *counter : 0) + counter_offset, `counter` a word in DEVICE memory that the caller advances there (so that a
 *                   replayed hipGraph draws fresh values).  key2 is not read.
 *                   Bits become a float as jax.random.uniform makes one: (bits >> 9 | 0x3f800000) - 1, times 2 scale, minus scale, clamped below. */
int32_t mppo_env_reinit(const mppo_model_t* m, int32_t N, float* state, float* obs, int32_t obs_ld, const uint8_t* mask, float scale,
                        int32_t rng_impl, uint64_t seed, int32_t rank, const uint32_t* key2, const int32_t* counter, int32_t counter_offset,
                        void* stream);
/* Debug / parity probe: one mjx.forward on caller-given (qpos,qvel,ctrl,qacc_warmstart) [N,*]
 * with every intermediate the parity tests compare exported.  Any output pointer may be NULL.
 * M [N,nv,nv]; efc_* [N,nefc]; J [N,nefc,nv]; cinert [N,nbody,10]; cvel [N,nbody,6]. */
typedef struct mppo_forward_probe {
  float *qM, *qfrc_bias, *qfrc_passive, *qfrc_actuator, *qacc_smooth, *efc_J, *efc_D, *efc_aref, *qacc, *cinert, *cvel,
      *subtree_com1, *xpos, *qacc_euler;
  int32_t* solver_niter;
} mppo_forward_probe_t;
int32_t mppo_physics_forward(const mppo_model_t* m, int32_t N, const float* qpos, const float* qvel, const float* ctrl,
                             const float* qacc_warmstart, const mppo_forward_probe_t* out, void* stream);

/* ---- random pushes: an external wrench on one body --------------------------------------------------------------------------
 * What MJX calls `xfrc_applied` (Brax: `pipeline_state.xfrc_applied` before `pipeline_step`), for ONE body per launch: a force and a torque in
 * world axes acting at the body's centre of mass `xipos[body]`, added to qfrc_smooth as `support.xfrc_accumulate` adds it inside
 * `forward.fwd_acceleration`:
 *     qfrc_smooth[d] += cdof[d] . (torque + (xipos[body] - subtree_com[root(body)]) x force, force)
 * for every dof d of `body` and of its ancestors, and for no other dof.  The wrench is constant over the n_frames frames of an env step.  It
 * changes qfrc_smooth and what follows from it (qacc_smooth, the solver's input, the Euler solve); qfrc_actuator, the observation of the
 * pre-step state, the reward's control cost and the NaN guard see it only through the state it produces.  The reset is never pushed.
 *
 * mppo_env_step_xfrc : mppo_env_step with `xfrc` [N][6] floats in DEVICE memory - per environment force (3) then torque (3) - acting on `body`
 *                   (1 .. nbody - 1; MPPO_EINVAL otherwise).  xfrc = NULL: exactly mppo_env_step, launch and bits (`body` is then not read); an
 *                   all-zero row leaves its environment's bits what the unpushed step gives.
 * mppo_physics_forward_xfrc : the probe mppo_physics_forward with the same two arguments: qacc_smooth, efc_aref, qacc and qacc_euler are those
 *                   under the wrench; qM, qfrc_bias, qfrc_passive, qfrc_actuator, the poses and cinert / cvel do not depend on it. */
int32_t mppo_env_step_xfrc(const mppo_model_t* m, int32_t N, int32_t n_frames, const mppo_reward_cfg_t* rc, float* state,
                           const float* reset_rec, const float* action, int32_t act_ld, float* obs, int32_t obs_ld,
                           float* reward, uint8_t* done, const mppo_env_metrics_t* metrics, int32_t body, const float* xfrc, void* stream);
int32_t mppo_physics_forward_xfrc(const mppo_model_t* m, int32_t N, const float* qpos, const float* qvel, const float* ctrl,
                                  const float* qacc_warmstart, const mppo_forward_probe_t* out, int32_t body, const float* xfrc, void* stream);
/* The random draw (csrc/push.h; host statement minppo_amd/jaxrng.py push_wrench_philox).  Stateless - a function of (seed, rank, environment,
 * step) alone, so nothing is added to the state record or to a checkpoint.  With S = ("PUSH" << 24) + (rank << 16), for local environment n:
 *     phase_n = word 0 of philox(counter = {n, 0xFFFFFFFF, lo(S), hi(S)}, key = seed) mod interval
 *     pushed at step s  iff  (s + phase_n) mod interval < duration;   window k = (s + phase_n) / interval      (uint32 arithmetic)
 *     fx, fy = uniform(word 0 / word 1 of philox({n, k, lo(S), hi(S)}, seed), -force, force);   fz = 0, torque = 0
 * bits -> float as in mppo_env_reinit.  Every environment is pushed on exactly `duration` of any `interval` consecutive steps, out of phase
 * with the others, by a horizontal force uniform on a square that holds for the whole window - across an episode's auto-reset too.  An
 * environment that is not pushed gets exact zeros.  The stream is the engine's Philox under both rng_impl values (the reference has no pushes).
 * Refused (MPPO_EINVAL): a negative or NaN force, interval < 1, duration outside 1 .. interval, rank outside 0 .. 255, and - wherever a model
 * is at hand - a body outside 1 .. nbody - 1.  force = 0 is "off" everywhere, and then nothing else of the configuration is read or refused.
 *
 * mppo_push_fill  : writes xfrc [N][6] (device) of step s = (counter ? *counter : 0) * counter_mul + counter_add, `counter` a word in DEVICE
 *                   memory (NULL: 0) read when the launch runs.  `body` is not read.  One launch, no workspace. */
typedef struct mppo_push_cfg {
  int32_t body, interval, duration, rank;
  float force;
  uint64_t seed;
} mppo_push_cfg_t;
int32_t mppo_push_fill(const mppo_push_cfg_t* cfg, int32_t N, const int32_t* counter, int32_t counter_mul, int32_t counter_add, float* xfrc,
                       void* stream);

/* ---- episode time limit: truncation --------------------------------------------------------------------------------------------
 * The reference has none (env.py:238-242 ends an episode on height only), so a policy that stands never finishes an episode: the episode statistics
 * dry up exactly when training succeeds, and randomised starts (reset noise, pushes) are seen once.  Brax's `EpisodeWrapper(episode_length)`,
 * legged_gym and MuJoCo Playground train with a limit and treat reaching it as a TRUNCATION, not a failure; so does this (csrc/limit.h, k_limit.hip).
 *
 * mppo_env_time_limit : one launch behind mppo_env_step (no change to the step kernel).  Environment n is truncated iff its episode did not end in that
 *     step (done[n] == 0) and either metrics->episode_lengths[n] (post-step) >= length, or `stagger` is set, metrics->timestep[n] == episode_lengths[n]
 *     (still its first episode since the reset) and episode_lengths[n] == first_n, where
 *         first_n = 1 + (word 0 of philox(counter = {n, 0xFFFFFFFE, lo(S), hi(S)}, key = seed) mod length),   S = ("LIMIT" << 24) + (rank << 16)
 *     in uint32 arithmetic (host statement: minppo_amd/jaxrng.py time_limit_first_philox).  Stagger shortens only the first episode of each environment,
 *     so that a batch does not reach the limit in the same step for ever (legged_gym randomises episode_length_buf for the same reason); the draw is
 *     stateless, nothing is added to the state record or to a checkpoint.  A truncated environment gets exactly what the step kernel writes for an ended
 *     episode: done = 1, truncated = 1, returned_episode_returns = episode_returns, returned_episode_lengths = episode_lengths, returned_episode = 1,
 *     episode_returns = 0, episode_lengths = 0, its state row = reset_rec (rec_dim words) and - obs may be NULL - its observation row = the record's first
 *     OP words.  reward and timestep stay.  Every other environment keeps every bit, and its `truncated` byte is written 0.  An environment that fell in
 *     exactly that step is a termination: its lengths are 0 already.  Fixed order, no atomics, one writer per word.
 *     MPPO_EINVAL: length < 1 (0 means "no limit" wherever a configuration is stored: there is then nothing to launch), rank outside 0 .. 255,
 *     metrics without the five episode arrays (and `timestep` under stagger), obs_ld below the padded observation width. */
typedef struct mppo_time_limit_cfg {
  int32_t length, stagger, rank, reserved;
  uint64_t seed;
} mppo_time_limit_cfg_t;
int32_t mppo_env_time_limit(const mppo_model_t* m, int32_t N, const mppo_time_limit_cfg_t* cfg, float* state, const float* reset_rec, float* obs, int32_t obs_ld,
                            uint8_t* done, uint8_t* truncated, const mppo_env_metrics_t* metrics, void* stream);

/* ---- domain randomisation: per-environment friction, actuator gain, payload ------------------------------------------------------
 * The reference has none (every environment is the one robot of the MJCF file).  legged_gym (`randomize_friction`, `randomize_base_mass`, motor strength),
 * MuJoCo Playground and Brax (`domain_randomize`: `geom_friction`, `actuator_gainprm` / `biasprm`, `body_mass` written into a vmapped model) randomise the
 * physical parameters of each environment; so does this (csrc/domrand.h, k_domrand.hip).  Environment n owns the row
 *     p_n = (friction_scale, actuator_scale, added_mass, 0)
 * of a table `domain` [N][4] floats in DEVICE memory, fixed for the whole run, and behaves IN EVERY BIT as the unrandomised entry points behave on the
 * model whose tables are replaced, in float32:
 *     con_friction[3c]   <- con_friction[3c] * friction_scale    for every contact slot c (mixing is a max: every geom's sliding friction scaled)
 *     act_gain[u]        <- act_gain[u] * actuator_scale         for every actuator
 *     act_bias[3u + k]   <- act_bias[3u + k] * actuator_scale    k = 0 .. 2, for every actuator NOT on a ball joint (a ball joint's motor keeps its gear there)
 *     body_mass[b]       <- body_mass[b] + added_mass            for the one body b = mass_body (body_inertia stays: a point payload at the centre of mass)
 * Force and control ranges and the joints' actuatorfrcrange are not scaled (a stronger motor saturates where it did); nothing derived at compile time
 * (dof_invweight0, body_invweight0, meaninertia) is recomputed - what `domain_randomize` does when it writes body_mass and geom_friction into an mjx.Model.
 * The row (1, 1, 0, .) changes no bit.  A randomised launch runs kernel instantiations of its own (csrc/env_kernel.h); every other launch runs the kernels
 * it always ran.
 *
 * The draw is stateless - a function of (seed, rank, environment) alone; nothing is added to the state record or to a checkpoint, a resumed run has the
 * same robots.  With S = ("DRAND" << 24) + (rank << 16), for local environment n:
 *     r = philox(counter = {n, 0xFFFFFFFD, lo(S), hi(S)}, key = seed)
 *     friction_scale = uniform(r.x, friction_min, friction_max); actuator_scale = uniform(r.y, actuator_min, actuator_max); added_mass = uniform(r.z, mass_min, mass_max)
 * bits -> float as in mppo_env_reinit; min == max gives exactly that value (host statement: minppo_amd/jaxrng.py domain_params_philox).  Philox under both
 * rng_impl values (the reference has no such stream).  Refused (MPPO_EINVAL, the message names the value): min > max, a negative friction or actuator
 * scale, a range that is not finite, rank outside 0 .. 255, and - wherever a model is at hand - mass_body outside 1 .. nbody - 1 and
 * body_mass[mass_body] + mass_min <= 0; a null table where one is required.
 *
 * mppo_domain_fill         : writes domain [N][4] (device).  One launch, no workspace; mass_body is not read (there is no model to check it against).
 * mppo_env_reset_domain    : mppo_env_reset and mppo_env_reinit in one, under a table: the reset kernel with the environment's own row.  mask = NULL: every
 *                        environment (state, and - each may be NULL - reset_rec = environment 0's record, obs, reward, done, metrics as mppo_env_reset writes
 *                        them); mask given: the environments it names, state and observation rows only, as mppo_env_reinit.  scale > 0: reset noise, drawn as
 *                        mppo_env_reinit draws it (rng_impl, seed, rank, key2, counter, counter_offset as there); scale = 0: the plain reset of each robot.
 *                        Under randomisation the one shared reset record is wrong for every environment but the one it came from: every restart goes through
 *                        this entry point over the step's `done` (the engine and the evaluator do so), which overwrites what the step copied.
 * mppo_env_step_domain     : mppo_env_step_xfrc's arguments plus the table.  xfrc may be NULL (push_body is then not read).
 * mppo_physics_forward_domain : mppo_physics_forward_xfrc's arguments plus the table; cinert, qM, qfrc_actuator, the rows and everything behind them are those
 *                        of the environment's own robot. */
typedef struct mppo_domain_cfg {
  float friction_min, friction_max, actuator_min, actuator_max, mass_min, mass_max;
  int32_t mass_body;
  uint64_t seed;
  int32_t rank;
} mppo_domain_cfg_t;
int32_t mppo_domain_fill(const mppo_domain_cfg_t* cfg, int32_t N, float* domain, void* stream);
int32_t mppo_env_reset_domain(const mppo_model_t* m, int32_t N, float* state, float* reset_rec, float* obs, int32_t obs_ld, float* reward, uint8_t* done,
                              const mppo_env_metrics_t* metrics, const uint8_t* mask, const float* domain, int32_t mass_body, float scale, int32_t rng_impl,
                              uint64_t seed, int32_t rank, const uint32_t* key2, const int32_t* counter, int32_t counter_offset, void* stream);
int32_t mppo_env_step_domain(const mppo_model_t* m, int32_t N, int32_t n_frames, const mppo_reward_cfg_t* rc, float* state, const float* reset_rec,
                             const float* action, int32_t act_ld, float* obs, int32_t obs_ld, float* reward, uint8_t* done, const mppo_env_metrics_t* metrics,
                             int32_t push_body, const float* xfrc, const float* domain, int32_t mass_body, void* stream);
int32_t mppo_physics_forward_domain(const mppo_model_t* m, int32_t N, const float* qpos, const float* qvel, const float* ctrl, const float* qacc_warmstart,
                                    const mppo_forward_probe_t* out, int32_t push_body, const float* xfrc, const float* domain, int32_t mass_body, void* stream);

/* ---- sensor noise and actuation latency: observation noise, delayed actions ---------------------------------------------------------
 * The reference has neither: env.py:245-261 returns the simulator's observation to the last bit and env.py:148-196 applies an action in the step it was
 * computed.  legged_gym (`add_noise`, `noise_scale_vec`), MuJoCo Playground (`noise_config`, action latency) and Isaac Lab (`ActionDelay`) train with both;
 * so does this (csrc/sensor.h, k_sensor.hip), as launches of their own beside the environment step.  Both draws are stateless Philox under both rng_impl values
 * (the reference has no such stream); bits -> float as in mppo_env_reinit.
 *
 * mppo_obs_noise_apply : one launch, in place on obs[n, 0:O] (row stride obs_ld).  With S = ("ONOIS" << 24) + (rank << 16) and the step
 *     s = (counter ? *counter : 0) * counter_mul + counter_add modulo 2^32 (`counter` a word in DEVICE memory, NULL: 0, read when the launch runs):
 *         r = philox(counter = {n, s, lo(S) + (j >> 2), hi(S)}, key = seed);   obs[n][j] <- obs[n][j] + uniform(word j & 3 of r, -sigma[j], sigma[j])
 *     one float32 add (host statement: minppo_amd/jaxrng.py obs_noise_philox).  `sigma`: DEVICE memory, 4 * ceil(O / 4) floats (the entries behind O are
 *     read and not used).  A column whose sigma is not above 0 is NOT WRITTEN - every bit stays, a -0 or a NaN included - and neither are the columns
 *     O .. obs_ld - 1; a negative sigma cannot be refused here (the table is device memory): the entry points that take the vector from the host
 *     (mppo_engine_set_obs_noise, mppo_evaluate_sensors) refuse it.  The state record is not touched: what is perturbed is what the policy reads.  One lane per
 *     four columns; 16-byte loads and stores when obs and sigma are 16-byte aligned and obs_ld is a multiple of 4.  One writer per word, no atomics.
 *     MPPO_EINVAL: a null pointer, N < 1, O outside 1 .. 262144 (the block index j >> 2 has 16 bits of lo(S)), rank outside 0 .. 255, obs_ld below the
 *     padded observation width.
 * mppo_action_delay_fill : writes delay [N] (device int32), the latency of every environment for the whole run: with S = ("DELAY" << 24) + (rank << 16),
 *         d_n = min + (word 0 of philox(counter = {n, 0xFFFFFFFC, lo(S), hi(S)}, key = seed) mod (max - min + 1))
 *     (host statement: minppo_amd/jaxrng.py action_delays_philox).  MPPO_EINVAL (the message names the value): min < 0, min > max, max > 16, rank outside 0 .. 255.
 * mppo_action_delay_apply : one launch IN FRONT OF an environment step.  `action` [N] rows of A (row stride act_ld) is the policy's; `applied` [N] rows of A
 *     (row stride applied_ld) is what the step is to be given; `hist` [D][N][A] floats, D = cfg->max, is the ring of past actions (zeroed by the caller at the
 *     reset).  With k = episode_lengths[n] and ts = timestep[n] as they stand BEFORE the step (the metrics of mppo_env_step) and d = delay[n]:
 *         out = d == 0 ? action[n] : (k < d ? 0 : hist[(ts - d) mod D][n]);   hist[ts mod D][n] <- action[n];   applied[n] <- out      (the read first)
 *     so the environment is given the policy's action of step k - d of the SAME episode, exact zeros on the first d steps of every episode (after a fall or a
 *     truncation alike: episode_lengths is 0 again, there is no clearing launch), and with d = 0 the very bits of the policy's action.  Delay counts env
 *     steps, whatever n_frames is.  cfg->min, seed and rank are not read.  MPPO_EINVAL: the refusals of mppo_action_delay_fill, max = 0 (there is nothing
 *     to launch), a null pointer, act_ld or applied_ld below A. */
typedef struct mppo_obs_noise_cfg {
  uint64_t seed;
  int32_t rank, reserved;
} mppo_obs_noise_cfg_t;
typedef struct mppo_action_delay_cfg {
  int32_t min, max, rank, reserved;
  uint64_t seed;
} mppo_action_delay_cfg_t;
int32_t mppo_obs_noise_apply(const mppo_obs_noise_cfg_t* cfg, int32_t N, int32_t O, float* obs, int32_t obs_ld, const float* sigma, const int32_t* counter,
                             int32_t counter_mul, int32_t counter_add, void* stream);
int32_t mppo_action_delay_fill(const mppo_action_delay_cfg_t* cfg, int32_t N, int32_t* delay, void* stream);
int32_t mppo_action_delay_apply(const mppo_action_delay_cfg_t* cfg, int32_t N, int32_t A, const int32_t* delay, const int32_t* timestep,
                                const int32_t* episode_lengths, const float* action, int32_t act_ld, float* hist, float* applied, int32_t applied_ld, void* stream);

/* ------------------------------------------------------------------------------------------
 * PPO stages
 * ---------------------------------------------------------------------------------------- */

/* Network geometry + activation choice (train.py:56-83; config.py:52-55). */
typedef struct mppo_net {
  int32_t O, OP, A, H;
  int32_t use_tanh;  /* actor activation; the critic is always ReLU (train.py:82) */
  int32_t bf16;      /* 0: exact f32 MFMA; 1: bf16-in/f32-accumulate MFMA for the hidden GEMMs */
  int32_t num_layers; /* hidden layers of each MLP (`model.num_layers`, config.py:53, train.py:79,82): 1 .. 4; 0 means 2, the
                         reference's default.  Two hidden layers take the fused kernels, other depths the layer-wise path. */
} mppo_net_t;

/* Length (floats) of the flat parameter / gradient / Adam-moment vectors: the model's parameters with every tensor starting on
 * a 16-byte boundary (250 140 for O = 225, A = 10, H = 256: 250 133 parameters + 7 alignment words, which hold zeros). */
size_t mppo_param_count(const mppo_net_t* net);

/* `ActorCritic.__call__` + sample + log_prob on n rows (train.py:157-160, 79-83):
 *   mean = actor(obs); value = critic(obs); action = mean + exp(log_std)*noise;
 *   log_prob = MVNDiag.log_prob(action).  noise may be NULL (then action/log_prob are not
 *   written: the bootstrap-value call, train.py:182).  ws: workspace, >= mppo_policy_ws_bytes. */
size_t mppo_policy_ws_bytes(const mppo_net_t* net, int32_t n);
int32_t mppo_policy_forward(const mppo_net_t* net, const float* params, int32_t n, const float* obs, int32_t obs_ld,
                            const float* noise, float* action, float* log_prob, float* value, float* mean_out,
                            void* ws, size_t ws_bytes, void* stream);

/* The dense contraction every MLP layer goes through (`nn.Dense` forward, train.py:63,68, and the
 * two products its backward needs), as a batched launch of up to 6 problems on the f32 matrix cores.
 *   variant 0: C = act(A.B + bias)                A [M,K] (rows optionally gathered), B [K,N]
 *   variant 1: C = (A.B^T) * act'(aux)            B stored [N,K]
 *   variant 2: C = A^T.B  (split-K slabs)         A stored [K,M] (rows = samples, optionally gathered);
 *              bias_out (optional) receives the column sums of B (the bias gradient), one slab per split
 * act: 0 none, 1 tanh, 2 relu.  Exposed so that benchmarks can time exactly the kernel the engine runs. */
typedef struct mppo_gemm_desc {
  const float* A; const float* B; float* C; const float* bias; const float* aux; const int32_t* gather; float* bias_out;
  int32_t M, N, K, lda, ldb, ldc, ldaux, act;
} mppo_gemm_desc_t;
int32_t mppo_gemm_batch(const mppo_gemm_desc_t* probs, int32_t count, int32_t variant, int32_t ksplit, size_t slab_stride,
                        int32_t bf16, void* stream);

/* `_calculate_gae` (train.py:185-205): reverse scan over T, independent per env. */
int32_t mppo_gae(int32_t T, int32_t N, float gamma, float lam, const float* reward, const float* value,
                 const uint8_t* done, const float* last_val, float* adv, float* target, void* stream);
/* mppo_gae under an episode time limit (Brax's compute_gae with its truncation mask): `truncated` [T][N] marks the samples mppo_env_time_limit cut (a
 * subset of `done`).  In the reverse scan, at such a sample: adv = 0, target = value (the same bits), the carried gae becomes 0 and next_value this
 * sample's value as always - the value of the observation after the reset is never used as the truncated state's successor.  Every other sample's
 * arithmetic is mppo_gae's: with an all-zero `truncated` the output bits are its bits; truncated = NULL is exactly mppo_gae, launch and bits. */
int32_t mppo_gae_truncated(int32_t T, int32_t N, float gamma, float lam, const float* reward, const float* value, const uint8_t* done,
                           const uint8_t* truncated, const float* last_val, float* adv, float* target, void* stream);

/* One `_update_minibatch` gradient (train.py:213-247): gathers rows idx[0..mb) of the flat
 * [B,...] batch, forward, clipped-PPO loss with the given advantage statistics
 * (adv_stat = {mean, 1/(std+1e-8)}; per-minibatch population statistics, train.py:235),
 * backward.  grad [P] receives d(total_loss)/d(params) with every row weighted by inv_count
 * (1/mb on one GPU, 1/(mb*world) when ranks are summed afterwards).  loss4 = {total, value,
 * actor, entropy} partial sums weighted the same way. */
typedef struct mppo_batch {
  const float* obs;       int32_t obs_ld;   /* [B,OP]        */
  const float* action;    int32_t act_ld;   /* [B,act_ld]    */
  const float* value;                        /* [B] old value */
  const float* log_prob;                     /* [B] old logp  */
  const float* adv;                          /* [B]           */
  const float* target;                       /* [B]           */
} mppo_batch_t;
typedef struct mppo_loss_cfg { float clip_eps, vf_coef, ent_coef; } mppo_loss_cfg_t;
/* *fused = 1 if mppo_minibatch_grad takes the fused row pass + single-launch weight gradients for this geometry
 * (H a multiple of 32 up to 256, A <= 32, 16-byte aligned observation rows), 0 if it runs the layer-wise kernels. */
int32_t mppo_minibatch_path(const mppo_net_t* net, const mppo_batch_t* batch, int32_t* fused);
/* *rows = minibatch rows per workgroup of the fused row pass for a minibatch of mb rows: 16, or 32 where the engine's minibatch loop
 * (pre_gathered = 1) runs a float network's row pass on two 16-row tiles per workgroup because the 16-row tiling would need more
 * workgroups than the chip has CUs (BASELINE configs[4]: 2560-row minibatches).  One row of loss partials is written per workgroup. */
int32_t mppo_minibatch_rows_per_workgroup(const mppo_net_t* net, int32_t mb, int32_t pre_gathered, int32_t* rows);
size_t mppo_grad_ws_bytes(const mppo_net_t* net, int32_t mb);
int32_t mppo_minibatch_grad(const mppo_net_t* net, const float* params, const mppo_batch_t* batch, const int32_t* idx,
                            int32_t mb, const float* adv_stat, float inv_count, const mppo_loss_cfg_t* lc, float* grad,
                            float* loss4, void* ws, size_t ws_bytes, void* stream);

/* The row-local half of mppo_minibatch_grad on its own (forward of both networks, loss terms, d loss / d outputs and the
 * activation gradients dZ2, dZ1; one fused launch when H % 32 == 0 and A <= 16).  Same arguments; leaves its results in
 * `ws` for the weight-gradient product.  Exposed so that benchmarks can time exactly this kernel. */
int32_t mppo_minibatch_rowpass(const mppo_net_t* net, const float* params, const mppo_batch_t* batch, const int32_t* idx,
                               int32_t mb, const float* adv_stat, float inv_count, const mppo_loss_cfg_t* lc, void* ws,
                               size_t ws_bytes, void* stream);

/* Per-minibatch advantage statistics for all E*M minibatches of an update in one launch:
 * sums[k] = {sum adv, sum adv^2} (float64) over rows idx[k*mb .. (k+1)*mb); then
 * mppo_adv_stats_finalize turns (possibly all-reduced) sums into {mean, 1/(std+1e-8)}. */
int32_t mppo_adv_sums(const float* adv, const int32_t* idx, int32_t num_minibatches_total, int32_t mb, double* sums,
                      void* stream);
int32_t mppo_adv_stats_finalize(const double* sums, int32_t num_minibatches_total, double count, float* stats,
                                void* stream);

/* `optax.chain(clip_by_global_norm(max_norm), adam(lr_schedule, eps))` + apply (train.py:98-101,
 * 115-124, 248).  The step index is count_base[0] + step_offset (device int32 + host int, so
 * that the call can be captured in a hipGraph); lr = anneal ? lr*(1 - (count // sched_div)/num_updates)
 * : lr  with sched_div = minibatch_size*update_epochs as written in the reference (quirk C-2).
 * ws: >= mppo_adam_ws_bytes(P). */
typedef struct mppo_adam_cfg {
  float lr, max_grad_norm, b1, b2, eps;
  int32_t anneal, sched_div, num_updates;
} mppo_adam_cfg_t;
size_t mppo_adam_ws_bytes(size_t P);
int32_t mppo_clip_adam(size_t P, float* params, float* m, float* v, const float* grad, const int32_t* count_base,
                       int32_t step_offset, const mppo_adam_cfg_t* cfg, void* ws, size_t ws_bytes, void* stream);

/* Shadow copies.  The gradient workspace also holds W2^T of both networks (2 x H x H floats): with them the backward row pass
 * streams the second-layer weights like a forward layer (23.9 -> 21.9 us for the headline minibatch).  The workspace carries no
 * state, so the caller says when the copies match `params`:
 *   mppo_shadow_refresh          builds them from `params` (one small launch; after an upload, a restore, an external write);
 *   mppo_clip_adam_shadow        = mppo_clip_adam that also writes the updated W2 entries into the copies of `grad_ws`;
 *   mppo_minibatch_*_shadow      = mppo_minibatch_rowpass / _grad reading the copies (results identical to the plain forms).
 * The engine (mppo_engine_update / _learn) refreshes once per update and uses the _shadow forms throughout. */
int32_t mppo_shadow_refresh(const mppo_net_t* net, const float* params, int32_t mb, void* grad_ws, size_t grad_ws_bytes, void* stream);
int32_t mppo_minibatch_rowpass_shadow(const mppo_net_t* net, const float* params, const mppo_batch_t* batch, const int32_t* idx,
                                      int32_t mb, const float* adv_stat, float inv_count, const mppo_loss_cfg_t* lc, void* ws,
                                      size_t ws_bytes, void* stream);
int32_t mppo_minibatch_grad_shadow(const mppo_net_t* net, const float* params, const mppo_batch_t* batch, const int32_t* idx,
                                   int32_t mb, const float* adv_stat, float inv_count, const mppo_loss_cfg_t* lc, float* grad,
                                   float* loss4, void* ws, size_t ws_bytes, void* stream);
int32_t mppo_clip_adam_shadow(const mppo_net_t* net, int32_t mb, void* grad_ws, size_t grad_ws_bytes, size_t P, float* params,
                              float* m, float* v, const float* grad, const int32_t* count_base, int32_t step_offset,
                              const mppo_adam_cfg_t* cfg, void* ws, size_t ws_bytes, void* stream);

/* Pre-gathered rows (the engine's minibatch loop).  The observation rows of a minibatch depend on the permutation only, not on
 * the parameters, so the row pass of optimizer step s gathers the rows of step s + 1 on extra workgroups of its own launch into
 * the other of two k-quad buffers of the gradient workspace (`parity` 0 / 1 names the buffer that holds the CURRENT step's rows);
 * step s + 1 then starts from a contiguous tile instead of the index -> row chain (reference train.py:261-265, the gather).
 * The same workgroups gather the rows' scalars of the loss (action, old log_prob, advantage, old value, target) behind the observation
 * rows of the buffer, four rows of a column per float4: the next row pass reads them without an index -> row chain either.
 *   mppo_gather_rows               rows idx[0 .. mb) -> buffer `parity` (the first step of an update)
 *   mppo_minibatch_rowpass_pre     = mppo_minibatch_rowpass_shadow reading buffer `parity` and gathering idx_next (may be NULL: the
 *                                    last step) into the other buffer
 *   mppo_minibatch_grad_pre        the same, followed by the weight-gradient launch: results identical to mppo_minibatch_grad. */
int32_t mppo_gather_rows(const mppo_net_t* net, const mppo_batch_t* batch, const int32_t* idx, int32_t mb, void* grad_ws,
                         size_t grad_ws_bytes, int32_t parity, void* stream);
int32_t mppo_minibatch_rowpass_pre(const mppo_net_t* net, const float* params, const mppo_batch_t* batch, const int32_t* idx,
                                   const int32_t* idx_next, int32_t mb, const float* adv_stat, float inv_count,
                                   const mppo_loss_cfg_t* lc, void* ws, size_t ws_bytes, int32_t parity, void* stream);
int32_t mppo_minibatch_grad_pre(const mppo_net_t* net, const float* params, const mppo_batch_t* batch, const int32_t* idx,
                                const int32_t* idx_next, int32_t mb, const float* adv_stat, float inv_count,
                                const mppo_loss_cfg_t* lc, float* grad, float* loss4, void* ws, size_t ws_bytes, int32_t parity,
                                void* stream);

/* Counter-based RNG (Philox4x32-10), the engine's own stream (not JAX threefry).
 * mppo_normal_fill: out[i] ~ N(0,1), i in [0,n), a pure function of (seed, stream_id, i).
 * mppo_permutation: idx = a uniformly random permutation of [0,B) (sort of random keys, as
 * jax.random.permutation does; train.py:258).  ws >= mppo_permutation_ws_bytes(B). */
int32_t mppo_normal_fill(uint64_t seed, uint64_t stream_id, size_t n, float* out, void* stream);
size_t mppo_permutation_ws_bytes(int32_t B);
int32_t mppo_permutation(uint64_t seed, uint64_t stream_id, int32_t B, int32_t* idx, void* ws, size_t ws_bytes,
                         void* stream);
/* jax.random-compatible streams (threefry2x32, conventions of jax 0.4.3x; host restatement: minppo_amd/jaxrng.py).
 * key2 / rng2 / *_keys are DEVICE pointers to uint32 pairs.
 *   mppo_threefry_normal      jax.random.normal(key, (n,))  (what `pi.sample(seed=key)` draws, train.py:158-159)
 *   mppo_threefry_bits        jax.random.bits(key, (n,))
 *   mppo_threefry_update_keys the split tree of one _update_step: rng2 (in/out), act_keys [T][2], sort_keys [E][rounds][2]
 *   mppo_threefry_permutation jax.random.permutation(key, B) given its `rounds` sort keys (ws as for mppo_permutation) */
int32_t mppo_threefry_normal(const uint32_t* key2, size_t n, float* out, void* stream);
int32_t mppo_threefry_bits(const uint32_t* key2, size_t n, uint32_t* out, void* stream);
int32_t mppo_threefry_update_keys(uint32_t* rng2, int32_t T, int32_t E, int32_t rounds, uint32_t* act_keys, uint32_t* sort_keys, void* stream);
/* mppo_threefry_update_keys that also writes the T step keys (`rng, step_rng = split(rng)`, train.py:163), step_keys [T][2] */
int32_t mppo_threefry_update_keys_step(uint32_t* rng2, int32_t T, int32_t E, int32_t rounds, uint32_t* act_keys, uint32_t* sort_keys,
                                       uint32_t* step_keys, void* stream);
int32_t mppo_threefry_permutation(const uint32_t* sort_keys, int32_t rounds, int32_t B, int32_t* idx, void* ws, size_t ws_bytes, void* stream);

/* Running observation normalisation (csrc/k_obsnorm.hip).  The reference feeds the raw observation to the network (train.py:157); this is what
 * Brax's `ppo.train(normalize_observations=True)` and gym's `NormalizeObservation` do, as two stages.  Per column c < O the running statistics
 * are float64: `stats` [1 + 2 O] = count n | mean[O] | M2[O] (sum of squared deviations).  The float32 `table` [2][table_ld] is what gets applied:
 * row 0 mean32 = (float)mean, row 1 inv_std32 = (float)(1 / sqrt(M2 / n + eps)); while n = 0 it is exactly 0 / 1, the identity.
 *   mppo_obs_norm_partials  G, the workgroups (= partial sums) of one apply launch over N rows: ceil(N / 128)
 *   mppo_obs_norm_apply     in place on obs[n, 0:O] (row stride obs_ld): y = (x - mean32[c]) * inv_std32[c] in float32 in that order, clamped to
 *                           [-clip, clip] when clip > 0.  Columns O .. obs_ld - 1 are not written.  partial != NULL ([G][2][O] float64): workgroup g
 *                           also writes S1 = sum d and S2 = sum d^2, d = (double)x - (double)mean32[c] of the RAW x, over its rows 128 g .. 128 g + 127
 *                           below N: each group of 8 rows (one wave) summed in row order, then the 16 groups' sums added in row order (one writer per
 *                           word, no atomics, nothing that depends on timing).  16-byte loads and stores when obs is 16-byte aligned and obs_ld a
 *                           multiple of 4.
 *   mppo_obs_norm_update    one small launch, one thread per column: sums the n_partials x [2][O] partials in index order, then merges the k = `rows`
 *                           rows they hold (Chan): b = mean32 + S1/k, M2b = max(S2 - S1^2/k, 0), delta = b - mean, n' = n + k, mean' = mean + delta k/n',
 *                           M2' = M2 + M2b + delta^2 n k/n' (mean32: the table as it stands, which the partials were taken against); then rewrites
 *                           the table, columns O .. table_ld - 1 as 0 / 1.  rows = 0 (then n_partials = 0, partial may be NULL): the table from the
 *                           statistics alone.  The same inputs give the same bytes on every run.
 *   mppo_obs_norm_rank_sums several ranks: one small launch, one thread per column, in front of the ranks' gather.  Adds this rank's n_partials x [2][O] partials
 *                           in index order (from +0.0, as mppo_obs_norm_update adds them) into slot `rank` of `slots` [world][2][O] float64 - a sum of -0.0 is
 *                           written as +0.0 - and writes +0.0 into every other slot; nothing outside `slots` is written.  Once every rank holds all slots
 *                           (a gather; or a sum all-reduce of `slots`, in which every foreign term is +0.0 and x + 0 is exact, so the order of the library's
 *                           additions does not matter), mppo_obs_norm_update(O, world, rows of all ranks, slots, ...) adds them in rank order and merges:
 *                           every rank that starts from the same statistics and table ends with the same bytes.  world = 1: update(n_partials = 1) on
 *                           the one slot gives the bytes of update on the partials themselves.  The reward scaling's partials are the case O = 1.
 *                           MPPO_EINVAL: O or n_partials below 1, rank outside 0 .. world - 1, a null or misaligned pointer. */
int32_t mppo_obs_norm_partials(int32_t N);
int32_t mppo_obs_norm_rank_sums(int32_t O, int32_t n_partials, const double* partial, int32_t rank, int32_t world, double* slots, void* stream);
int32_t mppo_obs_norm_apply(int32_t N, int32_t O, float* obs, int32_t obs_ld, const float* table, int32_t table_ld, float clip, double* partial, void* stream);
int32_t mppo_obs_norm_update(int32_t O, int32_t n_partials, int64_t rows, const double* partial, double* stats, float eps, float* table, int32_t table_ld,
                             void* stream);

/* Reward scaling (csrc/k_rewnorm.hip).  The reference's GAE reads the raw reward (train.py:185-205); this is what gym's `NormalizeReward`, SB3's
 * `VecNormalize(norm_reward=True)` and Brax's `reward_scaling` do: the rewards of a rollout divided by the running standard deviation of the
 * discounted return.  `table` [2] = mean32 | inv_std32 and `stats` [3] = count n | mean | M2 are those of mppo_obs_norm_update with O = 1, table_ld = 1.
 *   mppo_reward_norm_partials  G, the workgroups (= partial sums) of one apply launch over N environments: ceil(N / 256)
 *   mppo_reward_norm_apply     one thread per environment n, forward over t = 0 .. T - 1 from ret = carry[n]: ret = ret * gamma + reward[t][n] in float32
 *                              (a multiply, then an add: two roundings); d = (double)ret - (double)table[0] is summed into S1 = sum d, S2 = sum d^2;
 *                              scaled[t][n] = reward[t][n] * table[1] in float32, clamped to [-clip, clip] when clip > 0 (a NaN stays a NaN); then, where
 *                              done[t][n], ret = 0 (the return that ends an episode is counted, then the carry restarts); at the end carry[n] = ret.
 *                              Rewards are scaled, never centred: the mean only shifts the sums.  `scaled` may be `reward`.  partial != NULL ([G][2]
 *                              float64): workgroup g writes (S1, S2) over its environments 256 g .. 256 g + 255 below N - a thread's steps in t order,
 *                              then the 64 lanes of a wave, then the four waves in wave order; no atomics, the same inputs give the same bytes.
 *                              MPPO_EINVAL: non-positive T / N, a null pointer (partial excepted), a negative (or NaN) clip, pointers not 4-byte
 *                              (partial: 8-byte) aligned.
 * The merge is mppo_obs_norm_update(1, G, T * N, partial, stats, eps, table, 1, stream). */
int32_t mppo_reward_norm_partials(int32_t N);
int32_t mppo_reward_norm_apply(int32_t T, int32_t N, float gamma, const float* reward, const uint8_t* done, float* carry, const float* table, float clip,
                               float* scaled, double* partial, void* stream);

/* ------------------------------------------------------------------------------------------
 * Engine: the whole `_update_step` (train.py:146-283) as one call, launches enqueued from
 * C++ (optionally replayed from a hipGraph), gradients summed over ranks with RCCL.
 * ---------------------------------------------------------------------------------------- */
typedef struct mppo_engine mppo_engine_t;

typedef struct mppo_engine_cfg {
  int32_t num_envs;          /* N on THIS rank                                     */
  int32_t num_steps;         /* T  (rl.num_env_steps == training.num_steps)        */
  int32_t num_minibatches;   /* M                                                   */
  int32_t update_epochs;     /* E                                                   */
  int32_t n_frames;
  int32_t num_updates;       /* for the LR schedule (train.py:93)                  */
  int32_t world_size, rank;
  float gamma, gae_lambda;
  mppo_loss_cfg_t loss;
  mppo_adam_cfg_t adam;      /* sched_div / num_updates are filled by the engine   */
  mppo_reward_cfg_t reward;
  mppo_net_t net;
  uint64_t seed;
  int32_t use_graph;         /* capture the update in a hipGraph and replay it      */
  int32_t external_random;   /* 1: noise / permutations are written by the caller into the arena (parity tests) */
  int32_t rng_impl;          /* 0: the engine's Philox streams; 1: jax.random-compatible threefry2x32 streams following the
                              * reference's split tree (train.py:158,163,252,258); the carried key is arena region "jax_rng" */
  int32_t reserved0;
} mppo_engine_cfg_t;

/* Arena: ONE device allocation owned by the caller (a torch uint8 tensor); the engine lays
 * every buffer out inside it.  mppo_engine_arena_bytes gives the size; named regions can be
 * located with mppo_engine_region (offset in bytes, size in bytes) to view them as tensors:
 * "params" "adam_m" "adam_v" "grad" "count" "state" "reset_rec" "obs" "action" "value" "reward"
 * "log_prob" "done" "last_val" "adv" "target" "noise" "perm" "adv_stats" "losses" "rollout_stats" "jax_rng" "reset_rng"
 * "obs_norm_stats" (float64) "obs_norm_table" "obs_norm_partials" (float64)
 * "reward_norm_stats" (float64 [3]) "reward_norm_table" ([2]) "reward_norm_carry" ([N]) "reward_norm_partials" (float64 [G][2]) "reward_scaled" ([T][N])
 * "truncated" (bytes [T][N]: the samples an episode time limit cut, mppo_engine_set_time_limit)
 * "action_hist" ([16][N][A]: the latency's ring) "action_applied" ([N][A]: what the last step launch was given) "action_delay" (int32 [N]) "obs_noise_scale" ([OP])
 * "norm_slots" (float64 [G][2][O] then [G][2]: the ranks' gathered sums of the two normalisations, G = world_size; untouched on one rank)
 * ("rollout_stats": 8 floats: sum reward, episodes ended, sum of their returns, sum of their lengths, the two means, truncations (0 without a time limit), 0) ... */
int32_t mppo_engine_arena_bytes(const mppo_model_t* m, const mppo_engine_cfg_t* cfg, size_t* out);
int32_t mppo_engine_create(const mppo_model_t* m, const mppo_engine_cfg_t* cfg, void* arena, size_t arena_bytes,
                           mppo_engine_t** out);
int32_t mppo_engine_destroy(mppo_engine_t* e);
int32_t mppo_engine_region(const mppo_engine_t* e, const char* name, size_t* offset, size_t* nbytes);
/* RCCL: rank 0 makes an id (128 bytes), the caller broadcasts it, every rank calls comm_init.
 * Collective on the engine's stream: one sum all-reduce of the [P] gradient per optimizer step
 * and one of the [E*M*2] float64 advantage sums per update. */
int32_t mppo_comm_unique_id(void* id128);
int32_t mppo_engine_comm_init(mppo_engine_t* e, const void* id128);
/* Peer-to-peer gradient exchange between the ranks of one node, the alternative to RCCL (csrc/peer.h; the reference has no data
 * parallelism: train.py:136,140).  Every rank allocates one exchange buffer (fine-grained device memory; this call ALLOCATES and
 * synchronises the device) and exports it as a 64-byte hipIpc handle; the caller gathers the handles of all ranks in rank order
 * (64 * world_size bytes), hands them to every rank, and places a host-side barrier between the last connect and the first update.
 * From then on the weight-gradient launch of every optimizer step publishes the local gradient, and the Adam launch reduces this
 * rank's slice, broadcasts it and waits for the others' (two hops, no extra launch, part of the hipGraph); the advantage sums take one
 * small kernel per update.  Takes precedence over an RCCL communicator.  Requires HSA_ENABLE_IPC_MODE_LEGACY=0 on this pool.
 * shared_device != 0: several of the ranks run on ONE GPU (how the path is exercised on a one-GPU box): a kernel that waits for a peer
 * must then leave room for that peer's kernels on every CU, so the two waits of a step become one-wave kernels of their own and
 * nothing else waits (five launches per optimizer step instead of three).
 *   mppo_engine_comm_mode    *out = 0 no exchange, 1 RCCL, 2 peer-to-peer (fused), 3 peer-to-peer in two launches, 4 peer-to-peer,
 *                            shared-GPU form
 *   mppo_engine_peer_status  synchronises the device; *timed_out != 0: a rank waited longer than MPPO_PEER_TIMEOUT_MS (default
 *                            60000) for a peer - the kernels ran to their end, the results are invalid.  info8 (optional, 8 words):
 *                            the first such wait {kind: 1 a peer's local gradient, 2 a reduced piece, 3 a peer's advantage sums, 5 a peer's normalisation sums;
 *                            index; epoch waited for; value seen}, then {optimizer steps, updates, workgroups counted into an unfinished gradient slice (0 between
 *                            launches), pieces per slice}
 *   mppo_engine_peer_selftest  collective (every rank, after the barrier that follows connect), on `stream`: one all-reduce of a
 *                            known vector through the mapped buffers, then ONE full optimizer step's exchange on a known gradient and
 *                            scratch parameters in the form the engine will launch it (publish, reduce + broadcast of this rank's
 *                            slice, wait for the others, Adam); *ok = 0 when a wait timed out or a value is wrong on THIS rank.  The caller
 *                            agrees on the outcome across ranks and, if any rank failed, calls
 *   mppo_engine_peer_disable   on every rank (frees the exchange; mppo_engine_comm_init may follow) */
int32_t mppo_engine_peer_export(mppo_engine_t* e, void* handle64);
int32_t mppo_engine_peer_connect(mppo_engine_t* e, const void* handles, int32_t shared_device);
int32_t mppo_engine_comm_mode(const mppo_engine_t* e, int32_t* out);
int32_t mppo_engine_peer_status(const mppo_engine_t* e, int32_t* timed_out, int32_t* info8);
int32_t mppo_engine_peer_selftest(mppo_engine_t* e, void* stream, int32_t* ok);
/* One-way latency, in microseconds, of a system-scope flag between this rank and `other_rank`: `iters` round trips of one word through the two
 * ranks' exchange buffers, timed on the device (100 MHz clock) - what one dependent trip of the fused exchange costs on this machine (on one GPU
 * about 0.65 us; over an xGMI hop: the t_link of DESIGN.md 7.2).  BOTH ranks call it at the same time, one with initiator = 1; synchronises.
 * `bench.py --gpus N` reports it per peer of rank 0 (config.t_link_us). */
int32_t mppo_engine_peer_latency(mppo_engine_t* e, int32_t other_rank, int32_t iters, int32_t initiator, void* stream, double* one_way_us);
int32_t mppo_engine_peer_disable(mppo_engine_t* e);
/* env reset (train.py:142-144) */
int32_t mppo_engine_reset(mppo_engine_t* e, void* stream);
/* Reset noise (`HumanoidEnv.reset_noise_scale`, env.py:87,115-121; 0, the default: every environment restarts from the constant reset record
 * and nothing changes).  scale > 0: mppo_engine_reset follows its plain reset - which still makes the noise-free "reset_rec" - with
 * mppo_env_reinit over all environments, and every rollout step is followed by one masked mppo_env_reinit over that step's done[t] (state rows and
 * the rows of observation slot t + 1), inside the captured graph too.  Streams per cfg.rng_impl: threefry keys live in arena region "reset_rng"
 * ([T][2] step keys of the current update, written by the update's key kernel - with external_random = 1 by the caller - then [2] the reset
 * key, written by the caller before mppo_engine_reset); the Philox events are 0 for the reset and u * T + 1 + t for step t of update u, u the
 * device's update index "count"[1].  Call before mppo_engine_reset: after it (with another scale than the one the reset ran with: the environments hold that
 * scale's initial states), after mppo_engine_prepare or after the first mppo_engine_update it returns MPPO_ESTATE. */
int32_t mppo_engine_set_reset_noise(mppo_engine_t* e, float scale);
/* Observation normalisation (mppo_obs_norm_* above; enabled = 0, the default: the engine enqueues exactly the launches it enqueues without this call).
 * enabled != 0: every rollout step is followed by one mppo_obs_norm_apply on the rows it wrote - observation slot t + 1, after the step and after the
 * reset-noise reinit where that is on - with the table of arena region "obs_norm_table" ([2][OP]) and the partials of step t in "obs_norm_partials"
 * ([T][G][2][O]); the rollout ends with one mppo_obs_norm_update over the T * G partials (rows = T * N) into "obs_norm_stats" ([1 + 2 O] float64) and
 * the table: T + 1 launches more per update, inside the captured graph too.  So the table is frozen within an update, every observation is stored
 * normalised with the table of the moment it was collected (the learn phase reads what the rollout's forward read), and the count is updates * T * N.
 * mppo_engine_reset zeroes the statistics and writes the identity table; the observation it makes (slot 0) stays raw.  The three regions lie behind
 * every other one and exist whether or not the option is on.  Call before mppo_engine_reset, mppo_engine_prepare and the first mppo_engine_update:
 * afterwards it returns MPPO_ESTATE.  MPPO_EINVAL: a negative (or NaN) clip / eps.
 * world_size > 1 (every rank makes the same call, AFTER mppo_engine_peer_connect or mppo_engine_comm_init: without a connected transport enabling is
 * MPPO_EINVAL - the statistics would silently be one rank's): the rollout ends with mppo_obs_norm_rank_sums into arena region "norm_slots" ([G][2][O] float64, behind them
 * [G][2] for the reward scaling), ONE gather of the slots per update for both options on the transport the learn phase uses (the peer exchange's own small
 * kernel, inside the captured graph; or one float64 all-reduce of the slots on the communicator), and mppo_obs_norm_update(O, G, T * N * G, slots, ...): two or
 * three launches more.  Statistics and table are bit-identical on every rank, the count is updates * T * N * G.  mppo_engine_rollout then needs a connected
 * transport like mppo_engine_learn (MPPO_ESTATE without one).  One rank: exactly the launches and arguments described above. */
int32_t mppo_engine_set_obs_norm(mppo_engine_t* e, int32_t enabled, float clip, float eps);
/* Reward scaling (mppo_reward_norm_* above; enabled = 0, the default: the engine enqueues exactly the launches it enqueues without this call).
 * enabled != 0: behind the rollout's bootstrap critic forward, one mppo_reward_norm_apply over the T steps reads arena region "reward" and writes
 * "reward_scaled" ([T][N]) with the table of "reward_norm_table" ([2]), the carried discounted return of "reward_norm_carry" ([N]) and the partials
 * in "reward_norm_partials" ([G][2]); GAE then reads "reward_scaled"; behind GAE one mppo_obs_norm_update(1, G, T * N, ...) merges the partials into
 * "reward_norm_stats" ([3] float64) and rewrites the table: 2 launches more per update, inside the captured graph too.  So the scale is frozen within
 * an update - update u divides by the deviation collected through update u - 1, the first by 1 - and the count is updates * T * N.  "reward",
 * "rollout_stats" and the environment's metrics stay raw: users see real returns.  mppo_engine_reset zeroes the statistics and the carry and writes the
 * identity table 0 | 1.  The five regions lie behind every other one and exist whether or not the option is on.  Call before mppo_engine_reset,
 * mppo_engine_prepare and the first mppo_engine_update: afterwards it returns MPPO_ESTATE.  MPPO_EINVAL: a negative (or NaN) clip / eps.
 * world_size > 1: as for mppo_engine_set_obs_norm (a connected transport first) - the ranks' (S1, S2) travel in the same gather, the statistics and the scale are bit-identical on every
 * rank and count updates * T * N * G returns; "reward_norm_carry" stays this rank's own (one return per environment). */
int32_t mppo_engine_set_reward_norm(mppo_engine_t* e, int32_t enabled, float clip, float eps);
/* Random pushes during training (mppo_push_cfg_t above; NULL or force = 0, the default: the engine enqueues exactly the launches, with exactly the
 * arguments, it enqueues without this call).  force > 0: every rollout step's environment launch draws its wrench inside the kernel - no launch more,
 * no [N][6] array, no arena region - at step s = u * T + t, u the device's update index "count"[1] read when the launch runs, so a replayed captured
 * graph draws fresh pushes and a resumed run continues the sequence (checkpoints already carry the counter; nothing else is state).  `seed` and `rank`
 * of the configuration are NOT read: the engine configuration's are used, so every rank pushes its own environments from its own stream and nothing
 * crosses ranks - any world_size is allowed.  The same bits as mppo_push_fill(counter = "count" + 1, counter_mul = T, counter_add = t) followed by
 * mppo_env_step_xfrc.  Call before mppo_engine_reset, mppo_engine_prepare and the first mppo_engine_update: afterwards it returns MPPO_ESTATE.
 * MPPO_EINVAL: the refusals listed at mppo_push_cfg_t. */
int32_t mppo_engine_set_push(mppo_engine_t* e, const mppo_push_cfg_t* push);
/* An episode time limit during training (mppo_env_time_limit above; length = 0, the default: the engine enqueues exactly the launches, with exactly the
 * arguments, it enqueues without this call - the plain GAE included).  length > 0: every rollout step becomes step -> mppo_env_time_limit (seed and rank:
 * the engine configuration's; any world_size - nothing crosses ranks) -> the masked mppo_env_reinit where reset noise is on (its mask done[t] now includes
 * the truncations) -> the observation normalisation's apply, in the captured graph too; the step's `truncated` bytes are row t of the arena region
 * "truncated" [T][N] (behind every other region; it exists whether or not a limit is set), GAE is mppo_gae_truncated over it, and "rollout_stats"[6] is
 * the number of truncations of the rollout (0 without a limit).  Reward scaling needs nothing: its carry restarts behind every `done`.  Call before
 * mppo_engine_reset, mppo_engine_prepare and the first mppo_engine_update: afterwards it returns MPPO_ESTATE.  MPPO_EINVAL: a negative length. */
int32_t mppo_engine_set_time_limit(mppo_engine_t* e, int32_t length, int32_t stagger);
/* Domain randomisation during training (mppo_domain_cfg_t above; NULL or every range at its identity - friction and actuator 1 .. 1, mass 0 .. 0, the default:
 * no table is allocated and the engine enqueues exactly the launches, with exactly the arguments, it enqueues without this call).  Otherwise the engine
 * allocates the table [N][4] (its own device allocation, not a region of the arena: the arena's layout and a checkpoint are what they were - the table is a
 * function of seed and rank, so a resumed run that makes this call again has the same robots), fills it once here, and passes it to every reset, step and
 * re-initialisation launch, in the captured graph too: mppo_engine_reset is mppo_env_reset_domain (then, under reset noise, the same masked over everyone),
 * every rollout step mppo_env_step_domain - with the pushes drawn inside it as before - followed by mppo_env_reset_domain over done[t] (truncations included;
 * at scale 0 when reset noise is off: one launch per rollout step that an unrandomised run without reset noise does not have).  The split step is not used.
 * `seed` and `rank` of the configuration are NOT read: the engine configuration's are used - every rank randomises its own environments from its own stream,
 * nothing crosses ranks, any world_size is allowed.  Call before mppo_engine_reset, mppo_engine_prepare and the first mppo_engine_update: afterwards it
 * returns MPPO_ESTATE.  MPPO_EINVAL: the refusals listed at mppo_domain_cfg_t. */
int32_t mppo_engine_set_domain(mppo_engine_t* e, const mppo_domain_cfg_t* domain);
/* Sensor noise during training (mppo_obs_noise_apply above; scale = NULL or every entry 0, the default: the engine enqueues exactly the launches, with exactly
 * the arguments, it enqueues without this call).  `scale`: HOST memory, [O] floats, the half-width sigma_j of every observation column; it is copied into arena
 * region "obs_noise_scale" ([OP], pad columns 0) by this call.  Then mppo_engine_reset follows its reset (and the initial reinit) with mppo_obs_noise_apply on
 * observation slot 0 at step 0, and every rollout step becomes step -> time limit -> masked reinit -> mppo_obs_noise_apply(counter = "count" + 1, counter_mul = T,
 * counter_add = t + 1) on slot t + 1 -> the observation normalisation's apply, in the captured graph too: one launch more per rollout step.  So the noisy row
 * is what the trajectory stores, what the next forward, the critic's bootstrap and the learn phase read and what the normalisation's statistics collect; a
 * replayed graph draws fresh values and a resumed run continues the sequence (checkpoints carry the counter; nothing else is state).  The state records stay
 * exact.  Seed and rank are the engine configuration's; nothing crosses ranks, any world_size is allowed.  Call before mppo_engine_reset, mppo_engine_prepare
 * and the first mppo_engine_update: afterwards it returns MPPO_ESTATE.  MPPO_EINVAL: a negative (or NaN) entry - the message names it -, more than 262144
 * columns, and, with the noise on, an engine rank outside 0 .. 255. */
int32_t mppo_engine_set_obs_noise(mppo_engine_t* e, const float* scale);
/* Actuation latency during training (mppo_action_delay_fill / _apply above; 0 / 0, the default: the engine enqueues exactly the launches, with exactly the
 * arguments, it enqueues without this call).  max > 0: mppo_engine_reset zeroes arena region "action_hist" and fills "action_delay" (seed and rank: the engine
 * configuration's), and every rollout step's environment launch is preceded by one mppo_action_delay_apply(action[t] -> "action_applied") and given that buffer
 * (act_ld = A) instead of action[t], in the captured graph too: one launch more per rollout step.  "action" and "log_prob" stay the policy's own - what PPO's
 * ratio refers to -; the reward's control cost sees the applied action, which is what the robot did.  The ring is indexed by the environments' own "timestep",
 * so a checkpoint needs "action_hist" beside the regions it always had and a resumed run continues bit for bit.  The four regions lie behind every other one
 * and exist whether or not the options are on.  Call before mppo_engine_reset, mppo_engine_prepare and the first mppo_engine_update: afterwards it returns
 * MPPO_ESTATE.  MPPO_EINVAL: the refusals of mppo_action_delay_fill. */
int32_t mppo_engine_set_action_delay(mppo_engine_t* e, int32_t min, int32_t max);
/* one full update: T rollout steps, bootstrap value, GAE, E epochs x M minibatches */
int32_t mppo_engine_update(mppo_engine_t* e, void* stream);
/* what mppo_engine_update does before it enqueues anything: the one-time capture of the update into a hipGraph (no device work).
 * Several ranks: call it on every rank, then a host-side barrier, then the first update - the ranks then start their first gradient
 * exchange together, not a capture time apart (the peer-to-peer exchange bounds every wait by MPPO_PEER_TIMEOUT_MS) */
int32_t mppo_engine_prepare(mppo_engine_t* e, void* stream);
/* *out = 1 once mppo_engine_update replays a captured hipGraph, 0 while it launches eagerly (use_graph = 0, null stream, a failed
 * capture, or an RCCL communicator without MPPO_GRAPH_COMM=1: RCCL calls are captured into the graph only on request, and the
 * ranks then agree through one eager all-reduce that every capture succeeded) */
int32_t mppo_engine_graph_active(const mppo_engine_t* e, int32_t* out);
/* pieces of the update, for stage-wise parity tests */
int32_t mppo_engine_rollout(mppo_engine_t* e, void* stream);
int32_t mppo_engine_learn(mppo_engine_t* e, void* stream);

/* ------------------------------------------------------------------------------------------
 * Policy evaluation: K steps of N environments under a trained policy, episode statistics and an
 * optional joint trajectory, as one call.  The reference has no counterpart (`minppo/infer.py:22-27`
 * raises NotImplementedError) and no time limit (env.py:238-242 ends an episode on height only): a
 * policy that stands never finishes an episode, so the result also counts the environments that
 * never fell (`survivors`) and the returns they have collected so far.
 *
 * mppo_evaluate enqueues exactly this sequence on `stream` (launches only; no allocation,
 * synchronisation or blocking copy - every buffer is a region of `ws`, a large robot's out-of-LDS
 * matrices included), a composition of the entry points above that gives the same bits when the
 * caller writes it out:
 *   1. mppo_env_reset with zeroed metrics
 *   2. reset_noise_scale > 0: mppo_env_reinit(mask NULL, rng_impl 0, seed, rank 0, counter NULL, counter_offset 0)
 *   3. for t = 0 .. K - 1:
 *        noise = deterministic ? zeros (then action == mean) : mppo_normal_fill(seed, stream_id = t, N * A)
 *        mppo_policy_forward on the current observation; mppo_env_step with n_frames
 *        reset_noise_scale > 0: mppo_env_reinit(mask = done, the same stream, counter_offset = t + 1)
 *        mppo_eval_accumulate
 *   4. mppo_eval_reduce
 * `params`: the flat parameter vector of `net`.  `ws`: 256-byte aligned, >= mppo_eval_ws_bytes (0 for
 * arguments mppo_evaluate refuses).  `result`: DEVICE memory, 8-byte aligned, valid once the stream
 * has run; the same inputs give the same bytes on every run (fixed reduction order, no atomics).
 * `traj` (device; may be NULL when record_envs = 0): [K + 1][R][W] floats, W = nq + nv + A + 2, of
 * environments 0 .. R - 1: frame 0 = state[n, 0 : nq + nv] after the reset (and the initial reinit), the
 * other columns zero; frame t + 1 = the state after step t (for an environment whose episode ended:
 * its restart state) | that step's action [A] | reward | done (0 or 1).
 * ---------------------------------------------------------------------------------------- */
typedef struct mppo_eval_cfg {
  int32_t N, K, n_frames, deterministic, record_envs /* R, 0 .. N */;
  float reset_noise_scale;
  uint64_t seed;
  mppo_reward_cfg_t reward;
} mppo_eval_cfg_t;
typedef struct mppo_eval_result {  /* 8-byte fields in a fixed order */
  int64_t episodes;   /* episodes that ended within the K steps                                        */
  int64_t len_sum, len_min, len_max;   /* their lengths in env steps (0 when episodes = 0)             */
  int64_t survivors;  /* environments none of whose episodes ended                                     */
  int64_t steps;      /* K * N                                                                         */
  double ret_sum, ret_sumsq, ret_min, ret_max;   /* the ended episodes' returns; +inf / -inf when episodes = 0 */
  double survivor_ret_sum;   /* sum of the survivors' running episode_returns                          */
  double reward_sum;         /* sum of all K * N rewards                                               */
} mppo_eval_result_t;
size_t mppo_eval_ws_bytes(const mppo_model_t* m, const mppo_net_t* net, const mppo_eval_cfg_t* cfg);
int32_t mppo_evaluate(const mppo_model_t* m, const mppo_net_t* net, const float* params, const mppo_eval_cfg_t* cfg, void* ws,
                      size_t ws_bytes, mppo_eval_result_t* result, float* traj, void* stream);
/* mppo_evaluate for a policy trained on normalised observations: the same sequence with mppo_obs_norm_apply(N, O, obs, OP, obs_table, O, clip, NULL)
 * on the observation after every step (behind the reinit where there is one, in front of mppo_eval_accumulate); the observation after the reset is left
 * alone, as in the engine.  obs_table: DEVICE memory, [2][O] floats (mean32 | inv_std32, row stride O); NULL: exactly mppo_evaluate.  Same workspace. */
int32_t mppo_evaluate_obs_norm(const mppo_model_t* m, const mppo_net_t* net, const float* params, const mppo_eval_cfg_t* cfg, void* ws, size_t ws_bytes,
                               const float* obs_table, float clip, mppo_eval_result_t* result, float* traj, void* stream);
/* mppo_evaluate_obs_norm under random pushes - the robustness test: `survivors` of `steps / N` pushed steps is the figure two standing policies are
 * compared by.  push = NULL or force = 0: exactly mppo_evaluate_obs_norm (obs_table may be NULL as there).  Otherwise the documented sequence with
 *        mppo_push_fill(push with rank 0 and seed = cfg->seed, N, NULL, 0, t, xfrc) + mppo_env_step_xfrc(..., push->body, xfrc)
 * in place of step t's mppo_env_step - the same bits when the caller writes it out - except that the wrench is drawn inside the environment kernel:
 * no launch more and no wrench array, so the workspace is mppo_eval_ws_bytes' as before.  `seed` and `rank` of the configuration are not read.  A push
 * keeps running across an episode's restart.  MPPO_EINVAL: the refusals listed at mppo_push_cfg_t. */
int32_t mppo_evaluate_push(const mppo_model_t* m, const mppo_net_t* net, const float* params, const mppo_eval_cfg_t* cfg, void* ws, size_t ws_bytes,
                           const float* obs_table, float clip, const mppo_push_cfg_t* push, mppo_eval_result_t* result, float* traj, void* stream);
/* The two statistics stages on caller-given arrays (as mppo_gae / mppo_adv_sums are stages of the update).
 * `acc`: the per-environment accumulators, 10 * N 8-byte words in device memory, 8-byte aligned, slot-major (word n of
 * slot k at 8 * (k * N + n)): int64 episodes, len_sum, len_min, len_max; double ret_sum, ret_sumsq, ret_min, ret_max,
 * reward_sum, running episode_returns.  Every word has one writer; nothing is atomic.
 *   mppo_eval_accumulate  one step: reads reward [N] (done [N] only for the trajectory row: may be NULL when R = 0) and the env kernel's own bookkeeping (metrics: returned_episode,
 *                         returned_episode_returns, returned_episode_lengths, episode_returns as mppo_env_step left them -
 *                         returns are not re-derived) and updates `acc`; first != 0: `acc` is empty (written, not read).
 *                         R > 0 also writes one trajectory row [R][row_w + A + 2] = state[n, 0 : row_w] | action[n, 0 : A]
 *                         (NULL: zeros) | reward[n] | done[n] into traj_row.
 *   mppo_eval_reduce      the accumulators of N environments after K steps -> *result (device memory), one workgroup, fixed order. */
int32_t mppo_eval_accumulate(int32_t N, int32_t first, const float* reward, const uint8_t* done, const mppo_env_metrics_t* metrics,
                             void* acc, const float* state, int32_t state_ld, int32_t row_w, const float* action, int32_t act_ld,
                             int32_t A, int32_t R, float* traj_row, void* stream);
int32_t mppo_eval_reduce(int32_t N, int32_t K, const void* acc, mppo_eval_result_t* result, void* stream);
/* mppo_evaluate_push under an episode time limit (no stagger, rank 0): with episode_length > 0 the documented sequence with
 *        mppo_env_time_limit({episode_length, 0, 0, 0, cfg->seed}, ..., done, truncated, metrics)
 * behind every step's mppo_env_step (in front of the masked reinit, whose mask then includes the truncations, the observation normalisation and
 * mppo_eval_accumulate, which therefore counts a truncated episode as an episode, with its return and length), one mppo_eval_limit_count behind
 * mppo_eval_accumulate and one mppo_eval_limit_reduce at the end - the same bits when the caller writes it out.  The trajectory's `done` column
 * includes the truncations.  *result keeps its documented meaning (`survivors`: the environments none of whose episodes ended - under a limit
 * shorter than K that is none of them); *extra (DEVICE memory, 8-byte aligned) says why the episodes ended:
 *        truncated_episodes  the episodes the limit cut;  fallen_envs  the environments with at least one termination (N - fallen_envs never fell).
 * episode_length = 0: exactly mppo_evaluate_push, bytes and launches; *extra is not written (it may be NULL).  MPPO_EINVAL: a negative length.
 * `ws`: >= mppo_eval_limit_ws_bytes (mppo_eval_ws_bytes' regions, then truncated [N] and the counters), whatever episode_length is.
 *   mppo_eval_limit_count   one step: `acc` (2 * N int64 in device memory, 8-byte aligned: truncations [N] | terminations [N]) gains this step's
 *                           truncated[n] and done[n] && !truncated[n]; first != 0: `acc` is empty (written, not read).
 *   mppo_eval_limit_reduce  those counters -> *result (device memory): the first row's sum and the number of non-zero words of the second. */
typedef struct mppo_eval_limit_result {
  int64_t truncated_episodes;
  int64_t fallen_envs;
} mppo_eval_limit_result_t;
size_t mppo_eval_limit_ws_bytes(const mppo_model_t* m, const mppo_net_t* net, const mppo_eval_cfg_t* cfg);
int32_t mppo_evaluate_limit(const mppo_model_t* m, const mppo_net_t* net, const float* params, const mppo_eval_cfg_t* cfg, void* ws, size_t ws_bytes,
                            const float* obs_table, float clip, const mppo_push_cfg_t* push, int32_t episode_length, mppo_eval_result_t* result,
                            mppo_eval_limit_result_t* extra, float* traj, void* stream);
/* mppo_evaluate_limit under domain randomisation - the robustness sweep: "does this policy still stand at friction 0.3, or with 5 kg on its back?" is one
 * call with min = max.  domain = NULL or every range at its identity: exactly mppo_evaluate_limit, bytes and launches.  Otherwise the documented sequence with
 *        mppo_domain_fill(domain with rank 0 and seed = cfg->seed, N, table) in front, mppo_env_reset_domain for the reset (and, under reset noise, for the
 *        initial states), mppo_env_step_domain for step t, and mppo_env_reset_domain(mask = done, counter_offset = t + 1) behind every step (and behind the time
 *        limit's launch) whether or not reset noise is on
 * - the same bits when the caller writes it out.  `seed` and `rank` of the configuration are not read.  `ws`: >= mppo_eval_domain_ws_bytes
 * (mppo_eval_limit_ws_bytes' regions, then the table), whatever the ranges are.  MPPO_EINVAL: the refusals listed at mppo_domain_cfg_t. */
size_t mppo_eval_domain_ws_bytes(const mppo_model_t* m, const mppo_net_t* net, const mppo_eval_cfg_t* cfg);
int32_t mppo_evaluate_domain(const mppo_model_t* m, const mppo_net_t* net, const float* params, const mppo_eval_cfg_t* cfg, void* ws, size_t ws_bytes,
                             const float* obs_table, float clip, const mppo_push_cfg_t* push, int32_t episode_length, const mppo_domain_cfg_t* domain,
                             mppo_eval_result_t* result, mppo_eval_limit_result_t* extra, float* traj, void* stream);
/* mppo_evaluate_domain under sensor noise and actuation latency - "does it still stand with 20 ms of latency and noisy encoders?".  obs_noise_scale = NULL or
 * all zero and delay = NULL or 0 / 0: exactly mppo_evaluate_domain, bytes and launches.  Otherwise the documented sequence with
 *        mppo_action_delay_fill(delay with rank 0 and seed = cfg->seed, N, table) behind the reset, the ring zeroed;
 *        mppo_obs_noise_apply({cfg->seed, 0}, ..., sigma, NULL, 0, 0) on the observation after the reset (and the initial reinit);
 *        per step t: mppo_action_delay_apply(action -> applied, act_ld = A) in front of the step, which is given `applied`; and
 *        mppo_obs_noise_apply(..., NULL, 0, t + 1) behind the step, the time limit's launch and the masked reinit, in front of the observation normalisation
 * - the same bits when the caller writes it out; both apply under `deterministic` too.  obs_noise_scale: HOST memory, [O] floats (copied into the workspace: the
 * one host-to-device copy of this call, so enqueue it outside a stream capture; a negative entry is MPPO_EINVAL).  The trajectory's action columns stay the
 * policy's; traj_applied (device, may be NULL; written only under a latency): [K + 1][R][A], frame t + 1 = what step t's environments 0 .. R - 1 were given, frame 0
 * zero.  `seed` and `rank` of the delay configuration are not read.  `ws`: >= mppo_eval_sensors_ws_bytes (mppo_eval_domain_ws_bytes' regions, then the ring
 * [16][N][A], the applied actions, the latency table and sigma), whatever the options are. */
size_t mppo_eval_sensors_ws_bytes(const mppo_model_t* m, const mppo_net_t* net, const mppo_eval_cfg_t* cfg);
int32_t mppo_evaluate_sensors(const mppo_model_t* m, const mppo_net_t* net, const float* params, const mppo_eval_cfg_t* cfg, void* ws, size_t ws_bytes,
                              const float* obs_table, float clip, const mppo_push_cfg_t* push, int32_t episode_length, const mppo_domain_cfg_t* domain,
                              const float* obs_noise_scale, const mppo_action_delay_cfg_t* delay, mppo_eval_result_t* result, mppo_eval_limit_result_t* extra,
                              float* traj, float* traj_applied, void* stream);
int32_t mppo_eval_limit_count(int32_t N, int32_t first, const uint8_t* done, const uint8_t* truncated, void* acc, void* stream);
int32_t mppo_eval_limit_reduce(int32_t N, const void* acc, mppo_eval_limit_result_t* result, void* stream);

/* ---- rendering --------------------------------------------------------------------------------------------------------------
 * Frames of a rollout as images, ray-cast on the device (csrc/k_render.hip): what the reference leaves to MuJoCo's renderer
 * (env.render, minppo/env.py:264-333).  A scene is opened from the scene blob of minppo_amd/render.py (scene_blob: the kinematic
 * tree, the visuals, hull face planes, the ground plane, the cameras; layout in csrc/render.h), given in host memory (validated
 * there: a malformed blob is MPPO_EMODEL with a message) and in device memory (what the kernels read; it must outlive the handle).
 *
 * mppo_render draws F frames with one camera: two launches on `stream` (the visuals' and the camera's world poses from qpos,
 * then one ray per pixel), no synchronisation; the scratch for the poses belongs to the handle and grows on demand (a device
 * allocation on the first call and when a later call needs more: one render at a time per handle).  `qpos` is device memory,
 * frame f at qpos + f * q_ld: q_ld = nq for packed joint positions, q_ld = rec_dim to draw straight from state records or an
 * evaluation's trajectory rows (qpos is at offset 0 of both).  Outputs are device memory; any may be NULL.
 * The image: MuJoCo's camera convention (looks along -z, +x right, +y up, vertical fovy), row 0 at the top, one ray through every
 * pixel centre, no anti-aliasing; Lambert shading from one fixed directional light plus ambient, hard shadows, a two-tone 1 m
 * checker on the ground plane, a constant sky; meshes are drawn as their convex hulls. */
typedef struct mppo_scene mppo_scene_t;
typedef struct mppo_scene_dims { int32_t nq, nbody, ngeom, ncam, has_plane; } mppo_scene_dims_t;
int32_t mppo_scene_open(const void* host_blob, size_t nbytes, const void* dev_blob, mppo_scene_t** out);
int32_t mppo_scene_close(mppo_scene_t* s);
int32_t mppo_scene_get_dims(const mppo_scene_t* s, mppo_scene_dims_t* out);
typedef struct mppo_render_out {   /* any pointer may be NULL */
  uint8_t* rgb;      /* [F, H, W, 3] */
  float*   depth;    /* [F, H, W] distance along the unit ray; +inf on a miss */
  int32_t* geom_id;  /* [F, H, W] visual index; ngeom = ground plane; -1 = miss */
  float*   geom_pose;/* [F, ngeom, 12] world position + row-major rotation of every visual */
} mppo_render_out_t;
int32_t mppo_render(const mppo_scene_t* s, int32_t F, const float* qpos, int32_t q_ld, int32_t camera, int32_t width, int32_t height,
                    const mppo_render_out_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MINPPO_HIP_H */
