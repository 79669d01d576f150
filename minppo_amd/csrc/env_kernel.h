// What the environment kernel's translation unit (k_physics.hip: the kernel and its instantiations) and the model handle's (env_model.hip:
// the handle, its layout, the C ABI) share: the kernel's argument struct, the tag of a code object, the launch of an instantiation.
#pragma once
#include "model_view.h"
#include "mppo_common.h"
#include "push.h"
#include "domrand.h"

namespace mppo {

struct EnvArgs {
  int N, mode, n_frames;  // mode 0: reset (pipeline_init), 1: step, 2: probe (one forward on given inputs)
  float* state;
  const float* reset_in;
  float* reset_out;
  const float* action;
  int act_ld;
  float* obs;
  int obs_ld;
  float* reward;
  unsigned char* done;
  mppo_env_metrics_t met;
  mppo_reward_cfg_t rc;
  const float *p_qpos, *p_qvel, *p_ctrl, *p_warm;
  mppo_forward_probe_t probe;
  float* scratch;  // per-environment records in global memory for the matrices a large robot keeps out of LDS (PhysLds::gwords floats each; null if none)
  // mode 0 only - the reset from randomised states (env.py:115-121 with reset_noise_scale > 0): qpos = qpos0 + U(-s, s), qvel = U(-s, s), drawn in the
  // kernel per environment and element.  Behind everything the step kernel reads, so that its argument offsets stay what they were.
  const unsigned char* mask;    // [N], null: every environment; an environment whose byte is 0 is left alone (the engine passes a step's done[t])
  float noise_scale;            // s; 0: the plain reset
  int noise_impl;               // 0: the engine's Philox stream kStreamReset, 1: the reference's threefry tree (split(K, N)[n] -> split -> uniform), 2: the same from given key_n
  const unsigned* noise_key;    // threefry: K, two words in device memory (the reset key, train.py:142, or a step key, :163); impl 2: the N keys split(K, N), [N][2]
  unsigned long long noise_seed, noise_stream;  // philox: the key and the stream id (kStreamReset + (rank << 16))
  const int* noise_ctr;         // philox: the event counter's word in device memory (null: 0) ...
  int noise_ctr_mul, noise_ctr_add;  // ... event = word * mul + add: the engine's update index * T + 1 + t, so that a replayed graph draws fresh values
  // domain randomisation (domrand.h): row n = (friction_scale, actuator_scale, added_mass, 0) replaces, in float32 and before they are used, con_friction[3c] by
  // con_friction[3c] * friction_scale, act_gain[u] and (not on a ball joint) act_bias[3u + k] by their products with actuator_scale, body_mass[mass_body] by
  // body_mass[mass_body] + added_mass.  A launch is randomised (domain non-null) or it is not; a randomised launch runs a kernel instantiation of its own
  // (env_kernel_index below), any other reads nothing of what follows.  In front of the wrench's fields, which stay the LAST of the struct: the run-time-sized pushed kernels load them together with the first words
  // of PhysLds, the argument behind this one - anything put between the two would change those kernels' scalar loads, not only their offsets.
  const float* domain;          // [N][4]; null: the launch is not randomised
  int mass_body;                // 1 .. nbody - 1: the body that carries the payload
  // modes 1 and 2 only - an external wrench on one body (MJX xfrc_applied: world axes, at the body's centre of mass), constant over the frames of the step.
  // A launch is pushed (push_body > 0: the host sets it when xfrc is given or push.force > 0) or it is not; a pushed launch runs a kernel instantiation of its
  // own (env_kernel_index below), an unpushed one reads nothing of what follows.  Behind everything else, by the rule above.
  int push_body;                // 1 .. nbody - 1; 0: the launch is not pushed
  const float* xfrc;            // [N][6] force | torque; null: the wrench is drawn in the kernel (push.h) if push.force > 0, else there is none
  PushDraw push;                // the draw's parameters (force 0: off)
  const int* push_ctr;          // the step index's word in device memory (null: 0) ...
  int push_ctr_mul, push_ctr_add;  // ... step = word * mul + add: the engine's update index * T + t
};

// the kernel a launch runs (env_kernel's KMODE): its mode, and for a pushed step / probe the instantiation that holds the wrench's code; a randomised launch
// (EnvArgs::domain) runs the randomised family's reset, step or probe (6 .. 8), whose step and probe take a wrench behind a run-time test.  5 is the split step,
// which launch_env_spec picks by itself: no launch asks for it here.
constexpr int kEnvKernels = 9;
constexpr int kEnvKernelRand = 6;
inline int env_kernel_index(const EnvArgs& a) { return a.domain ? kEnvKernelRand + a.mode : a.mode >= 1 && a.push_body > 0 ? a.mode + 2 : a.mode; }

constexpr unsigned long long kStreamReset = 0x5245534554ull << 24;  // "RESET" (engine.hip: beside kStreamNoise / kStreamPerm)

// The tag a code object of k_physics.hip carries (its device symbol `mppo_env_kernel_tag`): the sizes of the three kernel-argument structs and the blob version -
// what has to agree between the library and a code object compiled apart from it for a launch to mean anything.
constexpr unsigned kEnvKernelTag = (unsigned)sizeof(ModelView) * 2654435761u ^ (unsigned)sizeof(EnvArgs) * 40503u ^ (unsigned)sizeof(PhysLds) * 2246822519u ^ kBlobVersion * 3266489917u ^
                                   (unsigned)kEnvsPerWave;

// k_physics.hip: the instantiation compiled for these dims (its index in spec_dims.inc; -1: none), whether a build added it (MPPO_SPECIALIZE), its launch (-1: run-time-sized)
int find_spec(const BlobDims& d);
bool spec_is_extra(int spec);
bool spec_has_split(int spec);  // the instantiation has a split step (KMODE 5), which launch_env_spec picks for small launches unless `may_split` is false
int32_t launch_env_spec(int spec, const ModelView& mv, const EnvArgs& a, const PhysLds& lds, int lds_bytes, int blocks, int waves, bool may_split, hipStream_t stream);

}  // namespace mppo
