// env_model.hip - the model handle of the environment kernel (k_physics.hip): a validated model's (model_blob.hip) LDS layout, the on-device check of a specialised kernel, attached code objects, the C ABI
#include "env_kernel.h"

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

struct mppo_model {
  mppo::ModelView mv;
  mppo::PhysLds lds;
  int lds_bytes;
  int waves;  // wavefronts per workgroup (mv.epw environments each: 4, fewer for a very large robot; one copy of the model tables per workgroup)
  int spec;  // index into the table of model-specialised kernels (spec_dims.inc), -1: the run-time-sized kernel
  bool no_split = false;  // keep the specialised step unsplit whatever the launch's size (spec_self_check compares both forms; a form that failed it is not used)
  // the records of the matrices a large robot keeps out of LDS (PhysLds::gwords floats per environment group of the grid), for launches
  // through mppo_env_reset / _step / mppo_physics_forward: owned by the handle, grown on demand (the engine passes a region of its arena
  // instead).  One stream at a time may launch through a handle that needs them.
  mutable float* scratch = nullptr;
  mutable size_t scratch_bytes = 0;
  int canon_words = 0;  // the table part's length as it follows from the dims (what a specialised kernel's compile-time layout choice saw)
  // a code object attached at run time (mppo_model_attach_kernel): the environment kernel compiled for exactly this robot's dimensions -
  // what MPPO_SPECIALIZE does at build time, for a robot the library was not built for
  bool jit = false;
  int jit_regchol = 0;  // the MPPO_REGCHOL_MAX_NV the code object was compiled with (its LDS layout follows from it)
  hipModule_t jit_module = nullptr;
  hipFunction_t jit_fn[mppo::kEnvKernels] = {};  // reset, step, probe, pushed step, pushed probe, (none), randomised reset, step, probe (env_kernel_index)
  std::vector<float> body_mass;  // the blob's body_mass on the host: what a payload's lower end is checked against (check_domain_cfg)
  std::vector<char> jit_image;
};

namespace mppo {
const ModelView& model_view(const mppo_model* m) { return m->mv; }
// bytes of global memory the environment kernel needs beside the state for N environments (0 for a robot whose matrices fit LDS)
size_t model_scratch_bytes(const mppo_model* m, int N) {
  if (m->lds.gwords <= 0) return 0;
  const int per_block = m->mv.epw * m->waves;
  return (size_t)cdiv(N, per_block) * per_block * (size_t)m->lds.gwords * sizeof(float);
}

// `ws`: the caller's region for the out-of-LDS matrices (the engine's arena), or null: the handle's own allocation, grown on demand
static int32_t launch_env(const mppo_model_t* m, EnvArgs a, hipStream_t stream, float* ws = nullptr, size_t ws_bytes = 0) {
  const int blocks = cdiv(a.N, m->mv.epw * m->waves);
  const size_t need = model_scratch_bytes(m, a.N);
  if (need > 0) {
    if (ws) {
      if (ws_bytes < need) return fail(MPPO_EINVAL, "environment kernel: the caller's scratch region holds %zu bytes, %d environments need %zu", ws_bytes, a.N, need);
      a.scratch = ws;
    } else {
      if (m->scratch_bytes < need) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (stream && hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
          return fail(MPPO_EINVAL, "environment kernel: this robot keeps %zu bytes of matrices in global memory for %d environments and the handle's allocation would have to grow inside a stream capture: launch once outside the capture first", need, a.N);
        if (m->scratch) { MPPO_CHECK_HIP(hipDeviceSynchronize()); (void)hipFree(m->scratch); m->scratch = nullptr; m->scratch_bytes = 0; }
        MPPO_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&m->scratch), need));
        m->scratch_bytes = need;
      }
      a.scratch = m->scratch;
    }
  }
  if (m->jit) {
    ModelView mv = m->mv;
    PhysLds lds = m->lds;
    void* params[] = {&mv, &a, &lds};
    MPPO_CHECK_HIP(hipModuleLaunchKernel(m->jit_fn[env_kernel_index(a)], blocks, 1, 1, 64 * m->waves, 1, 1, m->lds_bytes, stream, params, nullptr));
    return MPPO_OK;
  }
  return launch_env_spec(m->spec, m->mv, a, m->lds, m->lds_bytes, blocks, m->waves, !m->no_split, stream);
}
// the engine's entry: mppo_env_step with the out-of-LDS matrices in a region of the engine's arena (hipGraph capture: nothing is allocated)
int32_t env_step_ws(const mppo_model_t* m, int32_t N, int32_t n_frames, const mppo_reward_cfg_t* rc, float* state, const float* reset_rec, const float* action,
                    int32_t act_ld, float* obs, int32_t obs_ld, float* reward, uint8_t* done, const mppo_env_metrics_t* metrics, float* ws, size_t ws_bytes, hipStream_t stream) {
  EnvArgs a{};
  a.N = N; a.mode = 1; a.n_frames = n_frames; a.state = state; a.reset_in = reset_rec; a.action = action; a.act_ld = act_ld;
  a.obs = obs; a.obs_ld = obs_ld; a.reward = reward; a.done = done; a.rc = *rc;
  if (metrics) a.met = *metrics;
  return launch_env(m, a, stream, ws, ws_bytes);
}
// Domain randomisation.  What every entry point that takes a domain configuration refuses (with a model at hand: the payload's body and the mass it leaves)
int32_t check_domain_body(const char* who, const mppo_model_t* m, int32_t body) {
  MPPO_REQUIRE(body >= 1 && body < m->mv.nbody, "%s: mass_body %d outside 1 .. nbody - 1 = %d (0 is the world)", who, body, m->mv.nbody - 1);
  return MPPO_OK;
}
int32_t check_domain_cfg(const char* who, const mppo_model_t* m, const mppo_domain_cfg_t* c) {
  MPPO_REQUIRE(c->friction_min <= c->friction_max, "%s: friction_min %g > friction_max %g (or not a number)", who, (double)c->friction_min, (double)c->friction_max);
  MPPO_REQUIRE(c->actuator_min <= c->actuator_max, "%s: actuator_min %g > actuator_max %g (or not a number)", who, (double)c->actuator_min, (double)c->actuator_max);
  MPPO_REQUIRE(c->mass_min <= c->mass_max, "%s: mass_min %g > mass_max %g (or not a number)", who, (double)c->mass_min, (double)c->mass_max);
  MPPO_REQUIRE(c->friction_min >= 0.f, "%s: friction_min %g is negative", who, (double)c->friction_min);
  MPPO_REQUIRE(c->actuator_min >= 0.f, "%s: actuator_min %g is negative", who, (double)c->actuator_min);
  MPPO_REQUIRE(std::isfinite(c->friction_max) && std::isfinite(c->actuator_max) && std::isfinite(c->mass_min) && std::isfinite(c->mass_max),
               "%s: a range of the domain randomisation is not finite (friction_max %g, actuator_max %g, mass %g .. %g)", who, (double)c->friction_max, (double)c->actuator_max,
               (double)c->mass_min, (double)c->mass_max);
  MPPO_REQUIRE(c->rank >= 0 && c->rank < 256, "%s: rank %d (0 .. 255)", who, c->rank);
  if (m) {
    MPPO_TRY(check_domain_body(who, m, c->mass_body));
    const float m0 = m->body_mass[c->mass_body];
    MPPO_REQUIRE(m0 + c->mass_min > 0.f, "%s: body %d weighs %g kg: mass_min %g leaves it without mass", who, c->mass_body, (double)m0, (double)c->mass_min);
  }
  return MPPO_OK;
}
// a launch's randomisation: the table and the payload's body into the kernel's arguments (no table: nothing - the launch runs the kernels it always ran)
static int32_t set_domain(const mppo_model_t* m, const EnvDomain& dom, EnvArgs* a) {
  if (!dom.table) return MPPO_OK;
  MPPO_TRY(check_domain_body("environment kernel", m, dom.body));
  a->domain = dom.table; a->mass_body = dom.body;
  return MPPO_OK;
}
// Random pushes.  What every entry point that takes a push configuration refuses (the body is checked against the model by the callers that have one)
int32_t check_push_cfg(const char* who, const mppo_push_cfg_t* p) {
  MPPO_REQUIRE(p->force >= 0.f, "%s: push force %g is negative (or not a number)", who, (double)p->force);
  if (p->force == 0.f) return MPPO_OK;  // off: nothing else is read
  MPPO_REQUIRE(p->interval >= 1, "%s: push interval %d (at least 1 env step)", who, p->interval);
  MPPO_REQUIRE(p->duration >= 1 && p->duration <= p->interval, "%s: push duration %d outside 1 .. interval = %d", who, p->duration, p->interval);
  MPPO_REQUIRE(p->rank >= 0 && p->rank < 256, "%s: rank %d (0 .. 255)", who, p->rank);
  return MPPO_OK;
}
int32_t check_push_body(const char* who, const mppo_model_t* m, int32_t body) {
  MPPO_REQUIRE(body >= 1 && body < m->mv.nbody, "%s: push body %d outside 1 .. nbody - 1 = %d (0 is the world)", who, body, m->mv.nbody - 1);
  return MPPO_OK;
}
PushDraw push_draw_of(const mppo_push_cfg_t& p) {
  return PushDraw{p.force, p.interval, p.duration, p.seed, kStreamPush + ((unsigned long long)p.rank << 16)};
}
// env_step_ws under an external wrench (push.xfrc given, or drawn in the kernel when push.draw.force > 0; neither: exactly env_step_ws)
int32_t env_step_push_ws(const mppo_model_t* m, int32_t N, int32_t n_frames, const mppo_reward_cfg_t* rc, float* state, const float* reset_rec, const float* action,
                         int32_t act_ld, float* obs, int32_t obs_ld, float* reward, uint8_t* done, const mppo_env_metrics_t* metrics, const EnvPush& push, float* ws,
                         size_t ws_bytes, hipStream_t stream, const EnvDomain& dom) {
  EnvArgs a{};
  a.N = N; a.mode = 1; a.n_frames = n_frames; a.state = state; a.reset_in = reset_rec; a.action = action; a.act_ld = act_ld;
  a.obs = obs; a.obs_ld = obs_ld; a.reward = reward; a.done = done; a.rc = *rc;
  if (metrics) a.met = *metrics;
  MPPO_TRY(set_domain(m, dom, &a));
  if (push.xfrc || push.draw.force > 0.f) {
    MPPO_TRY(check_push_body("environment step", m, push.body));
    a.push_body = push.body; a.xfrc = push.xfrc;
    if (!push.xfrc) { a.push = push.draw; a.push_ctr = push.ctr; a.push_ctr_mul = push.mul; a.push_ctr_add = push.add; }
  }
  return launch_env(m, a, stream, ws, ws_bytes);
}
int32_t env_reset_ws(const mppo_model_t* m, int32_t N, float* state, float* reset_rec, float* obs, int32_t obs_ld, float* reward, uint8_t* done, const mppo_env_metrics_t* metrics,
                     float* ws, size_t ws_bytes, hipStream_t stream, const EnvDomain& dom) {
  EnvArgs a{};
  a.N = N; a.mode = 0; a.n_frames = 1; a.state = state; a.reset_out = reset_rec; a.obs = obs; a.obs_ld = obs_ld; a.reward = reward; a.done = done;
  if (metrics) a.met = *metrics;
  MPPO_TRY(set_domain(m, dom, &a));
  return launch_env(m, a, stream, ws, ws_bytes);
}
// the reset from randomised states over the environments `mask` names (null: all of them): the reset kernel with its noise fields set and nothing
// but the state rows and the observation rows to write - reward, done and the metrics are the step's, the reset record stays the noise-free one
int32_t env_reinit_ws(const mppo_model_t* m, int32_t N, float* state, float* obs, int32_t obs_ld, const uint8_t* mask, float scale, int32_t rng_impl, uint64_t seed,
                      int32_t rank, const uint32_t* key2, const int32_t* counter, int32_t counter_mul, int32_t counter_add, float* ws, size_t ws_bytes, hipStream_t stream,
                      const EnvDomain& dom) {
  // (the Philox stream numbers an environment's blocks of four elements in the 16 bits of the stream id below the rank)
  MPPO_REQUIRE(m->mv.nq + m->mv.nv <= 4 * 65536, "reset noise: %d noise elements per environment", m->mv.nq + m->mv.nv);
  EnvArgs a{};
  a.N = N; a.mode = 0; a.n_frames = 1; a.state = state; a.obs = obs; a.obs_ld = obs_ld;
  a.mask = mask; a.noise_scale = scale; a.noise_impl = rng_impl; a.noise_key = key2; a.noise_seed = seed;
  a.noise_stream = kStreamReset + ((unsigned long long)rank << 16);
  a.noise_ctr = counter; a.noise_ctr_mul = counter_mul; a.noise_ctr_add = counter_add;
  MPPO_TRY(set_domain(m, dom, &a));
  return launch_env(m, a, stream, ws, ws_bytes);
}

// MPPO_ENV_GENERIC=1 forces the run-time-sized kernel (A/B tests of the two instantiations); so does MPPO_ENV_SPILL, which only the
// run-time-sized kernel can follow (a specialised kernel's choice is compiled in)
static int env_spill_override() {
  const char* e = getenv("MPPO_ENV_SPILL");
  if (!e || !e[0]) return -1;
  const int v = atoi(e);
  return v == 0 ? 0 : v == 1 ? kSpillJ : (kSpillJ | kSpillM);
}
static bool generic_forced() { const char* e = getenv("MPPO_ENV_GENERIC"); return (e && e[0] == '1') || env_spill_override() >= 0; }

// LDS layout, matrices in global memory, environments per wave and waves per workgroup of a model whose `spec` is decided
static int32_t finalize_layout(mppo_model* m) {
  ModelView& v = m->mv;
  // (a model-specialised kernel of up to kRegCholMaxNv dofs keeps the inverse Cholesky factor in registers: no factor in its LDS layout; the
  // matrices that leave LDS for global memory - spill_for - are a function of the dims that the specialised kernel evaluated at compile time)
  // (MPPO_ENV_SPILL=0|1|3 overrides the choice - nothing, the Jacobian, the Jacobian and M in global memory - for A/B measurements and
  // for the test that holds the two placements bit-equal)
  const BlobDims bd = blob_dims_of(v);
  auto lds_for = [&](bool li_regs) {
    const int forced = env_spill_override();
    return make_phys_lds(bd, li_regs, forced >= 0 ? forced : spill_for(bd, li_regs, m->canon_words));
  };
  const bool fixed = m->spec >= 0 || m->jit;
  m->lds = lds_for(fixed && v.nv <= (m->jit ? m->jit_regchol : kRegCholMaxNv));
  // waves per workgroup: whatever puts the most waves on a CU (160 KB of LDS; every workgroup holds one copy of the model tables and
  // waves x 4 environments), the smaller workgroup on a tie.  MPPO_ENV_WAVES=1..4 overrides (measurements).
  // A robot too large for four environments per wave even with its matrices outside LDS runs two or one per wave on the
  // run-time-sized kernel - three quarters of the lanes idle, but it runs (round 5; before, it was refused).
  v.epw = kEnvsPerWave;
  if (fixed && ((long long)v.blob_words + (long long)m->lds.total * kEnvsPerWave) * 4 > 160 * 1024) {
    // (a specialised kernel carries four environments per wave; a robot too large for that runs the run-time-sized kernel with fewer)
    m->spec = -1;
    m->jit = false;
    m->lds = lds_for(false);
  }
  auto lds_of = [&](int w) { return (int)std::min<long long>(((long long)v.blob_words + (long long)m->lds.total * v.epw * w) * 4, 1 << 30); };
  while (lds_of(1) > 160 * 1024 && m->spec < 0 && !m->jit && v.epw > 1) v.epw /= 2;
  int best = 1, best_per_cu = 0;
  for (int w = 1; w <= kMaxWavesPerBlock; ++w) {
    const int per_cu = lds_of(w) <= 160 * 1024 ? (160 * 1024 / lds_of(w)) * w : 0;
    if (per_cu > best_per_cu) { best = w; best_per_cu = per_cu; }
  }
  if (const char* e = getenv("MPPO_ENV_WAVES")) { const int w = atoi(e); if (w >= 1 && w <= kMaxWavesPerBlock) best = w; }
  m->waves = best;
  m->lds_bytes = lds_of(best);
  if (m->lds_bytes > 160 * 1024) return fail(MPPO_EMODEL, "model needs %d bytes of LDS per workgroup for ONE environment (limit 163840)", m->lds_bytes);
  return MPPO_OK;
}

// A kernel instantiation that MPPO_SPECIALIZE added to this build has never been compared with anything: before it is trusted, a reset and
// four steps of 24 environments under pseudo-random controls must equal the run-time-sized kernel's bit for bit ON THIS DEVICE.  If they do
// not (round 6: a 34-dof / 93-body robot's instantiation, 250 spilled registers, ended every episode at its first step on the GPU while the
// same source was right on the emulator - a per-lane flag spilled inside divergent code: `bad_mid` in env_kernel says how it ended), the model runs the run-time-sized kernel and
// says so on stderr.  A few milliseconds at mppo_model_open; the BASELINE instantiations are held to the same standard by the test suite.
// Work on the device the model's tables are on, whatever the calling thread's current device is (restored on the way out)
struct OnDeviceOf {
  int cur = -1, dev = -1;
  hipError_t err = hipSuccess;
  explicit OnDeviceOf([[maybe_unused]] const void* p) {
#ifndef MPPO_EMU
    hipPointerAttribute_t attr{};
    err = hipGetDevice(&cur);
    if (err == hipSuccess) err = hipPointerGetAttributes(&attr, p);
    if (err == hipSuccess) { dev = attr.device; if (dev != cur) err = hipSetDevice(dev); }
#endif
  }
  ~OnDeviceOf() {
#ifndef MPPO_EMU
    if (dev != cur && dev >= 0 && cur >= 0) (void)hipSetDevice(cur);
#endif
  }
};
static int32_t spec_self_check(mppo_model* m) {
  OnDeviceOf where(m->mv.blob);
  MPPO_CHECK_HIP(where.err);
  const ModelView& v = m->mv;
  const int N = 24, steps = 4, nu = v.nu > 0 ? v.nu : 1;
  const size_t nstate = (size_t)N * v.rec_dim, nobs = (size_t)N * v.obs_pad, nact = (size_t)N * nu;
  const size_t words = nstate + v.rec_dim + nobs + (size_t)steps * nact + N + N;  // state, reset record, observation, controls, reward, done
  float* dev = nullptr;
  MPPO_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&dev), words * sizeof(float)));
  std::vector<float> act((size_t)steps * nact), got[3];
  unsigned lcg = 12345u;
  for (float& x : act) { lcg = lcg * 1664525u + 1013904223u; x = ((lcg >> 8) & 0xffff) / 32768.f - 1.f; }
  float *state = dev, *reset_rec = state + nstate, *obs = reset_rec + v.rec_dim, *actd = obs + nobs, *rew = actd + (size_t)steps * nact;
  unsigned char* done = reinterpret_cast<unsigned char*>(rew + N);
  mppo_reward_cfg_t rc{};
  rc.height_min_z = -1e9f; rc.height_max_z = 1e9f;
  mppo_model generic = *m;
  generic.spec = -1; generic.jit = false; generic.scratch = nullptr; generic.scratch_bytes = 0;
  int32_t st = finalize_layout(&generic);
  // (an instantiation with a split step runs these 24 environments split - one wave per SIMD at the most: launch_env_spec - so it is run once more unsplit;
  // BOTH forms are held to the run-time-sized kernel)
  const bool has_split = m->spec >= 0 && !m->jit && !m->no_split && spec_has_split(m->spec);
  mppo_model unsplit = *m;
  unsplit.no_split = true; unsplit.scratch = nullptr; unsplit.scratch_bytes = 0;
  for (int which = 0; which < (has_split ? 3 : 2) && st == MPPO_OK; ++which) {
    const mppo_model* mm = which == 0 ? m : which == 1 ? &generic : &unsplit;
    hipError_t he = hipMemset(dev, 0, words * sizeof(float));
    if (he == hipSuccess) he = hipMemcpy(actd, act.data(), act.size() * sizeof(float), hipMemcpyHostToDevice);
    if (he != hipSuccess) { st = fail(MPPO_EHIP, "specialised-kernel self-check: %s", hipGetErrorString(he)); break; }
    st = env_reset_ws(mm, N, state, reset_rec, obs, v.obs_pad, rew, done, nullptr, nullptr, 0, nullptr, EnvDomain{});
    for (int t = 0; t < steps && st == MPPO_OK; ++t)
      st = env_step_ws(mm, N, 1, &rc, state, reset_rec, actd + (size_t)t * nact, nu, obs, v.obs_pad, rew, done, nullptr, nullptr, 0, nullptr);
    if (st != MPPO_OK) break;
    got[which].resize(words);
    he = hipDeviceSynchronize();
    if (he == hipSuccess) he = hipMemcpy(got[which].data(), dev, words * sizeof(float), hipMemcpyDeviceToHost);
    if (he != hipSuccess) st = fail(MPPO_EHIP, "specialised-kernel self-check: %s", hipGetErrorString(he));
  }
  (void)hipFree(dev);
  if (generic.scratch) (void)hipFree(generic.scratch);
  if (unsplit.scratch) (void)hipFree(unsplit.scratch);
  if (st != MPPO_OK) return st;
  if (has_split && memcmp(got[0].data(), got[1].data(), words * sizeof(float)) != 0 && memcmp(got[2].data(), got[1].data(), words * sizeof(float)) == 0) {
    // the split step alone differs: the model keeps its specialised kernel, unsplit at every size
    fprintf(stderr, "minppo_amd: the split form of the environment step specialised for this robot (nv %d, %d bodies, %d contact slots) differs from the run-time-sized kernel "
                    "after a reset and %d steps of %d environments on this device: NOT used - the unsplit form, which agrees, runs at every size.\n", v.nv, v.nbody, v.ncon, steps, N);
    m->no_split = true;
    return MPPO_OK;
  }
  if (has_split && memcmp(got[2].data(), got[1].data(), words * sizeof(float)) != 0) got[0] = got[2];  // (the unsplit form differs: reported and handled below)
  // (the controls are the same bytes in both; everything else is the kernels' output)
  if (memcmp(got[0].data(), got[1].data(), words * sizeof(float)) != 0) {
    size_t bad = 0;
    for (size_t i = 0; i < words; ++i) bad += memcmp(&got[0][i], &got[1][i], 4) != 0;
    fprintf(stderr, "minppo_amd: the environment kernel specialised for this robot (nv %d, %d bodies, %d contact slots) differs from the run-time-sized kernel in %zu of %zu "
                    "words after a reset and %d steps of %d environments on this device: NOT used - the run-time-sized kernel runs instead.  (DESIGN.md 3.3 has the one such kernel met so far; "
                    "minppo_amd/build.py names the build variable that keeps a specialised kernel's factorisation out of registers.)\n", v.nv, v.nbody, v.ncon, bad, words, steps, N);
    if (m->scratch) { (void)hipFree(m->scratch); m->scratch = nullptr; m->scratch_bytes = 0; }
    m->spec = -1;
    m->jit = false;
    return finalize_layout(m);
  }
  return MPPO_OK;
}
}  // namespace mppo

extern "C" int32_t mppo_model_open(const void* host_blob, size_t nbytes, const void* dev_blob, mppo_model_t** out) {
  using namespace mppo;
  if (!host_blob || !dev_blob || !out) return fail(MPPO_EINVAL, "mppo_model_open: null argument");
  // (a blob of a wrong SIZE is refused first, by the validator: the order of refusals is what it always was)
  if (nbytes >= 4 * (size_t)kBlobHeaderWords && !(nbytes & 3) && (reinterpret_cast<uintptr_t>(dev_blob) & 15) != 0) return fail(MPPO_EINVAL, "device blob must be 16-byte aligned");
  std::unique_ptr<mppo_model, int32_t (*)(mppo_model_t*)> m(new mppo_model(), &mppo_model_close);  // (a refusal below frees what the handle holds by then)
  BlobDims bd{};
  MPPO_TRY(parse_model_blob(host_blob, nbytes, &m->mv, &bd, &m->canon_words));
  m->mv.blob = static_cast<const int32_t*>(dev_blob);
  {
    const float* bm = static_cast<const float*>(host_blob) + m->mv.o[BF_body_mass];
    m->body_mass.assign(bm, bm + m->mv.nbody);
  }
  m->spec = generic_forced() ? -1 : find_spec(bd);
  MPPO_TRY(finalize_layout(m.get()));
  // every specialised instantiation proves itself on the device it is about to run on (a few milliseconds): the ones a build adds (MPPO_SPECIALIZE) always,
  // the default ones too on hardware - the test suite holds them bit-equal on the builder's toolchain, a user's compiler is another one (on the emulator the
  // suite itself is the check)
#ifdef MPPO_EMU
  const bool check = m->spec >= 0 && spec_is_extra(m->spec);
#else
  const bool check = m->spec >= 0;
#endif
  if (check) MPPO_TRY(spec_self_check(m.get()));
  *out = m.release();
  return MPPO_OK;
}

extern "C" int32_t mppo_model_close(mppo_model_t* m) {
  if (m && m->scratch) (void)hipFree(m->scratch);
  if (m && m->jit_module) (void)hipModuleUnload(m->jit_module);
  delete m;
  return MPPO_OK;
}

extern "C" int32_t mppo_model_attach_kernel(mppo_model_t* m, const void* image, size_t nbytes, const char* const* names, int32_t regchol_max_nv, int32_t* used) {
  using namespace mppo;
  if (!m || !image || !nbytes || !names || !names[0] || !names[1] || !names[2] || !used) return fail(MPPO_EINVAL, "mppo_model_attach_kernel: null argument");
  *used = 0;
  if (m->jit) return fail(MPPO_EINVAL, "mppo_model_attach_kernel: a code object is attached to this model already");
  if (regchol_max_nv < 0 || regchol_max_nv > 64) return fail(MPPO_EINVAL, "mppo_model_attach_kernel: regchol_max_nv %d", regchol_max_nv);
  if (m->spec >= 0) return MPPO_OK;  // (the library holds this robot's kernel itself)
  if (generic_forced()) return MPPO_OK;
  // the kernels' names spell the dimensions they were compiled for: StaticModel<the members of BlobDims, in their order>, MODE
  const BlobDims bd = blob_dims_of(m->mv);
  int dims[17]; static_assert(sizeof dims == sizeof bd, "StaticModel's 17 template parameters are the members of BlobDims, in their order");
  memcpy(dims, &bd, sizeof bd);
  char want[256];
  int o = snprintf(want, sizeof want, "StaticModelI");
  for (int d : dims) o += snprintf(want + o, sizeof want - o, "Li%dE", d);
  for (int k = 0; k < 3; ++k) {
    char mode[320];
    snprintf(mode, sizeof mode, "%sEELi%dEEEv", want, k);
    if (!strstr(names[k], "env_kernel") || !strstr(names[k], mode))
      return fail(MPPO_EINVAL, "mppo_model_attach_kernel: kernel %d is named %s - not the environment kernel of this robot's dimensions and mode (%s)", k, names[k], mode);
  }
  OnDeviceOf where(m->mv.blob);  // (a module belongs to the device it was loaded on)
  MPPO_CHECK_HIP(where.err);
  m->jit_image.assign(static_cast<const char*>(image), static_cast<const char*>(image) + nbytes);
  hipModule_t mod = nullptr;
  hipError_t he = hipModuleLoadData(&mod, m->jit_image.data());
  if (he != hipSuccess) { m->jit_image.clear(); return fail(MPPO_EHIP, "mppo_model_attach_kernel: the code object does not load (%s)", hipGetErrorString(he)); }
  auto drop = [&](int32_t rc) { (void)hipModuleUnload(mod); m->jit_module = nullptr; m->jit = false; m->jit_image.clear(); m->jit_image.shrink_to_fit(); return rc; };
  hipDeviceptr_t tag_ptr = nullptr;
  size_t tag_bytes = 0;
  unsigned tag = 0;
  he = hipModuleGetGlobal(&tag_ptr, &tag_bytes, mod, "mppo_env_kernel_tag");
  if (he == hipSuccess && tag_bytes == sizeof tag) he = hipMemcpy(&tag, tag_ptr, sizeof tag, hipMemcpyDeviceToHost);
  if (he != hipSuccess || tag_bytes != sizeof tag) return drop(fail(MPPO_EINVAL, "mppo_model_attach_kernel: the code object carries no mppo_env_kernel_tag (%s)", hipGetErrorString(he)));
  if (tag != kEnvKernelTag) return drop(fail(MPPO_EINVAL, "mppo_model_attach_kernel: the code object was compiled from other kernel sources than this library (tag %08x, library %08x)", tag, kEnvKernelTag));
  for (int k = 0; k < 3; ++k) {
    he = hipModuleGetFunction(&m->jit_fn[k], mod, names[k]);
    if (he != hipSuccess) return drop(fail(MPPO_EINVAL, "mppo_model_attach_kernel: no kernel %s in the code object (%s)", names[k], hipGetErrorString(he)));
  }
  // the pushed step and the pushed probe (KMODE 3, 4): the step's and the probe's symbols with the mode's digit replaced - a code object of these sources holds them
  for (int k = 1; k <= 2; ++k) {
    std::string name(names[k]);
    char from[16], to[16];
    snprintf(from, sizeof from, "EELi%dEEEv", k);
    snprintf(to, sizeof to, "EELi%dEEEv", k + 2);
    const size_t at = name.rfind(from);
    if (at == std::string::npos) return drop(fail(MPPO_EINVAL, "mppo_model_attach_kernel: kernel %d is named %s", k, names[k]));
    name.replace(at, strlen(from), to);
    he = hipModuleGetFunction(&m->jit_fn[k + 2], mod, name.c_str());
    if (he != hipSuccess) return drop(fail(MPPO_EINVAL, "mppo_model_attach_kernel: no kernel %s in the code object (%s)", name.c_str(), hipGetErrorString(he)));
  }
  // the randomised reset, step and probe (KMODE 6 .. 8): the three symbols with the mode's digit k replaced by 6 + k
  for (int k = 0; k <= 2; ++k) {
    std::string name(names[k]);
    char from[16], to[16];
    snprintf(from, sizeof from, "EELi%dEEEv", k);
    snprintf(to, sizeof to, "EELi%dEEEv", kEnvKernelRand + k);
    const size_t at = name.rfind(from);
    if (at == std::string::npos) return drop(fail(MPPO_EINVAL, "mppo_model_attach_kernel: kernel %d is named %s", k, names[k]));
    name.replace(at, strlen(from), to);
    he = hipModuleGetFunction(&m->jit_fn[kEnvKernelRand + k], mod, name.c_str());
    if (he != hipSuccess) return drop(fail(MPPO_EINVAL, "mppo_model_attach_kernel: no kernel %s in the code object (%s)", name.c_str(), hipGetErrorString(he)));
  }
  // the layout the specialised kernel computed for itself at compile time; then the same proof a build-time instantiation gives
  m->jit_module = mod;
  m->jit = true;
  m->jit_regchol = regchol_max_nv;
  if (m->scratch) { MPPO_CHECK_HIP(hipDeviceSynchronize()); (void)hipFree(m->scratch); m->scratch = nullptr; m->scratch_bytes = 0; }
  int32_t rc = finalize_layout(m);
  if (rc == MPPO_OK && m->jit) rc = spec_self_check(m);
  if (rc != MPPO_OK) { m->jit = false; (void)finalize_layout(m); return drop(rc); }
  if (!m->jit) return drop(MPPO_OK);  // (too large for four environments per wave, or it failed the check: the run-time-sized kernel stays)
  *used = 1;
  return MPPO_OK;
}

extern "C" int32_t mppo_model_scratch_bytes(const mppo_model_t* m, int32_t N, size_t* out) {
  if (!m || !out || N < 1) return mppo::fail(MPPO_EINVAL, "mppo_model_scratch_bytes: null argument or N < 1");
  *out = mppo::model_scratch_bytes(m, N);
  return MPPO_OK;
}

extern "C" int32_t mppo_model_get_dims(const mppo_model_t* m, mppo_model_dims_t* o) {
  if (!m || !o) return mppo::fail(MPPO_EINVAL, "mppo_model_get_dims: null argument");
  const mppo::ModelView& v = m->mv;
  o->nq = v.nq; o->nv = v.nv; o->nu = v.nu; o->nbody = v.nbody; o->njnt = v.njnt; o->ncon = v.ncon; o->nlimit = v.nlimit; o->nefc = v.nefc;
  o->obs_dim = v.obs_dim; o->obs_pad = v.obs_pad; o->rec_dim = v.rec_dim; o->lds_bytes = m->lds_bytes; o->timestep = v.timestep;
  return MPPO_OK;
}

extern "C" int32_t mppo_model_is_specialized(const mppo_model_t* m, int32_t* out) {
  if (!m || !out) return mppo::fail(MPPO_EINVAL, "mppo_model_is_specialized: null argument");
  *out = m->spec >= 0 ? 1 : m->jit ? 2 : 0;
  return MPPO_OK;
}

extern "C" int32_t mppo_env_reset(const mppo_model_t* m, int32_t N, float* state, float* reset_rec, float* obs, int32_t obs_ld,
                                  float* reward, uint8_t* done, const mppo_env_metrics_t* metrics, void* stream) {
  using namespace mppo;
  MPPO_REQUIRE(m && state && reset_rec, "mppo_env_reset: null model / state / reset_rec");
  MPPO_REQUIRE(N >= 1, "mppo_env_reset: N = %d", N);
  MPPO_REQUIRE(m->mv.nq >= 3, "mppo_env_reset: the environment reads qpos[2] as the height (env.py:239); nq = %d", m->mv.nq);
  MPPO_REQUIRE(!obs || obs_ld >= m->mv.obs_pad, "mppo_env_reset: obs_ld %d < padded observation width %d", obs_ld, m->mv.obs_pad);
  return env_reset_ws(m, N, state, reset_rec, obs, obs_ld, reward, done, metrics, nullptr, 0, static_cast<hipStream_t>(stream), EnvDomain{});
}

extern "C" int32_t mppo_env_reinit(const mppo_model_t* m, int32_t N, float* state, float* obs, int32_t obs_ld, const uint8_t* mask, float scale, int32_t rng_impl,
                                   uint64_t seed, int32_t rank, const uint32_t* key2, const int32_t* counter, int32_t counter_offset, void* stream) {
  using namespace mppo;
  MPPO_REQUIRE(m && state, "mppo_env_reinit: null model / state");
  MPPO_REQUIRE(N >= 1, "mppo_env_reinit: N = %d", N);
  MPPO_REQUIRE(m->mv.nq >= 3, "mppo_env_reinit: the environment reads qpos[2] as the height (env.py:239); nq = %d", m->mv.nq);
  MPPO_REQUIRE(!obs || obs_ld >= m->mv.obs_pad, "mppo_env_reinit: obs_ld %d < padded observation width %d", obs_ld, m->mv.obs_pad);
  MPPO_REQUIRE(scale >= 0.f, "mppo_env_reinit: scale %g is negative (or not a number)", (double)scale);
  MPPO_REQUIRE(rng_impl >= 0 && rng_impl <= 2, "mppo_env_reinit: rng_impl %d (0 philox, 1 threefry, 2 threefry from per-environment keys)", rng_impl);
  MPPO_REQUIRE(rng_impl == 0 || scale == 0.f || key2, "mppo_env_reinit: the threefry stream needs a key (two words in device memory)");
  MPPO_REQUIRE(rank >= 0 && rank < 256, "mppo_env_reinit: rank %d (0 .. 255)", rank);
  return env_reinit_ws(m, N, state, obs, obs_ld, mask, scale, rng_impl, seed, rank, key2, counter, 1, counter_offset, nullptr, 0, static_cast<hipStream_t>(stream), EnvDomain{});
}

extern "C" int32_t mppo_env_step(const mppo_model_t* m, int32_t N, int32_t n_frames, const mppo_reward_cfg_t* rc, float* state,
                                 const float* reset_rec, const float* action, int32_t act_ld, float* obs, int32_t obs_ld, float* reward,
                                 uint8_t* done, const mppo_env_metrics_t* metrics, void* stream) {
  using namespace mppo;
  MPPO_REQUIRE(m && rc && state && reset_rec && action && obs && reward && done, "mppo_env_step: null argument");
  MPPO_REQUIRE(N >= 1 && n_frames >= 1, "mppo_env_step: N = %d, n_frames = %d", N, n_frames);
  MPPO_REQUIRE(m->mv.nq >= 3, "mppo_env_step: the environment reads qpos[2] as the height (env.py:239); nq = %d", m->mv.nq);
  MPPO_REQUIRE(act_ld >= m->mv.nu, "mppo_env_step: act_ld %d < nu %d", act_ld, m->mv.nu);
  MPPO_REQUIRE(obs_ld >= m->mv.obs_pad, "mppo_env_step: obs_ld %d < padded observation width %d", obs_ld, m->mv.obs_pad);
  return env_step_ws(m, N, n_frames, rc, state, reset_rec, action, act_ld, obs, obs_ld, reward, done, metrics, nullptr, 0, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mppo_physics_forward(const mppo_model_t* m, int32_t N, const float* qpos, const float* qvel, const float* ctrl,
                                        const float* qacc_warmstart, const mppo_forward_probe_t* out, void* stream) {
  using namespace mppo;
  MPPO_REQUIRE(m && qpos && qvel && qacc_warmstart && out, "mppo_physics_forward: null argument");
  MPPO_REQUIRE(ctrl || m->mv.nu == 0, "mppo_physics_forward: ctrl is null but the model has actuators");
  MPPO_REQUIRE(N >= 1, "mppo_physics_forward: N = %d", N);
  EnvArgs a{};
  a.N = N; a.mode = 2; a.n_frames = 1; a.p_qpos = qpos; a.p_qvel = qvel; a.p_ctrl = ctrl; a.p_warm = qacc_warmstart; a.probe = *out;
  return launch_env(m, a, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mppo_env_step_xfrc(const mppo_model_t* m, int32_t N, int32_t n_frames, const mppo_reward_cfg_t* rc, float* state,
                                      const float* reset_rec, const float* action, int32_t act_ld, float* obs, int32_t obs_ld, float* reward,
                                      uint8_t* done, const mppo_env_metrics_t* metrics, int32_t body, const float* xfrc, void* stream) {
  using namespace mppo;
  MPPO_REQUIRE(m && rc && state && reset_rec && action && obs && reward && done, "mppo_env_step_xfrc: null argument");
  MPPO_REQUIRE(N >= 1 && n_frames >= 1, "mppo_env_step_xfrc: N = %d, n_frames = %d", N, n_frames);
  MPPO_REQUIRE(m->mv.nq >= 3, "mppo_env_step_xfrc: the environment reads qpos[2] as the height (env.py:239); nq = %d", m->mv.nq);
  MPPO_REQUIRE(act_ld >= m->mv.nu, "mppo_env_step_xfrc: act_ld %d < nu %d", act_ld, m->mv.nu);
  MPPO_REQUIRE(obs_ld >= m->mv.obs_pad, "mppo_env_step_xfrc: obs_ld %d < padded observation width %d", obs_ld, m->mv.obs_pad);
  if (xfrc) MPPO_TRY(check_push_body("mppo_env_step_xfrc", m, body));
  EnvPush push{};
  push.body = body; push.xfrc = xfrc;
  return env_step_push_ws(m, N, n_frames, rc, state, reset_rec, action, act_ld, obs, obs_ld, reward, done, metrics, push, nullptr, 0, static_cast<hipStream_t>(stream), EnvDomain{});
}

extern "C" int32_t mppo_physics_forward_xfrc(const mppo_model_t* m, int32_t N, const float* qpos, const float* qvel, const float* ctrl,
                                             const float* qacc_warmstart, const mppo_forward_probe_t* out, int32_t body, const float* xfrc, void* stream) {
  using namespace mppo;
  MPPO_REQUIRE(m && qpos && qvel && qacc_warmstart && out, "mppo_physics_forward_xfrc: null argument");
  MPPO_REQUIRE(ctrl || m->mv.nu == 0, "mppo_physics_forward_xfrc: ctrl is null but the model has actuators");
  MPPO_REQUIRE(N >= 1, "mppo_physics_forward_xfrc: N = %d", N);
  if (xfrc) MPPO_TRY(check_push_body("mppo_physics_forward_xfrc", m, body));
  EnvArgs a{};
  a.N = N; a.mode = 2; a.n_frames = 1; a.p_qpos = qpos; a.p_qvel = qvel; a.p_ctrl = ctrl; a.p_warm = qacc_warmstart; a.probe = *out;
  if (xfrc) { a.push_body = body; a.xfrc = xfrc; }
  return launch_env(m, a, static_cast<hipStream_t>(stream));
}

/* ---- domain randomisation: the entry points with a table (include/minppo_hip.h) ---- */
extern "C" int32_t mppo_env_reset_domain(const mppo_model_t* m, int32_t N, float* state, float* reset_rec, float* obs, int32_t obs_ld, float* reward, uint8_t* done,
                                         const mppo_env_metrics_t* metrics, const uint8_t* mask, const float* domain, int32_t mass_body, float scale, int32_t rng_impl,
                                         uint64_t seed, int32_t rank, const uint32_t* key2, const int32_t* counter, int32_t counter_offset, void* stream) {
  using namespace mppo;
  MPPO_REQUIRE(m && state, "mppo_env_reset_domain: null model / state");
  MPPO_REQUIRE(domain, "mppo_env_reset_domain: null table (domain, [N][4] floats in device memory)");
  MPPO_REQUIRE(N >= 1, "mppo_env_reset_domain: N = %d", N);
  MPPO_REQUIRE(m->mv.nq >= 3, "mppo_env_reset_domain: the environment reads qpos[2] as the height (env.py:239); nq = %d", m->mv.nq);
  MPPO_REQUIRE(!obs || obs_ld >= m->mv.obs_pad, "mppo_env_reset_domain: obs_ld %d < padded observation width %d", obs_ld, m->mv.obs_pad);
  MPPO_REQUIRE(scale >= 0.f, "mppo_env_reset_domain: scale %g is negative (or not a number)", (double)scale);
  MPPO_REQUIRE(rng_impl >= 0 && rng_impl <= 2, "mppo_env_reset_domain: rng_impl %d (0 philox, 1 threefry, 2 threefry from per-environment keys)", rng_impl);
  MPPO_REQUIRE(rng_impl == 0 || scale == 0.f || key2, "mppo_env_reset_domain: the threefry stream needs a key (two words in device memory)");
  MPPO_REQUIRE(rank >= 0 && rank < 256, "mppo_env_reset_domain: rank %d (0 .. 255)", rank);
  MPPO_TRY(check_domain_body("mppo_env_reset_domain", m, mass_body));
  MPPO_REQUIRE(m->mv.nq + m->mv.nv <= 4 * 65536, "reset noise: %d noise elements per environment", m->mv.nq + m->mv.nv);
  // (the reset kernel with everything it can be given: the full reset's outputs - each may be null - and the re-initialisation's mask and noise)
  EnvArgs a{};
  a.N = N; a.mode = 0; a.n_frames = 1; a.state = state; a.reset_out = reset_rec; a.obs = obs; a.obs_ld = obs_ld; a.reward = reward; a.done = done;
  if (metrics) a.met = *metrics;
  a.mask = mask; a.noise_scale = scale; a.noise_impl = rng_impl; a.noise_key = key2; a.noise_seed = seed;
  a.noise_stream = kStreamReset + ((unsigned long long)rank << 16);
  a.noise_ctr = counter; a.noise_ctr_mul = 1; a.noise_ctr_add = counter_offset;
  a.domain = domain; a.mass_body = mass_body;
  return launch_env(m, a, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mppo_env_step_domain(const mppo_model_t* m, int32_t N, int32_t n_frames, const mppo_reward_cfg_t* rc, float* state,
                                        const float* reset_rec, const float* action, int32_t act_ld, float* obs, int32_t obs_ld, float* reward,
                                        uint8_t* done, const mppo_env_metrics_t* metrics, int32_t push_body, const float* xfrc, const float* domain,
                                        int32_t mass_body, void* stream) {
  using namespace mppo;
  MPPO_REQUIRE(m && rc && state && reset_rec && action && obs && reward && done, "mppo_env_step_domain: null argument");
  MPPO_REQUIRE(domain, "mppo_env_step_domain: null table (domain, [N][4] floats in device memory)");
  MPPO_REQUIRE(N >= 1 && n_frames >= 1, "mppo_env_step_domain: N = %d, n_frames = %d", N, n_frames);
  MPPO_REQUIRE(m->mv.nq >= 3, "mppo_env_step_domain: the environment reads qpos[2] as the height (env.py:239); nq = %d", m->mv.nq);
  MPPO_REQUIRE(act_ld >= m->mv.nu, "mppo_env_step_domain: act_ld %d < nu %d", act_ld, m->mv.nu);
  MPPO_REQUIRE(obs_ld >= m->mv.obs_pad, "mppo_env_step_domain: obs_ld %d < padded observation width %d", obs_ld, m->mv.obs_pad);
  if (xfrc) MPPO_TRY(check_push_body("mppo_env_step_domain", m, push_body));
  MPPO_TRY(check_domain_body("mppo_env_step_domain", m, mass_body));
  EnvPush push{};
  push.body = xfrc ? push_body : 0; push.xfrc = xfrc;
  return env_step_push_ws(m, N, n_frames, rc, state, reset_rec, action, act_ld, obs, obs_ld, reward, done, metrics, push, nullptr, 0, static_cast<hipStream_t>(stream),
                          EnvDomain{domain, mass_body});
}

extern "C" int32_t mppo_physics_forward_domain(const mppo_model_t* m, int32_t N, const float* qpos, const float* qvel, const float* ctrl, const float* qacc_warmstart,
                                               const mppo_forward_probe_t* out, int32_t push_body, const float* xfrc, const float* domain, int32_t mass_body,
                                               void* stream) {
  using namespace mppo;
  MPPO_REQUIRE(m && qpos && qvel && qacc_warmstart && out, "mppo_physics_forward_domain: null argument");
  MPPO_REQUIRE(domain, "mppo_physics_forward_domain: null table (domain, [N][4] floats in device memory)");
  MPPO_REQUIRE(ctrl || m->mv.nu == 0, "mppo_physics_forward_domain: ctrl is null but the model has actuators");
  MPPO_REQUIRE(N >= 1, "mppo_physics_forward_domain: N = %d", N);
  if (xfrc) MPPO_TRY(check_push_body("mppo_physics_forward_domain", m, push_body));
  MPPO_TRY(check_domain_body("mppo_physics_forward_domain", m, mass_body));
  EnvArgs a{};
  a.N = N; a.mode = 2; a.n_frames = 1; a.p_qpos = qpos; a.p_qvel = qvel; a.p_ctrl = ctrl; a.p_warm = qacc_warmstart; a.probe = *out;
  if (xfrc) { a.push_body = push_body; a.xfrc = xfrc; }
  a.domain = domain; a.mass_body = mass_body;
  return launch_env(m, a, static_cast<hipStream_t>(stream));
}
