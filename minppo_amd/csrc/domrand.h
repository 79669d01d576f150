// domrand.h - domain randomisation: the draw of an environment's physical parameters, and what a launch is told about them.  Shared by the fill kernel
// (k_domrand.hip: the one-off launch that writes the table), the model handle (env_model.hip: the launches that read it) and the engine / the evaluator,
// which own a table; minppo_amd/jaxrng.py domain_params_philox restates the draw.
//
// Environment n owns the row (friction_scale, actuator_scale, added_mass, 0) of a device table domain[N][4], fixed for the whole run (legged_gym draws these
// at environment creation, MuJoCo Playground's domain_randomize once per vmapped model).  Stateless - a function of (seed, rank, environment) alone: no word in
// the state record, nothing in a checkpoint, a resumed run has the same robots.  With S = "DRAND" << 24 + (rank << 16):
//   r = philox(counter = {n, 0xFFFFFFFD, lo(S), hi(S)}, key = seed)
//   friction_scale = uniform_from_bits(r.x, fmin, fmax);  actuator_scale = uniform_from_bits(r.y, amin, amax);  added_mass = uniform_from_bits(r.z, mmin, mmax)
// min == max gives exactly that value (the product with hi - lo = 0 is 0, the sum lo, the clamp lo).  Only the multiply / add / clamp of uniform_from_bits: the
// host restatement is exact.
#pragma once
#include "mppo_common.h"
#include "philox.h"
#include "threefry.h"

namespace mppo {

constexpr unsigned long long kStreamDomain = 0x4452414E44ull << 24;  // "DRAND" (beside kStreamPush / kStreamReset / kStreamNoise / kStreamPerm)
constexpr unsigned kDomainCounter = 0xFFFFFFFDu;                       // word 1 of the counter (the pushes' phase has 0xFFFFFFFF in a stream of its own)

struct DomainDraw {
  float fmin, fmax, amin, amax, mmin, mmax;
  unsigned long long seed, stream;  // the key and the stream id (kStreamDomain + (rank << 16))
};

// row n of the table
__host__ __device__ inline void domain_draw(const DomainDraw& p, unsigned env, float* row4) {
  const U4 r = philox4x32(env, kDomainCounter, (unsigned)p.stream, (unsigned)(p.stream >> 32), (unsigned)p.seed, (unsigned)(p.seed >> 32));
  row4[0] = uniform_from_bits(r.x, p.fmin, p.fmax);
  row4[1] = uniform_from_bits(r.y, p.amin, p.amax);
  row4[2] = uniform_from_bits(r.z, p.mmin, p.mmax);
  row4[3] = 0.f;
}

// what a reset, step or re-initialisation launch is told: the table (null: the launch is not randomised and runs the kernels it always ran) and the payload's body
struct EnvDomain {
  const float* table;  // [N][4] device
  int body;            // 1 .. nbody - 1
};

// "the feature is on": some range differs from the identity row (1, 1, 0)
inline bool domain_cfg_on(const mppo_domain_cfg_t& c) {
  return !(c.friction_min == 1.f && c.friction_max == 1.f && c.actuator_min == 1.f && c.actuator_max == 1.f && c.mass_min == 0.f && c.mass_max == 0.f);
}

// env_model.hip: the refusals every entry point with a domain configuration shares (m null: the body and the mass are not checked against a model)
int32_t check_domain_cfg(const char* who, const mppo_model_t* m, const mppo_domain_cfg_t* c);
int32_t check_domain_body(const char* who, const mppo_model_t* m, int32_t body);
// k_domrand.hip: the table written out
int32_t domain_fill_launch(const mppo_domain_cfg_t& c, int N, float* domain, hipStream_t stream);

}  // namespace mppo
