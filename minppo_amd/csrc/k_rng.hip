// k_rng.hip — JAX-stream-compatible random numbers on the device: threefry2x32 keys, `jax.random.split`,
// `jax.random.normal` and the sort keys of `jax.random.permutation`, in the conventions of jax 0.4.3x
// (threefry_partitionable = False): reference minppo/train.py:158 (`pi.sample(seed=action_rng)`), :163, :252, :258.
// The host restatement these kernels are tested against, and the status of the claim, are in minppo_amd/jaxrng.py.
//   threefry_normal_kernel : jax.random.normal(key, (n,)): bits = threefry_2x32(key, iota(n)) with the counter array split in
//                            halves (thread i produces elements i and i + ceil(n/2)), uniform in (-1, 1) by the mantissa trick,
//                            sqrt(2) erf_inv(u) with XLA's float32 polynomial (Giles)
//   threefry_bits_kernel   : jax.random.bits(key, (n,)) + the identity permutation (first sort round)
//   threefry_chain_kernel  : the split tree of one `_update_step`, one thread: T x {action key, step key}, E x {epoch key ->
//                            one sub-key per sort round}; the carried key lives in the arena, so a captured graph draws fresh
//                            keys every replay.  The step keys (train.py:163: what `step_rngs` are split from) are written out when
//                            the caller asks for them: the environment kernel's reset noise draws from them (k_physics.hip)
#include <wave_ops.h>

#include "mppo_common.h"
#include "ppo_layout.h"
#include "threefry.h"

namespace mppo {

__device__ __forceinline__ float normal_from_bits(unsigned bits) {
  const float lo = -0.99999994f;  // nextafter(-1, 0)
  const float f = __uint_as_float((bits >> 9) | 0x3F800000u) - 1.0f;
  const float u = fmaxf(lo, f * (1.0f - lo) + lo);
  // XLA ErfInv32
  float w = -log1pf(-(u * u));
  const bool lt = w < 5.0f;
  w = lt ? w - 2.5f : sqrtf(w) - 3.0f;
  float p = lt ? 2.81022636e-08f : -0.000200214257f;
  p = (lt ? 3.43273939e-07f : 0.000100950558f) + p * w;
  p = (lt ? -3.5233877e-06f : 0.00134934322f) + p * w;
  p = (lt ? -4.39150654e-06f : -0.00367342844f) + p * w;
  p = (lt ? 0.00021858087f : 0.00573950773f) + p * w;
  p = (lt ? -0.00125372503f : -0.0076224613f) + p * w;
  p = (lt ? -0.00417768164f : 0.00943887047f) + p * w;
  p = (lt ? 0.246640727f : 1.00167406f) + p * w;
  p = (lt ? 1.50140941f : 2.83297682f) + p * w;
  return 1.41421354f * (p * u);
}

__global__ void __launch_bounds__(256) threefry_normal_kernel(const unsigned* __restrict__ key2, size_t n, float* __restrict__ out) {
  const size_t half = (n + 1) / 2, i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= half) return;
  const size_t j = i + half;
  const U2 y = threefry2x32(key2[0], key2[1], (unsigned)i, j < n ? (unsigned)j : 0u);  // the padding counter of an odd n is 0
  out[i] = normal_from_bits(y.x);
  if (j < n) out[j] = normal_from_bits(y.y);
}

__global__ void __launch_bounds__(256) threefry_bits_kernel(const unsigned* __restrict__ key2, size_t n, unsigned* __restrict__ out, int* __restrict__ iota) {
  const size_t half = (n + 1) / 2, i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= half) return;
  const size_t j = i + half;
  const U2 y = threefry2x32(key2[0], key2[1], (unsigned)i, j < n ? (unsigned)j : 0u);
  out[i] = y.x;
  if (iota) iota[i] = (int)i;
  if (j < n) { out[j] = y.y; if (iota) iota[j] = (int)j; }
}

__global__ void threefry_chain_kernel(unsigned* __restrict__ rng2, int T, int E, int rounds, unsigned* __restrict__ act_keys, unsigned* __restrict__ sort_keys,
                                      unsigned* __restrict__ step_keys) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  U2 rng{rng2[0], rng2[1]};
  for (int t = 0; t < T; ++t) {
    const U2 act = split_key(rng, 1);  // rng, action_rng = split(rng)   (train.py:158)
    rng = split_key(rng, 0);
    act_keys[2 * t] = act.x; act_keys[2 * t + 1] = act.y;
    if (step_keys) { const U2 stp = split_key(rng, 1); step_keys[2 * t] = stp.x; step_keys[2 * t + 1] = stp.y; }
    rng = split_key(rng, 0);           // rng, step_rng = split(rng)     (train.py:163; the step keys feed the reset noise, if there is any)
  }
  for (int e = 0; e < E; ++e) {
    U2 k = split_key(rng, 1);          // rng, _rng = split(rng)         (train.py:252)
    rng = split_key(rng, 0);
    for (int r = 0; r < rounds; ++r) {  // _shuffle: key, subkey = split(key) per sort round
      const U2 sub = split_key(k, 1);
      k = split_key(k, 0);
      sort_keys[2 * (e * rounds + r)] = sub.x; sort_keys[2 * (e * rounds + r) + 1] = sub.y;
    }
  }
  rng2[0] = rng.x; rng2[1] = rng.y;
}

int32_t threefry_normal(const unsigned* key2, size_t n, float* out, hipStream_t s) {
  hipLaunchKernelGGL(threefry_normal_kernel, dim3(cdiv((long)((n + 1) / 2), 256)), dim3(256), 0, s, key2, n, out);
  MPPO_CHECK_LAUNCH("threefry_normal_kernel");
  return MPPO_OK;
}
int32_t threefry_bits(const unsigned* key2, size_t n, unsigned* out, int* iota, hipStream_t s) {
  hipLaunchKernelGGL(threefry_bits_kernel, dim3(cdiv((long)((n + 1) / 2), 256)), dim3(256), 0, s, key2, n, out, iota);
  MPPO_CHECK_LAUNCH("threefry_bits_kernel");
  return MPPO_OK;
}
int32_t threefry_chain(unsigned* rng2, int T, int E, int rounds, unsigned* act_keys, unsigned* sort_keys, unsigned* step_keys, hipStream_t s) {
  hipLaunchKernelGGL(threefry_chain_kernel, dim3(1), dim3(64), 0, s, rng2, T, E, rounds, act_keys, sort_keys, step_keys);
  MPPO_CHECK_LAUNCH("threefry_chain_kernel");
  return MPPO_OK;
}

}  // namespace mppo

using namespace mppo;

extern "C" int32_t mppo_threefry_normal(const uint32_t* key2, size_t n, float* out, void* stream) {
  MPPO_REQUIRE(key2 && out && n >= 1, "mppo_threefry_normal: bad argument");
  return threefry_normal(key2, n, out, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mppo_threefry_bits(const uint32_t* key2, size_t n, uint32_t* out, void* stream) {
  MPPO_REQUIRE(key2 && out && n >= 1, "mppo_threefry_bits: bad argument");
  return threefry_bits(key2, n, out, nullptr, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mppo_threefry_update_keys(uint32_t* rng2, int32_t T, int32_t E, int32_t rounds, uint32_t* act_keys, uint32_t* sort_keys, void* stream) {
  MPPO_REQUIRE(rng2 && act_keys && sort_keys && T >= 1 && E >= 1 && rounds >= 1, "mppo_threefry_update_keys: bad argument");
  return threefry_chain(rng2, T, E, rounds, act_keys, sort_keys, nullptr, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mppo_threefry_update_keys_step(uint32_t* rng2, int32_t T, int32_t E, int32_t rounds, uint32_t* act_keys, uint32_t* sort_keys, uint32_t* step_keys,
                                                  void* stream) {
  MPPO_REQUIRE(rng2 && act_keys && sort_keys && step_keys && T >= 1 && E >= 1 && rounds >= 1, "mppo_threefry_update_keys_step: bad argument");
  return threefry_chain(rng2, T, E, rounds, act_keys, sort_keys, step_keys, static_cast<hipStream_t>(stream));
}
