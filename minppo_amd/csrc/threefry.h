// threefry.h — Threefry-2x32-20 and `jax.random.split` in the conventions of jax 0.4.3x (threefry_partitionable = False): shared by the
// stream kernels (k_rng.hip) and the environment kernel's reset noise (k_physics.hip).  Host restatement: minppo_amd/jaxrng.py.
#pragma once
#include <hip/hip_runtime.h>

namespace mppo {

struct U2 { unsigned x, y; };

__host__ __device__ inline unsigned rotl32(unsigned v, int r) { return (v << r) | (v >> (32 - r)); }

__host__ __device__ inline U2 threefry2x32(unsigned k0, unsigned k1, unsigned x0, unsigned x1) {
  const unsigned k2 = k0 ^ k1 ^ 0x1BD11BDAu;
  // (written out: indexed key / rotation tables end up in scratch memory on the device)
#define TF_MIX(R) { x0 += x1; x1 = rotl32(x1, R) ^ x0; }
#define TF_ROUNDS_A TF_MIX(13) TF_MIX(15) TF_MIX(26) TF_MIX(6)
#define TF_ROUNDS_B TF_MIX(17) TF_MIX(29) TF_MIX(16) TF_MIX(24)
  x0 += k0; x1 += k1;
  TF_ROUNDS_A x0 += k1; x1 += k2 + 1u;
  TF_ROUNDS_B x0 += k2; x1 += k0 + 2u;
  TF_ROUNDS_A x0 += k0; x1 += k1 + 3u;
  TF_ROUNDS_B x0 += k1; x1 += k2 + 4u;
  TF_ROUNDS_A x0 += k2; x1 += k0 + 5u;
#undef TF_ROUNDS_A
#undef TF_ROUNDS_B
#undef TF_MIX
  return {x0, x1};
}

// jax.random.split(key)[which]: threefry_2x32(key, [0, 1, 2, 3]) -> halves (0, 1 | 2, 3) -> out = [y0(0,2), y0(1,3), y1(0,2), y1(1,3)]
__host__ __device__ inline U2 split_key(U2 key, int which) {
  const U2 a = threefry2x32(key.x, key.y, 0u, 2u), b = threefry2x32(key.x, key.y, 1u, 3u);
  return which == 0 ? U2{a.x, b.x} : U2{a.y, b.y};
}

// word i of threefry_2x32(key, iota(n)), the bits behind jax.random.bits / uniform / split(key, n / 2): the counter array is split in
// halves (an odd n is padded with a 0 counter), the cipher runs on the pairs (first half, second half), the two output halves follow each other
__host__ __device__ inline unsigned threefry_iota_word(U2 key, unsigned i, unsigned n) {
  const unsigned half = (n + 1u) / 2u;
  if (i < half) return threefry2x32(key.x, key.y, i, i + half < n ? i + half : 0u).x;
  return threefry2x32(key.x, key.y, i - half, i).y;
}

// jax.random.split(key, num)[which]: words 2 which, 2 which + 1 of threefry_2x32(key, iota(2 num))
__host__ __device__ inline U2 split_key_n(U2 key, unsigned num, unsigned which) {
  return U2{threefry_iota_word(key, 2u * which, 2u * num), threefry_iota_word(key, 2u * which + 1u, 2u * num)};
}

// jax.random.uniform's float from 32 random bits (mantissa trick, then the clamp at the lower end): minval = lo, maxval = hi.  The product and
// the sum round separately, as the host statement's do
__host__ __device__ inline float uniform_from_bits(unsigned bits, float lo, float hi) {
  union { unsigned u; float f; } c;
  c.u = (bits >> 9) | 0x3F800000u;
  const float f = c.f - 1.0f;
#if defined(__HIP_DEVICE_COMPILE__)
  const float v = __fadd_rn(__fmul_rn(f, hi - lo), lo);
#else
  volatile float p = f * (hi - lo);
  const float v = p + lo;
#endif
  return v > lo ? v : lo;
}

}  // namespace mppo
