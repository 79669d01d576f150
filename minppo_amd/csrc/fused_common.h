// fused_common.h — what the row-pass kernels of k_fused.hip (fused_mlp_kernel, gather_rows_kernel) and fused_bf16.h (bf16_rowpass_kernel) share:
// the argument block, the LDS layout, the k-quad store helpers, the gather role and the phase timers.
#pragma once
#include <wave_ops.h>

#include "mppo_common.h"
#include "ppo_layout.h"
#include "wgrad.h"

namespace mppo {

// Phase timers (profiling builds only, -DMPPO_FUSED_TIMERS: tools/fused_phases.py): wave 0 of the first training workgroup stamps
// s_memtime at the phase boundaries into a device array that mppo_debug_fused_timers() copies out.  The macros test a compile-time
// `ROLLOUT` of the function they stand in (only training launches are stamped).
#ifdef MPPO_FUSED_TIMERS
__device__ unsigned long long g_fused_t[24 + 64];
#define FT(k) do { if (!ROLLOUT && blockIdx.x == 40 && blockIdx.y == 0 && threadIdx.x == 0) g_fused_t[k] = __builtin_amdgcn_s_memtime(); } while (0)
#define FTW(k) do { if (!ROLLOUT && blockIdx.x == 40 && blockIdx.y == 0 && (threadIdx.x & 63) == 0) g_fused_t[(k) + (threadIdx.x >> 6)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define FT(k) do { } while (0)
#define FTW(k) do { } while (0)
#endif

constexpr float kLog2PiF = 1.8378770664093453f;
constexpr int FRT = 16;  // rows per workgroup
#ifndef MPPO_ROLLOUT_WAVES
#define MPPO_ROLLOUT_WAVES 4
#endif
#ifndef MPPO_TRAIN_WAVES
#define MPPO_TRAIN_WAVES 2
#endif

__device__ __forceinline__ float fused_tanh(float x) {
  const float e = __expf(2.f * x);
  return 1.f - __fdividef(2.f, e + 1.f);
}

struct FusedArgs {
  int mb, O, OP, A, AP, DP, H, use_tanh;
  const float* params;
  ParamLayout L;
  mppo_batch_t b;
  const int* idx;
  const float* adv_stat;
  float inv_count;
  mppo_loss_cfg_t lc;
  float *h1[2], *h2[2], *dz2[2], *dz1[2];
  float *dout, *xmb, *partial;
  const float* w2t[2];  // W2^T shadow copies (W2T = true instantiations)
  const unsigned short* frag[2];  // bf16 fragment-order copies per network: W1 (KP x H) | W2 | W2^T (BF16 && W2T instantiations)
  // rollout mode (ROLLOUT = true): forward + pi.sample + pi.log_prob (train.py:157-160); rows are not gathered
  const float* noise;
  float *action, *log_prob, *value, *mean_out;
  int net0;  // first network of the launch: 0 = actor + critic, 1 = critic only (bootstrap value, train.py:182)
  // engine minibatch loop (PRE = true instantiations, ppo_layout.h XPre): this step's rows, already gathered, in k-quad layout; the
  // workgroups with blockIdx.y >= 2 gather the NEXT step's rows (idx_next) into xnext while the others compute.  They are
  // the LAST rows of the grid: workgroups are dispatched in linear order, so the gather fills the CUs the row tiles leave idle
  // (96 of 256 at the headline shape) and never delays a row tile (it did, by 2 us, as columns of the grid at 8192 environments)
  const float* xpre;
  float* xnext;
  const int* idx_next;
  int skip;  // timing experiments only (MPPO_FUSED_SKIP bit mask): 1 L1, 2 L2, 4 heads, 8 dZ2, 16 dZ1, 32 activation stores, 64 gather
};

// LDS of one fused_mlp_kernel workgroup, in floats: ROWS = 16 RT rows per tile, row strides XS (x tile: first-layer K padded to whole
// 32-k stages, + 4), HS (hidden tiles: H + 4) and SD (output-space tiles: 16 OT).  The +4 makes a ds_read_b128 of 4 consecutive k conflict-free.
//   xt [ROWS][XS]  x tile; then the partial head tiles s_hp [H/32 waves][RT][OT][64 lanes][4] (the x tile is dead between layer 1 and dZ2);
//                  then the dZ2 tile [ROWS][HS]
//   h1t, h2t [ROWS][HS] | s_do [ROWS][SD] d mean (cols < A, zero beyond), critic: col 0 = d value | s_red [ROWS][SD] d log_std terms | s_l [ROWS] per-row loss
// The host sizes the launch (fused_smem_bytes) and the device carves its pointers from the same members.
struct FusedLds {
  int KP, XS, HS, SD, rows, R0;
  __host__ __device__ FusedLds(int O, int H, int OT, int RT)
      : KP((O + 31) & ~31), XS(KP + 4), HS(H + 4), SD(16 * OT), rows(FRT * RT), R0(rows * (XS > HS ? XS : HS)) {}
  __host__ __device__ size_t floats() const { return (size_t)R0 + 2 * (size_t)rows * HS + 2 * (size_t)rows * SD + rows; }
  __device__ __forceinline__ float* xt(float* sm) const { return sm; }
  __device__ __forceinline__ float* h1t(float* sm) const { return sm + R0; }
  __device__ __forceinline__ float* h2t(float* sm) const { return h1t(sm) + rows * HS; }
  __device__ __forceinline__ float* s_do(float* sm) const { return h2t(sm) + rows * HS; }
  __device__ __forceinline__ float* s_red(float* sm) const { return s_do(sm) + rows * SD; }
  __device__ __forceinline__ float* s_l(float* sm) const { return s_red(sm) + rows * SD; }
  __device__ __forceinline__ float* s_hp(float* sm) const { return sm; }
};

// K-quad operands of the weight-gradient kernel.  Float network: one float4 per (quad of rows, column).  bf16 network (BF16 = true):
// the weight-gradient MFMAs round their operands to bf16 anyway, so the row pass stores them ROUNDED - 8 bytes per quad, the same
// index (quad_index) in units of bf16: half the bytes written here and read there, no conversion in the consumer, same results.
template <bool BF16>
__device__ __forceinline__ void store_quad(float* base, size_t qi, const float (&q)[4]) {
  if (BF16) stream_store(base + (qi >> 1), bf16x4_bits(pack_bf16x4(q[0], q[1], q[2], q[3])));
  else wt_store(base, qi, make_float4(q[0], q[1], q[2], q[3]));
}
// two adjacent columns (c0 even): 32 bytes as two float4, or 16 bytes of bf16
// WT: write-through (sc0 sc1) stores - the bytes leave this XCD's L2 while the kernel is still computing instead of waiting, dirty, for the
// end-of-kernel flush, and the weight-gradient launch finds them in memory: 13.9 -> 12.6 us there.  The row pass itself pays 0.9 us for it
// (a wave retires when its write-through stores are acknowledged); net 6.59 -> 6.555 ms per update.  All four operand stores or none:
// write-through for h1 / h2 / dZ2 and a streaming store for the last one (dZ1) measured 6.82 ms.
// float networks: SPLIT-PAIR column order inside a quad row (wgrad.h) - the even column of the lane's pair at qi, the odd one at qi2, half
// a quad row further: each of the two store instructions then writes whole lines across the lanes
template <bool BF16, bool WT = true>
__device__ __forceinline__ void store_quad2(float* base, size_t qi, size_t qi2, const float (&q0)[4], const float (&q1)[4]) {
  if (BF16) {
    const float2 a = bf16x4_bits(pack_bf16x4(q0[0], q0[1], q0[2], q0[3])), b = bf16x4_bits(pack_bf16x4(q1[0], q1[1], q1[2], q1[3]));
    if (WT) wt_store(base, qi >> 1, make_float4(a.x, a.y, b.x, b.y));
    else stream_store(base + (qi >> 1), make_float4(a.x, a.y, b.x, b.y));
  } else if (WT) {
    wt_store(base, qi, make_float4(q0[0], q0[1], q0[2], q0[3]));
    wt_store(base, qi2, make_float4(q1[0], q1[1], q1[2], q1[3]));
  } else {
    stream_store(base + qi, make_float4(q0[0], q0[1], q0[2], q0[3]));
    stream_store(base + qi2, make_float4(q1[0], q1[1], q1[2], q1[3]));
  }
}
// positions of the column pair (c0, c0 + 1), c0 even, of quad row `row` in an operand of `cols` columns: plain order for a bf16 network
// (one 16-byte store holds both), split-pair order for a float network
template <bool BF16>
__device__ __forceinline__ void pair_index(size_t row, size_t c0, size_t cols, size_t& qi, size_t& qi2) {
  if (BF16) { qi = quad_index(row, c0, cols); qi2 = qi + 4; }
  else { qi = ((row >> 2) * cols + (c0 >> 1)) * 4; qi2 = qi + (cols >> 1) * 4; }
}

// Gather role of a PRE launch: 16 rows of the NEXT minibatch (half = blockIdx.y picks two of the tile's four quads) from the
// trajectory into the k-quad buffer; rows past the minibatch are written as zeros (the buffer is an operand of the weight-gradient
// product and of the first layer).  Depends on the permutation only - it runs beside the workgroups that compute this step.
template <bool BF16>
__device__ __forceinline__ void gather_rows_tile(const FusedArgs& a, int tile, int half) {
  const int OP = a.OP, row0 = tile * FRT;
  for (int e = threadIdx.x; e < 2 * OP; e += blockDim.x) {
    const int qd = 2 * half + e / OP, c = e % OP;
    long ix[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = row0 + 4 * qd + j;
      ix[j] = a.idx_next[r < a.mb ? r : a.mb - 1];
    }
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float x = a.b.obs[ix[j] * a.b.obs_ld + c];
      v[j] = row0 + 4 * qd + j < a.mb ? x : 0.f;
    }
    store_quad<BF16>(a.xnext, quad_index(row0 + 4 * qd, c, OP), v);
  }
  // the same rows' scalars of the loss, behind the observation quads (ppo_layout.h xquad_floats): float4 = one column of four rows
  if (a.b.action) {
    const int A = a.A, SC = A + 4;
    float* sq = a.xnext + xquad_obs_floats(OP, a.mb);
    for (int e = threadIdx.x; e < 2 * SC; e += blockDim.x) {
      const int qd = 2 * half + e / SC, c = e % SC;
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = row0 + 4 * qd + j;
        const long ix = a.idx_next[r < a.mb ? r : a.mb - 1];
        const float x = c < A ? a.b.action[ix * a.b.act_ld + c] : c == A ? a.b.log_prob[ix] : c == A + 1 ? a.b.adv[ix] : c == A + 2 ? a.b.value[ix] : a.b.target[ix];
        v[j] = r < a.mb ? x : 0.f;
      }
      *reinterpret_cast<float4*>(sq + ((size_t)((row0 >> 2) + qd) * SC + c) * 4) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}

}  // namespace mppo
