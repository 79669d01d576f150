// deep_bf16.h — the row pass of a bf16 network with two hidden layers and an observation the fused kernels refuse (k_deep_bf16.hip:
// wide_bf16_kernel): its LDS layout and the launchers that k_ppo.hip dispatches to.  The argument block and the output buffers are
// deep_mlp_kernel's (deep.h: DeepArgs, plain row-major), so that everything behind the row pass runs unchanged.
#pragma once
#include "deep.h"

namespace mppo {

// LDS of one wide_bf16_kernel workgroup, in bytes.  The 16-row tiles that feed the bf16 matrix instructions (x, h1, dZ2) are kept ALREADY
// ROUNDED, 2 bytes per element: sixteen rows of O = 1575 are 52 KB against the float tile's 103 KB.  Row
// strides in bf16 elements: XSB = KP rounded up to 128, + 8 (x tile; KP = first-layer K padded to whole 32-k stages) and HSB = H + 8
// (H = 256) are 4 (mod 64) dwords, any other H 4 (mod 16): the sixteen rows of an 8-byte read of a quarter wave fall into different banks.
//   rollout : x | h1 | h2 (float, row stride HS = H + 4: the A operand of the exact head product) | s_hp [H/32][OT][64][4] head partials
//   training: the same, then dZ2 (bf16) | s_do | s_red [16][16 OT] | s_l [16]
// The x tile is RESIDENT or the geometry is refused (wide_bf16_supported): 160 KB take K up to 3392 at H = 256, A > 16.
// The host sizes the launch (bytes()) and the device carves its pointers from the same members.
struct WideBf16Lds {
  int KP, XSB, HSB, HS, SD, nw;
  bool rollout;
  __host__ __device__ WideBf16Lds(int O, int H, int OT, bool rollout_)
      : KP((O + 31) & ~31), XSB(((KP + 127) & ~127) + 8), HSB(H + 8), HS(H + 4), SD(16 * OT), nw(H / 32), rollout(rollout_) {}
  __host__ __device__ size_t x_bytes() const { return (size_t)kDeepRows * XSB * 2; }
  __host__ __device__ size_t hb_bytes() const { return (size_t)kDeepRows * HSB * 2; }
  __host__ __device__ size_t h2_bytes() const { return (size_t)kDeepRows * HS * 4; }
  __host__ __device__ size_t hp_bytes() const { return (size_t)nw * (SD / 16) * 256 * 4; }
  __host__ __device__ size_t bytes() const {
    const size_t fwd = x_bytes() + hb_bytes() + h2_bytes() + hp_bytes();
    return rollout ? fwd : fwd + hb_bytes() + (2 * (size_t)kDeepRows * SD + kDeepRows) * 4;
  }
  __host__ __device__ unsigned short* xb(unsigned char* sm) const { return reinterpret_cast<unsigned short*>(sm); }
  __host__ __device__ unsigned short* h1b(unsigned char* sm) const { return reinterpret_cast<unsigned short*>(sm + x_bytes()); }
  __host__ __device__ float* h2t(unsigned char* sm) const { return reinterpret_cast<float*>(sm + x_bytes() + hb_bytes()); }
  __host__ __device__ float* s_hp(unsigned char* sm) const { return reinterpret_cast<float*>(sm + x_bytes() + hb_bytes() + h2_bytes()); }
  __host__ __device__ unsigned short* dzb(unsigned char* sm) const { return reinterpret_cast<unsigned short*>(sm + x_bytes() + hb_bytes() + h2_bytes() + hp_bytes()); }
  __host__ __device__ float* s_do(unsigned char* sm) const { return reinterpret_cast<float*>(sm + x_bytes() + 2 * hb_bytes() + h2_bytes() + hp_bytes()); }
  __host__ __device__ float* s_red(unsigned char* sm) const { return s_do(sm) + kDeepRows * SD; }
  __host__ __device__ float* s_l(unsigned char* sm) const { return s_red(sm) + kDeepRows * SD; }
};

// k_deep_bf16.hip.  The predicates decide the dispatch in k_ppo.hip (policy_forward, minibatch_rowpass), which asks the fused kernels first: bf16
// network, two hidden layers, H a multiple of 32 in [32, 256], A <= 32, observation rows of stride OP (a multiple of 4) on a 16-byte boundary,
// and the layout above within kDeepLdsMax.
bool wide_bf16_supported(const mppo_net_t& net, const mppo_batch_t& b);
bool wide_bf16_rollout_supported(const mppo_net_t& net, const float* obs, int obs_ld);
int32_t wide_bf16_forward_backward(const mppo_net_t& net, const float* params, const mppo_batch_t& batch, const int* idx, int mb, const float* adv_stat,
                                   float inv_count, const mppo_loss_cfg_t& lc, const GradBufs& g, hipStream_t stream);
int32_t wide_bf16_policy_forward(const mppo_net_t& net, const float* params, int n, const float* obs, int obs_ld, const float* noise, float* action,
                                 float* log_prob, float* value, float* mean_out, int AP, hipStream_t stream);

}  // namespace mppo
