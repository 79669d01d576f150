// deep.h — the depth-generic row pass (k_deep.hip: deep_mlp_kernel) for networks of 1 to 4 hidden layers: its argument block, its LDS
// layout and the launchers that k_ppo.hip dispatches to.  Two hidden layers are fused_mlp_kernel's (k_fused.hip) wherever that kernel takes
// the geometry; nothing here touches it.
#pragma once
#include "ppo_layout.h"

namespace mppo {

constexpr int kDeepRows = 16;             // minibatch rows per workgroup (one 16 x 16 MFMA row tile)
constexpr size_t kDeepLdsMax = 160 * 1024;  // LDS of a CU: geometries beyond it are refused by the ..._supported predicates
constexpr int kDeepSlab = 96;             // streamed first layer: observation columns per LDS slab = one turn of the weight ring (3 stages of 32 k)
constexpr int kDeepSlabChunks = kDeepRows * kDeepSlab / 4;  // float4 pieces of a slab
constexpr int kDeepSlabQ = kDeepSlabChunks / 64;            // ... per thread of the narrowest workgroup (one wave)

struct DeepArgs {
  int mb, O, OP, A, AP, DP, H, nl, use_tanh;
  const float* params;
  int w[2][kMaxHidden + 1], b[2][kMaxHidden + 1], log_std;  // parameter offsets [network][layer]; layer nl = the output layer
  mppo_batch_t bt;
  const int* idx;  // training: row i of the tile is row idx[i] of the batch
  const float* adv_stat;
  float inv_count;
  mppo_loss_cfg_t lc;
  // training outputs, plain row-major (the layer-wise path's own buffers): activations and dZ [mb][H] per network and hidden layer,
  // dOut [mb][AP + 4], the gathered rows [mb][OP], one row of loss partials [4 + AP] per 16-row tile
  float *h[2][kMaxHidden], *dz[2][kMaxHidden];
  float *dout, *xmb, *partial;
  // rollout role: forward + pi.sample + pi.log_prob + value on rows 0 .. mb - 1 of bt.obs
  const float* noise;
  float *action, *log_prob, *value, *mean_out;
  int net0;  // first network of the launch: 0 actor (+ critic), 1 critic only
};

// LDS of one deep_mlp_kernel workgroup, in floats.  Row strides: XS = KP + 4 (x tile, first-layer K padded to whole 32-k stages),
// HS = H + 4 (hidden tiles), SD = 16 OT (output-space tiles); the + 4 makes a ds_read_b128 of four consecutive k conflict-free.
// T = 16 HS floats is one hidden tile, R0 = 16 max(XS, HS) the first region: the x tile, and a hidden-width tile once x is dead.
//   rollout : R0 + T.  Layer l reads tile l & 1 and writes tile (l + 1) & 1 (tile 0 = R0); the head partials s_hp [H/32][OT][64][4]
//             go over the tile the last layer READ (8 H OT <= T floats).
//   training: R0 + (L + 1) T + 2 * 16 SD + 16.  x | h_0 .. h_{L-1} (all kept: the backward reads act'(h_l) from them) | D1 | s_do | s_red | s_l.
//             The dZ tiles ping-pong between D0 = R0 (x is dead after layer 0) and D1: dZ_l lives in D(l & 1); s_hp shares D1.
//   streamed (stream = true: the resident layout is beyond a CU's LDS): the x tile is never resident.  The first region holds a ring of two
//             slabs of 16 x kDeepSlab observation columns, row stride XS = kDeepSlab + 4, slab s in half s & 1: R0 = 16 max(2 XS, HS) - for
//             H >= 196 no more than a hidden tile, whatever O.  Everything behind the first region is as above.
// The host sizes the launch (bytes()) and the device carves its pointers from the same members.
struct DeepLds {
  int KP, XS, HS, SD, T, R0, L;
  bool rollout;
  __host__ __device__ DeepLds(int O, int H, int OT, int L_, bool rollout_, bool stream)
      : KP((O + 31) & ~31), XS(stream ? kDeepSlab + 4 : KP + 4), HS(H + 4), SD(16 * OT), T(kDeepRows * HS),
        R0(kDeepRows * ((stream ? 2 * XS : XS) > HS ? (stream ? 2 * XS : XS) : HS)), L(L_), rollout(rollout_) {}
  __host__ __device__ size_t floats() const {
    return rollout ? (size_t)R0 + T : (size_t)R0 + (size_t)(L + 1) * T + 2 * (size_t)kDeepRows * SD + kDeepRows;
  }
  __host__ __device__ size_t bytes() const { return sizeof(float) * floats(); }
  __host__ __device__ float* xt(float* sm) const { return sm; }
  __host__ __device__ float* slab(float* sm, int s) const { return (s & 1) ? sm + kDeepRows * XS : sm; }        // streamed: slab s of the ring
  __host__ __device__ float* tile(float* sm, int k) const { return (k & 1) ? sm + R0 : sm; }                  // rollout ping-pong
  __host__ __device__ float* h(float* sm, int l) const { return sm + R0 + (size_t)l * T; }                     // training: hidden layer l
  __host__ __device__ float* dz(float* sm, int l) const { return (l & 1) ? sm + R0 + (size_t)L * T : sm; }     // training: dZ_l
  __host__ __device__ float* s_hp(float* sm, int last_in) const { return rollout ? tile(sm, last_in) : dz(sm, 1); }
  __host__ __device__ float* s_do(float* sm) const { return sm + R0 + (size_t)(L + 1) * T; }
  __host__ __device__ float* s_red(float* sm) const { return s_do(sm) + kDeepRows * SD; }
  __host__ __device__ float* s_l(float* sm) const { return s_red(sm) + kDeepRows * SD; }
};

// k_deep.hip.  The predicates decide the dispatch in k_ppo.hip (policy_forward, minibatch_rowpass), which asks the two-layer kernels first: depth 1 to 4,
// float network, H a multiple of 32 in [32, 256], A <= 32, observation rows of stride OP (a multiple of 4) on a 16-byte boundary.  Any O: the resident layout
// where it is within kDeepLdsMax, the streamed one otherwise.
bool deep_supported(const mppo_net_t& net, const mppo_batch_t& b);
bool deep_rollout_supported(const mppo_net_t& net, const float* obs, int obs_ld);
int32_t deep_forward_backward(const mppo_net_t& net, const float* params, const mppo_batch_t& batch, const int* idx, int mb, const float* adv_stat,
                              float inv_count, const mppo_loss_cfg_t& lc, const GradBufs& g, hipStream_t stream);
int32_t deep_policy_forward(const mppo_net_t& net, const float* params, int n, const float* obs, int obs_ld, const float* noise, float* action, float* log_prob,
                            float* value, float* mean_out, int AP, hipStream_t stream);

}  // namespace mppo
