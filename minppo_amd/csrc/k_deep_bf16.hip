// k_deep_bf16.hip — the row-local half of a minibatch step, and the rollout policy step, of a bf16 network (training.mlp_dtype = bf16) with two
// hidden layers whose observation is too wide for the fused kernels (k_fused.hip / fused_bf16.h: a weight-gradient tile table of 736 columns, a
// float x tile within 160 KB), in ONE launch:
//   x -> h1 -> h2 -> output layer -> clipped-PPO loss terms -> d(loss)/d(outputs) -> dZ2 -> dZ1
// The arithmetic is oracle/ppo_oracle.py's bf16 = True, rounding point for rounding point what fused_bf16.h computes at narrow O: operands
// rounded to bf16 (nearest even) in x.W1, h1.W2 and dZ2.W2^T with float accumulation; the output layer and dOut.W3^T exact float; activation
// derivatives from the float activations; whatever the weight-gradient products read as a B operand (dZ1, dZ2, dOut) is stored rounded, as
// floats, so that the column sums the bias gradients are made of are sums of the values the products multiply.
//
// Work split: deep_mlp_kernel's - one workgroup = 16 rows (training: gathered by permutation index) of ONE network (blockIdx.y: 0 actor,
// 1 critic), H/32 waves, wave w owns hidden columns [32w, 32w + 32) as two interleaved 16-column tiles - on v_mfma_f32_16x16x32_bf16: one
// instruction per tile and 32-k stage where the float kernel issues eight.
// Data movement (WideBf16Lds, deep_bf16.h): the x tile is RESIDENT in LDS, already rounded (2 bytes per element: 52 KB at O = 1575), so the
// first layer is one uninterrupted walk over K - no slab ring, no barrier inside it - up to K = 3392.  A thread owns ONE row of the tile (2H / 16 threads per row),
// resolves its index once and brings the row in as 16-byte pieces, four requests in flight.  h1 and dZ2 live in LDS as bf16, h2 as float (A
// operand of the exact head product); the lane's own float activations stay in its registers for the derivatives.
// Weights come from the FLOAT parameters and are rounded in registers (fused_pipes.h BStage: the ring's loads; packed to bf16 in front of the
// MFMA): the stand-alone entry points work from `params` alone and the engine's layer-wise optimizer step keeps no shadow copies (DESIGN.md
// 3.1e has the price).  Three-deep register ring as GemmPipe, one accumulation chain per ring slot and tile: six independent chains per wave.
// The output layer's weights and the rows' loss scalars are requested behind the first layer's loop - a phase ahead of their use, and out of
// the registers of the kernel's longest loop.
#include "deep_bf16.h"
#include "fused_common.h"
#include "fused_pipes.h"

namespace mppo {

// eight floats -> the bits of eight bf16 (round to nearest even): one operand of v_mfma_f32_16x16x32_bf16
__device__ __forceinline__ float4 bf16x8_bits(const float (&x)[8]) {
  const float2 lo = bf16x4_bits(pack_bf16x4(x[0], x[1], x[2], x[3])), hi = bf16x4_bits(pack_bf16x4(x[4], x[5], x[6], x[7]));
  return make_float4(lo.x, lo.y, hi.x, hi.y);
}
// two floats rounded to bf16, as floats
__device__ __forceinline__ float2 round2_bf16(float a, float b) {
  const unsigned u = __float_as_uint(bf16x4_bits(pack_bf16x4(a, b, 0.f, 0.f)).x);
  return make_float2(__uint_as_float(u << 16), __uint_as_float(u & 0xFFFF0000u));
}

// The weight stream of one bf16 product: GemmPipe's ring (fused_pipes.h: branch-free range-checked loads, stage S + 2 requested while stage S
// computes) in front of the 32-k bf16 instruction.  Stage S: the instruction's k slot 8 (lane >> 4) + 4 g + c carries k = 32 S + 16 g +
// 4 (lane >> 4) + c for A and B alike (frag_index's order): the A operand is the lane's two 8-byte LDS reads side by side, the B operand
// BStage's eight floats of a column, rounded.  `At`: a 16-row bf16 tile in LDS, row stride AS elements.
template <bool NT>
struct Bf16Ring {
  BStage<NT> b0, b1;
  BufView wb;
  __device__ __forceinline__ void prefetch(int K, int Kvalid, const float* W, int H, int n0, int lane) {
    const int j = lane & 15, kq = lane >> 4, last = K / 32 - 1;
    wb = make_buf(W, (unsigned)Kvalid * (unsigned)H * 4u);
    b0.load(W, wb, H, K, 0, n0, j, kq);
    b1.load(W, wb, H, K, last < 1 ? last : 1, n0, j, kq);
  }
  static __device__ __forceinline__ float4 read_a(const unsigned short* arow, int S) {
    const float2 a0 = *reinterpret_cast<const float2*>(arow + 32 * S), a1 = *reinterpret_cast<const float2*>(arow + 32 * S + 16);
    return make_float4(a0.x, a0.y, a1.x, a1.y);
  }
  static __device__ __forceinline__ void mma(const float4& A, const BStage<NT>& b, f32x4 (&acc)[2]) {
    mfma_bf16_16x16x32(A, bf16x8_bits(b.x0), acc[0]);
    mfma_bf16_16x16x32(A, bf16x8_bits(b.x1), acc[1]);
  }
  // acc[slot][tile]: the caller adds the three slots.  The A operands of a whole turn are read in front of it (an LDS round trip per stage
  // would stand between every two instructions of a chain).
  __device__ __forceinline__ void run(const unsigned short* At, int AS, int K, const float* W, int H, int n0, int lane, f32x4 (&acc)[3][2]) {
    const int j = lane & 15, kq = lane >> 4;
    const unsigned short* arow = At + j * AS + 4 * kq;
    const int nst = K / 32, last = nst - 1;
    BStage<NT> b2;
    int S = 0;
    for (; S + 2 < nst; S += 3) {
      const float4 a0 = read_a(arow, S), a1 = read_a(arow, S + 1), a2 = read_a(arow, S + 2);
      b2.load(W, wb, H, K, S + 2, n0, j, kq);
      MPPO_SCHED_FENCE();
      mma(a0, b0, acc[0]);
      MPPO_SCHED_FENCE();
      b0.load(W, wb, H, K, S + 3 < last ? S + 3 : last, n0, j, kq);
      MPPO_SCHED_FENCE();
      mma(a1, b1, acc[1]);
      MPPO_SCHED_FENCE();
      b1.load(W, wb, H, K, S + 4 < last ? S + 4 : last, n0, j, kq);
      MPPO_SCHED_FENCE();
      mma(a2, b2, acc[2]);
      MPPO_SCHED_FENCE();
    }
    if (S < nst) mma(read_a(arow, S), b0, acc[0]);
    if (S + 1 < nst) mma(read_a(arow, S + 1), b1, acc[1]);
  }
};

template <bool ROLLOUT, int OT>
__global__ void __launch_bounds__(512, 2) wide_bf16_kernel(DeepArgs a) {
  constexpr int SD = 16 * OT;  // row stride of the per-row output-space tiles
  MPPO_DYN_SMEM(smem_raw);
  const int H = a.H, O = a.O, OP = a.OP, A = a.A, AP = a.AP;
  const int net = blockIdx.y + (ROLLOUT ? a.net0 : 0);  // 0 actor, 1 critic
  const WideBf16Lds lds(O, H, OT, ROLLOUT);             // the layout the host sized the launch from
  const int KP = lds.KP, XSB = lds.XSB, HSB = lds.HSB, HS = lds.HS;
  unsigned short *xb = lds.xb(smem_raw), *h1b = lds.h1b(smem_raw);
  float *h2t = lds.h2t(smem_raw), *s_hp = lds.s_hp(smem_raw);
  const int t = threadIdx.x, nthr = blockDim.x, lane = t & 63, wave = t >> 6;
  const int row0 = blockIdx.x * kDeepRows;
  const bool tanh_act = net == 0 && a.use_tanh;
  const int nout = net ? 1 : A;
  const int n0 = 32 * wave, cj = lane & 15, rq = lane >> 4, c0 = n0 + 2 * cj;
  const bool gather = !ROLLOUT && a.idx;
  const float* W1 = a.params + a.w[net][0];
  const float* W2 = a.params + a.w[net][1];

  // ---- the first two stages of W1 (they depend on nothing computed here) ----
  Bf16Ring<false> fwd;
  fwd.prefetch(KP, O, W1, H, n0, lane);
  const float2 bz1 = *reinterpret_cast<const float2*>(a.params + a.b[net][0] + c0), bz2 = *reinterpret_cast<const float2*>(a.params + a.b[net][1] + c0);

  // ---- P0: observation rows -> LDS, rounded.  Thread t owns row t / tpr of the tile and every tpr-th 16-byte piece of it; four pieces are requested
  // together (clamped addresses, masked uses).  Columns O .. KP - 1 are written as zeros: the weight view returns zeros for those k as well, and
  // what lies behind an observation's O columns need not be finite.  The actor workgroup also writes the gathered rows [mb][OP] (raw floats: A
  // operand of the first layer's weight gradient, rounded there). ----
  {
    const int tpr = nthr >> 4, xr = t / tpr, xc = t - xr * tpr, kp4 = KP >> 2;
    const int gi = row0 + xr < a.mb ? row0 + xr : a.mb - 1;
    const float* xsrc = a.bt.obs + (gather ? (long)a.idx[gi] : (long)gi) * a.bt.obs_ld;
    const bool xst = !ROLLOUT && net == 0 && row0 + xr < a.mb;
    unsigned short* xdst = xb + xr * XSB;
    for (int cb = xc; cb < kp4; cb += 4 * tpr) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int c = 4 * (cb + u * tpr);
        v[u] = *reinterpret_cast<const float4*>(xsrc + (c < OP ? c : OP - 4));
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int c = 4 * (cb + u * tpr);
        if (c < KP) {
          const bf16x4 p = pack_bf16x4(c < O ? v[u].x : 0.f, c + 1 < O ? v[u].y : 0.f, c + 2 < O ? v[u].z : 0.f, c + 3 < O ? v[u].w : 0.f);
          *reinterpret_cast<float2*>(xdst + c) = bf16x4_bits(p);
          if (xst && c < OP) stream_store(a.xmb + (size_t)(row0 + xr) * OP + c, v[u]);
        }
      }
    }
  }
  __syncthreads();

  // ---- layer 1: h1 = act(x . W1 + b1), one walk over K ----
  f32x4 acc[3][2];
  auto acc_zero = [&]() {
#pragma unroll
    for (int s = 0; s < 3; ++s)
      for (int r = 0; r < 4; ++r) { acc[s][0][r] = 0.f; acc[s][1][r] = 0.f; }
  };
  acc_zero();
  fwd.run(xb, XSB, KP, W1, H, n0, lane, acc);
  // ---- requested now, consumed phases later: the first two stages of W2, the output layer's weights and biases, the rows' scalars of the loss ----
  fwd.prefetch(H, H, W2, H, n0, lane);
  const float* W3 = a.params + a.w[net][2];
  const float* B3 = a.params + a.b[net][2];
  const float adv_mean = ROLLOUT ? 0.f : a.adv_stat[0], adv_rstd = ROLLOUT ? 1.f : a.adv_stat[1];
  float ls[OT], b3v[OT];  // output o = cj + 16 ot of this lane
#pragma unroll
  for (int ot = 0; ot < OT; ++ot) {
    const int o = cj + 16 * ot;
    ls[ot] = (net == 0 && o < A) ? a.params[a.log_std + o] : 0.f;
    b3v[ot] = o < nout ? B3[o] : 0.f;
  }
  // w3p: B operands of the head product (k = 32 wave + 16 g + 4 rq + c, output o); w3q: B operands of dZ2 = dOut . W3^T (hidden columns c0,
  // c0 + 1; contracted output 4 m + rq)
  float w3p[OT][8], w3q[4 * OT][2];
#pragma unroll
  for (int ot = 0; ot < OT; ++ot)
#pragma unroll
    for (int gc = 0; gc < 8; ++gc) {
      const int o = cj + 16 * ot, k = n0 + 16 * (gc >> 2) + 4 * rq + (gc & 3);
      w3p[ot][gc] = o < nout ? W3[k * nout + o] : 0.f;
    }
  if (!ROLLOUT) {
#pragma unroll
    for (int m = 0; m < 4 * OT; ++m) {
      const int ai = 4 * m + rq;
      w3q[m][0] = ai < nout ? W3[c0 * nout + ai] : 0.f;
      w3q[m][1] = ai < nout ? W3[(c0 + 1) * nout + ai] : 0.f;
    }
  }
  // actor: action[o], old log_prob, advantage | critic: old value, target | rollout: noise[o].  Raw loads on clamped addresses; every use is masked.
  long prow[4];
  bool pon[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = row0 + 4 * rq + r;
    pon[r] = i < a.mb;
    const int ic = pon[r] ? i : a.mb - 1;
    prow[r] = gather ? (long)a.idx[ic] : (long)ic;
  }
  float pf0[OT][4], pf1[4], pf2[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    pf1[r] = pf2[r] = 0.f;
#pragma unroll
    for (int ot = 0; ot < OT; ++ot) pf0[ot][r] = 0.f;
  }
  if (ROLLOUT) {
    if (net == 0 && a.noise) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int ot = 0; ot < OT; ++ot) {
          const int o = cj + 16 * ot;
          const float v = a.noise[(size_t)prow[r] * A + (o < A ? o : A - 1)];
          pf0[ot][r] = (pon[r] && o < A) ? v : 0.f;
        }
    }
  } else if (net == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int ot = 0; ot < OT; ++ot) {
        const int o = cj + 16 * ot;
        pf0[ot][r] = a.bt.action[prow[r] * a.bt.act_ld + (o < A ? o : A - 1)];
      }
      pf1[r] = a.bt.log_prob[prow[r]];
      pf2[r] = a.bt.adv[prow[r]];
    }
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      pf0[0][r] = a.bt.value[prow[r]];
      pf1[r] = a.bt.target[prow[r]];
    }
  }
  float h1r[2][4], h2r[2][4];  // the lane's own float activations (columns c0, c0 + 1 of rows 4 rq .. 4 rq + 3): the derivatives' inputs
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int rr = 4 * rq + r;
    float v0 = acc[0][0][r] + acc[1][0][r] + acc[2][0][r] + bz1.x, v1 = acc[0][1][r] + acc[1][1][r] + acc[2][1][r] + bz1.y;
    if (tanh_act) { v0 = fused_tanh(v0); v1 = fused_tanh(v1); } else { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); }
    h1r[0][r] = v0; h1r[1][r] = v1;
    *reinterpret_cast<float*>(h1b + rr * HSB + c0) = bf16x4_bits(pack_bf16x4(v0, v1, 0.f, 0.f)).x;
    if (!ROLLOUT && row0 + rr < a.mb) stream_store(a.h[net][0] + (size_t)(row0 + rr) * H + c0, make_float2(v0, v1));
  }
  __syncthreads();

  // ---- layer 2: h2 = act(h1 . W2 + b2); the backward product's first stages arrive under its epilogue, the heads and the loss ----
  Bf16Ring<true> bwd;
  acc_zero();
  fwd.run(h1b, HSB, H, W2, H, n0, lane, acc);
  if (!ROLLOUT) bwd.prefetch(H, H, W2, H, n0, lane);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int rr = 4 * rq + r;
    float v0 = acc[0][0][r] + acc[1][0][r] + acc[2][0][r] + bz2.x, v1 = acc[0][1][r] + acc[1][1][r] + acc[2][1][r] + bz2.y;
    if (tanh_act) { v0 = fused_tanh(v0); v1 = fused_tanh(v1); } else { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); }
    h2r[0][r] = v0; h2r[1][r] = v1;
    *reinterpret_cast<float2*>(h2t + rr * HS + c0) = make_float2(v0, v1);
    if (!ROLLOUT && row0 + rr < a.mb) stream_store(a.h[net][1] + (size_t)(row0 + rr) * H + c0, make_float2(v0, v1));
  }
  __syncthreads();

  // ---- output layer, exact float: OT 16 x 16 tiles (rows x outputs), K = H split over the waves, partial tiles summed through LDS ----
  {
    f32x4 hp[OT];
#pragma unroll
    for (int ot = 0; ot < OT; ++ot)
      for (int r = 0; r < 4; ++r) hp[ot][r] = 0.f;
    const float* arow = h2t + cj * HS + 4 * rq + n0;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const float4 av = *reinterpret_cast<const float4*>(arow + 16 * g);
#pragma unroll
      for (int ot = 0; ot < OT; ++ot) {
        mfma_f32_16x16x4(av.x, w3p[ot][4 * g + 0], hp[ot]); mfma_f32_16x16x4(av.y, w3p[ot][4 * g + 1], hp[ot]);
        mfma_f32_16x16x4(av.z, w3p[ot][4 * g + 2], hp[ot]); mfma_f32_16x16x4(av.w, w3p[ot][4 * g + 3], hp[ot]);
      }
    }
#pragma unroll
    for (int ot = 0; ot < OT; ++ot)
      *reinterpret_cast<float4*>(s_hp + ((wave * OT + ot) * 64 + lane) * 4) = make_float4(hp[ot][0], hp[ot][1], hp[ot][2], hp[ot][3]);
  }
  __syncthreads();
  // every wave adds the partial tiles in the same order: lane (cj, rq) holds out[ot][r] = output cj + 16 ot of row 4 rq + r, so that a row's
  // outputs span one 16-lane DPP row and row reductions are group16 sums.  Only wave 0 stores.
  float out[OT][4];
  const int nw = nthr >> 6;
#pragma unroll
  for (int ot = 0; ot < OT; ++ot) {
    out[ot][0] = out[ot][1] = out[ot][2] = out[ot][3] = 0.f;
    for (int w = 0; w < nw; ++w) {
      const float4 q = *reinterpret_cast<const float4*>(s_hp + ((w * OT + ot) * 64 + lane) * 4);
      out[ot][0] += q.x; out[ot][1] += q.y; out[ot][2] += q.z; out[ot][3] += q.w;
    }
  }
  const bool st = wave == 0;
  float sum_ls_l = 0.f;
#pragma unroll
  for (int ot = 0; ot < OT; ++ot) sum_ls_l += ls[ot];
  if (ROLLOUT) {
    // pi.sample + pi.log_prob (train.py:158-160) / value (train.py:157,182): deep_mlp_kernel's arithmetic, statement for statement
    if (net == 0) {
      const float sum_ls = group16_sum(sum_ls_l);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = row0 + 4 * rq + r;
        const bool on = i < a.mb;
        float z2 = 0.f;
#pragma unroll
        for (int ot = 0; ot < OT; ++ot) {
          const int o = cj + 16 * ot;
          if (on && o < A) {
            const float mean = out[ot][r] + b3v[ot];
            const float act = mean + __expf(ls[ot]) * pf0[ot][r];
            const float z = (act - mean) * __expf(-ls[ot]);
            z2 += z * z;
            if (st) {
              a.action[(size_t)i * A + o] = act;
              if (a.mean_out) a.mean_out[(size_t)i * AP + o] = mean;
            }
          }
        }
        const float ss = group16_sum(z2);
        if (st && on && cj == 0) a.log_prob[i] = -0.5f * ss - sum_ls - 0.5f * (float)A * kLog2PiF;
      }
    } else {
      const float b3c = group16_sum(b3v[0]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = row0 + 4 * rq + r;
        const float v = group16_sum(cj == 0 ? out[0][r] : 0.f) + b3c;
        if (st && i < a.mb && cj == 0) a.value[i] = v;
      }
    }
    return;
  }
  // ---- loss terms and d loss / d outputs (train.py:223-243; deep_mlp_kernel's arithmetic).  dOut goes to LDS exact (A operand of the exact
  // dOut . W3^T) and to memory rounded (B operand of the output layer's weight gradient, and its bias gradient's terms) ----
  unsigned short* dzb = lds.dzb(smem_raw);
  float *s_do = lds.s_do(smem_raw), *s_red = lds.s_red(smem_raw), *s_l = lds.s_l(smem_raw);
  if (net == 0) {
    const float sum_ls = group16_sum(sum_ls_l);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = 4 * rq + r, i = row0 + rr;
      const bool on = i < a.mb;
      float z[OT], zz = 0.f;
#pragma unroll
      for (int ot = 0; ot < OT; ++ot) {
        z[ot] = 0.f;
        if (on && cj + 16 * ot < A) z[ot] = (pf0[ot][r] - (out[ot][r] + b3v[ot])) * __expf(-ls[ot]);
        zz += z[ot] * z[ot];
      }
      const float ss = group16_sum(zz);
      float la = 0.f, dlogp = 0.f;
      if (on) {
        const float logp = -0.5f * ss - sum_ls - 0.5f * (float)A * kLog2PiF;
        const float ratio = __expf(logp - pf1[r]);
        const float g = (pf2[r] - adv_mean) * adv_rstd;
        const float la1 = ratio * g;
        const float la2 = fminf(fmaxf(ratio, 1.f - a.lc.clip_eps), 1.f + a.lc.clip_eps) * g;
        la = -fminf(la1, la2) * a.inv_count;
        const bool unclipped = (ratio >= 1.f - a.lc.clip_eps) && (ratio <= 1.f + a.lc.clip_eps);
        dlogp = (unclipped || la1 < la2) ? -g * ratio * a.inv_count : 0.f;
      }
      if (st) {
#pragma unroll
        for (int ot = 0; ot < OT; ++ot) {
          const int o = cj + 16 * ot;
          const float dm = (on && o < A) ? dlogp * z[ot] * __expf(-ls[ot]) : 0.f;
          s_do[rr * SD + o] = dm;
          s_red[rr * SD + o] = o < A ? dlogp * (z[ot] * z[ot] - 1.f) : 0.f;
          if (on && o < AP) a.dout[(size_t)i * a.DP + o] = round2_bf16(dm, 0.f).x;  // d mean in columns [0, A), zeros up to AP
        }
        if (cj == 0) s_l[rr] = la;
      }
    }
  } else {
    const float b3c = group16_sum(b3v[0]);  // lane cj = 0 holds the critic's single output bias
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = 4 * rq + r, i = row0 + rr;
      const bool on = i < a.mb;
      const float vnew = group16_sum(cj == 0 ? out[0][r] : 0.f) + b3c;
      float lv = 0.f, dv = 0.f;
      if (on) {
        const float ov = pf0[0][r], tg = pf1[r];
        const float vc = ov + fminf(fmaxf(vnew - ov, -a.lc.clip_eps), a.lc.clip_eps);
        const float vl1 = (vnew - tg) * (vnew - tg), vl2 = (vc - tg) * (vc - tg);
        lv = 0.5f * fmaxf(vl1, vl2) * a.inv_count;
        const bool vin = fabsf(vnew - ov) <= a.lc.clip_eps;
        dv = (vin || vl1 > vl2) ? (vnew - tg) * a.inv_count * a.lc.vf_coef : 0.f;
      }
      if (st) {
#pragma unroll
        for (int ot = 0; ot < OT; ++ot) s_do[rr * SD + cj + 16 * ot] = (cj == 0 && ot == 0) ? dv : 0.f;
        if (cj == 0) s_l[rr] = lv;
        if (on && cj < 4) a.dout[(size_t)i * a.DP + AP + cj] = cj == 0 ? round2_bf16(dv, 0.f).x : 0.f;  // d value in column AP, zeros in AP + 1 .. AP + 3
      }
    }
  }
  __syncthreads();
  // one row of loss partials per tile: column 0 actor loss, 1 value loss, 4 + o d log_std[o]
  {
    float* prow_out = a.partial + (size_t)blockIdx.x * (4 + AP);
    if (net == 0) {
      if (t == 0) { float s = 0.f; for (int r = 0; r < kDeepRows; ++r) s += s_l[r]; prow_out[0] = s; }
      if (t == 2 || t == 3) prow_out[t] = 0.f;
      if (t >= 4 && t < 4 + AP) { float s = 0.f; if (t - 4 < A) for (int r = 0; r < kDeepRows; ++r) s += s_red[r * SD + (t - 4)]; prow_out[t] = s; }
    } else if (t == 0) {
      float s = 0.f; for (int r = 0; r < kDeepRows; ++r) s += s_l[r]; prow_out[1] = s;
    }
  }
  // ---- dZ2 = (dOut . W3^T) * act'(h2), exact float product -> LDS as bf16 (the backward product's A operand) + memory, rounded ----
  {
    f32x4 d0, d1;
    for (int r = 0; r < 4; ++r) { d0[r] = 0.f; d1[r] = 0.f; }
#pragma unroll
    for (int m = 0; m < 4 * OT; ++m) {
      const float av = s_do[cj * SD + 4 * m + rq];
      mfma_f32_16x16x4(av, w3q[m][0], d0); mfma_f32_16x16x4(av, w3q[m][1], d1);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = 4 * rq + r;
      const float hx = h2r[0][r], hy = h2r[1][r];
      const float z0 = tanh_act ? d0[r] * (1.f - hx * hx) : (hx > 0.f ? d0[r] : 0.f);
      const float z1 = tanh_act ? d1[r] * (1.f - hy * hy) : (hy > 0.f ? d1[r] : 0.f);
      *reinterpret_cast<float*>(dzb + rr * HSB + c0) = bf16x4_bits(pack_bf16x4(z0, z1, 0.f, 0.f)).x;
      if (row0 + rr < a.mb) stream_store(a.dz[net][1] + (size_t)(row0 + rr) * H + c0, round2_bf16(z0, z1));
    }
  }
  __syncthreads();
  // ---- dZ1 = (dZ2 . W2^T) * act'(h1): W2 as stored ([H][H], rows = inputs: float4 along the contraction), no shadow copy ----
  {
    acc_zero();
    bwd.run(dzb, HSB, H, W2, H, n0, lane, acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = 4 * rq + r;
      const float s0 = acc[0][0][r] + acc[1][0][r] + acc[2][0][r], s1 = acc[0][1][r] + acc[1][1][r] + acc[2][1][r];
      const float gx = h1r[0][r], gy = h1r[1][r];
      const float z0 = tanh_act ? s0 * (1.f - gx * gx) : (gx > 0.f ? s0 : 0.f);
      const float z1 = tanh_act ? s1 * (1.f - gy * gy) : (gy > 0.f ? s1 : 0.f);
      if (row0 + rr < a.mb) stream_store(a.dz[net][0] + (size_t)(row0 + rr) * H + c0, round2_bf16(z0, z1));
    }
  }
}

// ---- every instantiation the library launches; the dynamic-LDS attribute is set on exactly these ----
using WideBf16Fn = void (*)(DeepArgs);
struct WideBf16Kernel { bool rollout; int ot; WideBf16Fn fn; };
static const WideBf16Kernel kWideBf16Kernels[] = {{false, 1, wide_bf16_kernel<false, 1>}, {false, 2, wide_bf16_kernel<false, 2>},
                                                  {true, 1, wide_bf16_kernel<true, 1>}, {true, 2, wide_bf16_kernel<true, 2>}};

static WideBf16Lds wide_bf16_lds(const mppo_net_t& net, bool rollout) { return WideBf16Lds(net.O, net.H, net.A > 16 ? 2 : 1, rollout); }

static bool wide_bf16_geometry(const mppo_net_t& net, const float* obs, int obs_ld, bool rollout) {
  return net.bf16 && net_layers(net) == 2 && net.H % 32 == 0 && net.H >= 32 && net.H <= 256 && net.A <= 32 && obs_ld == net.OP && (net.OP % 4) == 0 &&
         (reinterpret_cast<uintptr_t>(obs) & 15) == 0 && wide_bf16_lds(net, rollout).bytes() <= kDeepLdsMax;
}
bool wide_bf16_supported(const mppo_net_t& net, const mppo_batch_t& b) { return wide_bf16_geometry(net, b.obs, b.obs_ld, false); }
bool wide_bf16_rollout_supported(const mppo_net_t& net, const float* obs, int obs_ld) { return wide_bf16_geometry(net, obs, obs_ld, true); }

static int32_t wide_bf16_launch(bool rollout, const mppo_net_t& net, const DeepArgs& a, int ny, hipStream_t stream) {
  const size_t smem = wide_bf16_lds(net, rollout).bytes();
  MPPO_REQUIRE(smem <= kDeepLdsMax, "wide_bf16_kernel: %zu bytes of LDS (the dispatch asks wide_bf16_supported first)", smem);
  static thread_local size_t attr_for = 0;
  if (smem > 64 * 1024 && attr_for < smem) {  // (a launch above 64 KB needs the attribute)
    for (const WideBf16Kernel& k : kWideBf16Kernels) MPPO_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k.fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    attr_for = smem;
  }
  WideBf16Fn fn = nullptr;
  for (const WideBf16Kernel& k : kWideBf16Kernels)
    if (k.rollout == rollout && k.ot == (net.A > 16 ? 2 : 1)) fn = k.fn;
  MPPO_REQUIRE(fn, "wide_bf16_kernel: no instantiation for this launch");
  hipLaunchKernelGGL(fn, dim3(cdiv(a.mb, kDeepRows), ny), dim3(2 * net.H), smem, stream, a);
  MPPO_CHECK_LAUNCH(rollout ? "wide_bf16_kernel<rollout>" : "wide_bf16_kernel");
  return MPPO_OK;
}

static DeepArgs wide_bf16_args(const mppo_net_t& net, const float* params, int n, int AP) {
  DeepArgs a{};
  const ParamLayout L = param_layout(net);
  a.mb = n; a.O = net.O; a.OP = net.OP; a.A = net.A; a.AP = AP; a.DP = AP + 4; a.H = net.H; a.nl = L.nl; a.use_tanh = net.use_tanh;
  a.params = params; a.log_std = L.log_std;
  for (int l = 0; l <= L.nl; ++l) { a.w[0][l] = L.a_w[l]; a.b[0][l] = L.a_b[l]; a.w[1][l] = L.c_w[l]; a.b[1][l] = L.c_b[l]; }
  return a;
}

// The row-local half of a minibatch step in one launch: both networks, grid (mb / 16 tiles, 2).  Results in the GradBufs, plain layout.
int32_t wide_bf16_forward_backward(const mppo_net_t& net, const float* params, const mppo_batch_t& batch, const int* idx, int mb, const float* adv_stat,
                                   float inv_count, const mppo_loss_cfg_t& lc, const GradBufs& g, hipStream_t stream) {
  DeepArgs a = wide_bf16_args(net, params, mb, g.f.AP);
  a.bt = batch; a.idx = idx; a.adv_stat = adv_stat; a.inv_count = inv_count; a.lc = lc;
  for (int l = 0; l < a.nl; ++l) { a.h[0][l] = g.f.ha[l]; a.h[1][l] = g.f.hc[l]; a.dz[0][l] = g.dza[l]; a.dz[1][l] = g.dzc[l]; }
  a.dout = g.dout; a.xmb = g.xmb; a.partial = g.partial;
  return wide_bf16_launch(false, net, a, 2, stream);
}

// Rollout policy step on n rows in one launch: hidden layers, heads, sample + log-prob, value.  noise == nullptr: critic only (the bootstrap
// value); value == nullptr: actor only.
int32_t wide_bf16_policy_forward(const mppo_net_t& net, const float* params, int n, const float* obs, int obs_ld, const float* noise, float* action,
                                 float* log_prob, float* value, float* mean_out, int AP, hipStream_t stream) {
  DeepArgs a = wide_bf16_args(net, params, n, AP);
  a.bt.obs = obs; a.bt.obs_ld = obs_ld;
  a.noise = noise; a.action = action; a.log_prob = log_prob; a.value = value; a.mean_out = mean_out;
  a.net0 = noise ? 0 : 1;
  return wide_bf16_launch(true, net, a, noise && value ? 2 : 1, stream);
}

}  // namespace mppo
