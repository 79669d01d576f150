// k_deep.hip — the row-local half of a minibatch step, and the rollout policy step, for networks of 1 to 4 hidden layers in ONE launch:
//   x -> h_0 -> ... -> h_{L-1} -> output layer -> clipped-PPO loss terms -> d(loss)/d(outputs) -> dZ_{L-1} -> ... -> dZ_0
// (reference minppo/train.py:56-68 `MLP([hidden_size] * num_layers + [out])`, :222-243 the loss, :157-160,182 the rollout).  Two hidden layers are
// fused_mlp_kernel's (k_fused.hip, tried first by the dispatch in k_ppo.hip) and come here only where that kernel refuses them (an observation
// wider than its weight-gradient tile table, a weight offset off a 16-byte boundary); without this kernel a depth takes 2L layer-wise launches
// per optimizer step and L + 1 per rollout step, every activation going to HBM and back between them.
//
// Work split: one workgroup = 16 rows (training: gathered by permutation index) of ONE network (blockIdx.y: 0 actor, 1 critic), H/32 waves; wave w
// owns hidden columns [32w, 32w + 32) of every layer as two interleaved 16 x 16 tiles of v_mfma_f32_16x16x4_f32 - exact f32 products.
// Data movement: the row tile stays in LDS from x to dZ_0 (DeepLds, deep.h).  Weights stream L2 -> registers through the three-deep ring of
// fused_pipes.h: ONE forward ring walks the layers (its next layer's first two stages are requested before the epilogue and barrier of the
// current one), ONE backward ring reads W_{l+1} as stored ([H][H] rows = inputs: GemmPipe<true>, float4 along the contraction), no shadow copies.
// The output layer's weights sit in registers: the head GEMM splits K = H over the waves and sums the partial tiles through LDS.
// Training keeps every h_l in LDS for act'(h_l); the dZ tiles ping-pong between the dead x tile and one more tile.  The rollout role keeps two
// ping-pong tiles only, so that two workgroups fit a CU.
// Outputs (training): the layer-wise path's buffers in plain row-major layout - h_l and dZ_l [mb][H], dOut [mb][AP + 4], the gathered rows
// [mb][OP], one row of loss partials per 16-row tile - consumed unchanged by the layer-wise weight-gradient GEMMs and grad_reduce_kernel.
// Only rows below mb are stored: a last partial tile stays inside the workspace.
// XSTREAM (the resident x tile would not fit a CU's LDS: wide robots): the x tile is never resident.  Layer 0 consumes the observation in slabs of
// kDeepSlab = 96 columns through a ring of two LDS slabs.  A thread resolves the rows of its float4 pieces once; per slab it requests the pieces of
// slab s + 1 from memory, multiplies slab s (one turn of the weight ring: GemmPipe::run_part, the ring walks on across the slab boundaries), stores
// the pieces into the other half of the ring (and, the actor workgroup, into xmb) and meets ONE barrier: the half it stores to was last read before the
// previous slab's barrier, and is read after this one.  Same stages, same order, one accumulation: the bits of the resident form.  Behind layer 0
// the two forms are the same code.
#include "deep.h"
#include "fused_common.h"
#include "fused_pipes.h"

namespace mppo {

template <bool ROLLOUT, int OT, int XQ>  // XQ: 0 = resident x tile; streamed: float4 pieces of a slab per thread (kDeepSlabChunks <= XQ blockDim.x)
__global__ void __launch_bounds__(512, ROLLOUT ? MPPO_ROLLOUT_WAVES : MPPO_TRAIN_WAVES) deep_mlp_kernel(DeepArgs a) {
  constexpr bool XSTREAM = XQ > 0;
  constexpr int NQ = XSTREAM ? XQ : 1;
  constexpr int SD = 16 * OT;  // row stride of the per-row output-space tiles
  MPPO_DYN_SMEM(smem_raw);
  float* sm = reinterpret_cast<float*>(smem_raw);
  const int H = a.H, O = a.O, OP = a.OP, A = a.A, AP = a.AP, L = a.nl;
  const int net = blockIdx.y + (ROLLOUT ? a.net0 : 0);  // 0 actor, 1 critic
  const DeepLds lds(O, H, OT, L, ROLLOUT, XSTREAM);      // the layout the host sized the launch from
  const int KP = lds.KP, XS = lds.XS, HS = lds.HS;
  float* xt = lds.xt(sm);
  const int t = threadIdx.x, nthr = blockDim.x, lane = t & 63, wave = t >> 6;
  const int row0 = blockIdx.x * kDeepRows;
  const bool tanh_act = net == 0 && a.use_tanh;
  const int nout = net ? 1 : A;
  const int n0 = 32 * wave, cj = lane & 15, rq = lane >> 4, c0 = n0 + 2 * cj;

  // ---- requested now, consumed phases later (nothing here depends on anything computed in this kernel): the first two weight stages of
  // layer 0, the output layer's weights and biases, the per-row scalars of the loss ----
  GemmPipe<false> fwd;
  fwd.prefetch(KP, O, a.params + a.w[net][0], H, n0, lane);
  const float* W3 = a.params + a.w[net][L];
  const float* B3 = a.params + a.b[net][L];
  const float adv_mean = ROLLOUT ? 0.f : a.adv_stat[0], adv_rstd = ROLLOUT ? 1.f : a.adv_stat[1];
  float ls[OT], b3v[OT];  // output o = cj + 16 ot of this lane
#pragma unroll
  for (int ot = 0; ot < OT; ++ot) {
    const int o = cj + 16 * ot;
    ls[ot] = (net == 0 && o < A) ? a.params[a.log_std + o] : 0.f;
    b3v[ot] = o < nout ? B3[o] : 0.f;
  }
  // w3p: B operands of the head GEMM (k = 32 wave + 16 g + 4 rq + c, output o); w3q: B operands of dZ_{L-1} = dOut . W_out^T (hidden
  // columns c0, c0 + 1; contracted output 4 m + rq)
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
  // ---- the index -> row chain: every index this thread needs first and together, then what they point at (clamped addresses, masked uses) ----
  const int kp4 = KP / 4, nx = kDeepRows * kp4;  // float4 chunks of the x tile
  const bool gather = !ROLLOUT && a.idx;
  auto chunk_row = [&](int e) {
    const int gi = row0 + e / kp4 < a.mb ? row0 + e / kp4 : a.mb - 1;
    return gather ? (long)a.idx[gi] : (long)gi;
  };
  const int e0 = t, e1 = t + nthr < nx ? t + nthr : t;  // (this thread's first two chunks; a wide workgroup on a narrow observation has threads without one)
  const long xrow0 = XSTREAM ? 0 : chunk_row(e0), xrow1 = XSTREAM ? 0 : chunk_row(e1);
  // streamed: piece q of this thread is float4 e = t + q nthr of EVERY slab - row e / 24 of the tile, columns 4 (e % 24) .. + 3 of the slab - so
  // its row is resolved here, once (xsrc: that row at the piece's column of slab 0)
  const float* xsrc[NQ];
  if (XSTREAM) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int e = t + q * nthr, r = e / (kDeepSlab / 4);
      const int gi = row0 + r < a.mb ? row0 + r : a.mb - 1;  // (e past the slab: a clamped row, never loaded)
      xsrc[q] = a.bt.obs + (gather ? (long)a.idx[gi] : (long)gi) * a.bt.obs_ld + 4 * (e % (kDeepSlab / 4));
    }
  }
  long prow[4];
  bool pon[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = row0 + 4 * rq + r;
    pon[r] = i < a.mb;
    const int ic = pon[r] ? i : a.mb - 1;
    prow[r] = gather ? (long)a.idx[ic] : (long)ic;
  }
  auto load_chunk = [&](int e, long row) {
    const int c = (e % kp4) * 4;
    return c < OP ? *reinterpret_cast<const float4*>(a.bt.obs + row * a.bt.obs_ld + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  // (the K tail of the first layer, columns OP .. KP - 1, is zero in LDS; the weight view returns zeros for its rows as well)
  auto put_chunk = [&](int e, const float4& q) {
    const int r = e / kp4, c = (e % kp4) * 4;
    *reinterpret_cast<float4*>(xt + r * XS + c) = q;
    // the gathered rows, [mb][OP], for the first layer's weight gradient (the actor workgroup writes them)
    if (!ROLLOUT && net == 0 && row0 + r < a.mb && c < OP) stream_store(a.xmb + (size_t)(row0 + r) * OP + c, q);
  };
  // streamed: the pieces of slab s -> registers (zeros from column OP on: the K tail, and every piece of a slab past the last) ...
  float4 xq[NQ];
  auto load_slab = [&](int s) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int e = t + q * nthr, c = s * kDeepSlab + 4 * (e % (kDeepSlab / 4));
      xq[q] = (e < kDeepSlabChunks && c < OP) ? *reinterpret_cast<const float4*>(xsrc[q] + s * kDeepSlab) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  // ... and from there into its half of the ring, and the gathered rows [mb][OP]
  auto put_slab = [&](int s) {
    float* sl = lds.slab(sm, s);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int e = t + q * nthr, r = e / (kDeepSlab / 4), cs = 4 * (e % (kDeepSlab / 4)), c = s * kDeepSlab + cs;
      if (e < kDeepSlabChunks) {
        *reinterpret_cast<float4*>(sl + r * XS + cs) = xq[q];
        if (!ROLLOUT && net == 0 && row0 + r < a.mb && c < OP) stream_store(a.xmb + (size_t)(row0 + r) * OP + c, xq[q]);
      }
    }
  };
  float4 xq0, xq1;
  if (XSTREAM) load_slab(0);
  else { xq0 = load_chunk(e0, xrow0); xq1 = load_chunk(e1, xrow1); }
  // actor: action[o], old log_prob, advantage | critic: old value, target | rollout: noise[o].  Raw loads on clamped addresses; every use is masked.
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
  // ---- P0: observation rows -> LDS (streamed: the first slab) ----
  if (XSTREAM) put_slab(0);
  else {
    if (e0 < nx) put_chunk(e0, xq0);
    if (t + nthr < nx) put_chunk(e1, xq1);
    for (int e = t + 2 * nthr; e < nx; e += nthr) put_chunk(e, load_chunk(e, chunk_row(e)));  // (narrow networks: more than two chunks per thread)
  }
  __syncthreads();

  // ---- forward: layer l multiplies tile `in` by W_l into the wave's 16 x 32 slab, bias + activation -> tile `out` (and, training, h_l in memory) ----
  GemmPipe<true> bwd;
  const float* in = xt;
  int in_stride = XS, K = KP;
  for (int l = 0; l < L; ++l) {
    const float2 bz = *reinterpret_cast<const float2*>(a.params + a.b[net][l] + c0);
    f32x4 acc0, acc1;
    for (int r = 0; r < 4; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    // rollout: four waves per SIMD hide the fill latency, and the 128-VGPR budget has no room for a ring that lives across the epilogue
    if (ROLLOUT && l > 0) fwd.prefetch(H, H, a.params + a.w[net][l], H, n0, lane);
    if (XSTREAM && l == 0) {
      const int nst = KP / 32, nslab = (nst + 2) / 3;
      for (int s = 0; s < nslab; ++s) {
        load_slab(s + 1);  // (past the last slab: no piece is below OP, nothing is loaded)
        fwd.template run_part<false>(lds.slab(sm, s), XS, 3 * s, nst - 3 * s < 3 ? nst - 3 * s : 3, KP, a.params + a.w[net][0], H, n0, lane, acc0, acc1);
        if (s + 1 < nslab) {  // (uniform)
          put_slab(s + 1);
          __syncthreads();
        }
      }
    } else {
      fwd.template run<false>(in, in_stride, K, a.params + a.w[net][l], H, n0, lane, acc0, acc1);
    }
    if (!ROLLOUT) {  // the next GEMM's first two stages arrive under this layer's epilogue and barrier (the last layer: under heads and loss)
      if (l + 1 < L) fwd.prefetch(H, H, a.params + a.w[net][l + 1], H, n0, lane);
      else if (L > 1) bwd.prefetch(H, H, a.params + a.w[net][L - 1], H, n0, lane);
    }
    float* out = ROLLOUT ? lds.tile(sm, l + 1) : lds.h(sm, l);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = 4 * rq + r;
      float v0 = acc0[r] + bz.x, v1 = acc1[r] + bz.y;
      if (tanh_act) { v0 = fused_tanh(v0); v1 = fused_tanh(v1); } else { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); }
      *reinterpret_cast<float2*>(out + rr * HS + c0) = make_float2(v0, v1);
      if (!ROLLOUT && row0 + rr < a.mb) stream_store(a.h[net][l] + (size_t)(row0 + rr) * H + c0, make_float2(v0, v1));
    }
    __syncthreads();
    in = out; in_stride = HS; K = H;
  }
  const float* hl = in;  // h_{L-1}

  // ---- output layer on the matrix cores: OT 16 x 16 tiles (rows x outputs), K = H split over the waves, partial tiles summed through LDS ----
  float* s_hp = lds.s_hp(sm, L - 1);  // (rollout: the tile layer L - 1 read, dead since its barrier)
  {
    f32x4 hp[OT];
#pragma unroll
    for (int ot = 0; ot < OT; ++ot)
      for (int r = 0; r < 4; ++r) hp[ot][r] = 0.f;
    const float* arow = hl + cj * HS + 4 * rq + n0;
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
    // pi.sample + pi.log_prob (train.py:158-160) / value (train.py:157,182): the arithmetic of head_kernel<., false> and fused_mlp_kernel
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
  // ---- loss terms and d loss / d outputs (train.py:223-243; the arithmetic of fused_mlp_kernel) ----
  float *s_do = lds.s_do(sm), *s_red = lds.s_red(sm), *s_l = lds.s_l(sm);
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
          if (on && o < AP) a.dout[(size_t)i * a.DP + o] = dm;  // d mean in columns [0, A), zeros up to AP
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
        if (on && cj < 4) a.dout[(size_t)i * a.DP + AP + cj] = cj == 0 ? dv : 0.f;  // d value in column AP, zeros in AP + 1 .. AP + 3
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
  // ---- dZ_{L-1} = (dOut . W_out^T) * act'(h_{L-1}) on the matrix cores (K = outputs padded to 16 OT) -> its dZ tile + memory ----
  {
    f32x4 d0, d1;
    for (int r = 0; r < 4; ++r) { d0[r] = 0.f; d1[r] = 0.f; }
#pragma unroll
    for (int m = 0; m < 4 * OT; ++m) {
      const float av = s_do[cj * SD + 4 * m + rq];
      mfma_f32_16x16x4(av, w3q[m][0], d0); mfma_f32_16x16x4(av, w3q[m][1], d1);
    }
    float* dzt = lds.dz(sm, L - 1);  // (D0: the x tile, dead since layer 0's barrier; D1: s_hp, dead since the barrier above)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = 4 * rq + r;
      const float2 hv = *reinterpret_cast<const float2*>(hl + rr * HS + c0);
      const float z0 = tanh_act ? d0[r] * (1.f - hv.x * hv.x) : (hv.x > 0.f ? d0[r] : 0.f);
      const float z1 = tanh_act ? d1[r] * (1.f - hv.y * hv.y) : (hv.y > 0.f ? d1[r] : 0.f);
      *reinterpret_cast<float2*>(dzt + rr * HS + c0) = make_float2(z0, z1);
      if (row0 + rr < a.mb) stream_store(a.dz[net][L - 1] + (size_t)(row0 + rr) * H + c0, make_float2(z0, z1));
    }
  }
  // ---- dZ_l = (dZ_{l+1} . W_{l+1}^T) * act'(h_l), l = L - 2 .. 0: reads D((l + 1) & 1), writes D(l & 1) ----
  for (int l = L - 2; l >= 0; --l) {
    __syncthreads();
    f32x4 acc0, acc1;
    for (int r = 0; r < 4; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    bwd.template run<false>(lds.dz(sm, l + 1), HS, H, a.params + a.w[net][l + 1], H, n0, lane, acc0, acc1);
    if (l > 0) bwd.prefetch(H, H, a.params + a.w[net][l], H, n0, lane);
    const float* hcur = lds.h(sm, l);
    float* dzt = lds.dz(sm, l);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = 4 * rq + r;
      const float2 hv = *reinterpret_cast<const float2*>(hcur + rr * HS + c0);
      const float z0 = tanh_act ? acc0[r] * (1.f - hv.x * hv.x) : (hv.x > 0.f ? acc0[r] : 0.f);
      const float z1 = tanh_act ? acc1[r] * (1.f - hv.y * hv.y) : (hv.y > 0.f ? acc1[r] : 0.f);
      if (l > 0) *reinterpret_cast<float2*>(dzt + rr * HS + c0) = make_float2(z0, z1);
      if (row0 + rr < a.mb) stream_store(a.dz[net][l] + (size_t)(row0 + rr) * H + c0, make_float2(z0, z1));
    }
  }
}

// ---- every instantiation the library launches; the dynamic-LDS attribute is set on exactly these ----
using DeepKernelFn = void (*)(DeepArgs);
struct DeepKernel { bool rollout; int ot, xq; DeepKernelFn fn; };
#define MPPO_DEEP_FORMS(XQ) {false, 1, XQ, deep_mlp_kernel<false, 1, XQ>}, {false, 2, XQ, deep_mlp_kernel<false, 2, XQ>}, \
                            {true, 1, XQ, deep_mlp_kernel<true, 1, XQ>}, {true, 2, XQ, deep_mlp_kernel<true, 2, XQ>}
// (streamed: as many pieces per thread as the workgroup needs for the 384 of a slab and no more - 1 from six waves on (H >= 192, the wide robots'
// networks), 2 from three, 3 at two waves, kDeepSlabQ = 6 at one: a form sized for one wave would carry staging registers that a wider workgroup never fills)
static const DeepKernel kDeepKernels[] = {MPPO_DEEP_FORMS(0), MPPO_DEEP_FORMS(1), MPPO_DEEP_FORMS(2), MPPO_DEEP_FORMS(3), MPPO_DEEP_FORMS(kDeepSlabQ)};

// The resident layout wherever it fits a CU's LDS (every geometry keeps the form it has had), the streamed one beyond
static bool deep_streamed(const mppo_net_t& net, bool rollout) {
  return DeepLds(net.O, net.H, net.A > 16 ? 2 : 1, net_layers(net), rollout, false).bytes() > kDeepLdsMax;
}
static int deep_pieces(const mppo_net_t& net, bool rollout) { return !deep_streamed(net, rollout) ? 0 : cdiv(kDeepSlabChunks, 2 * net.H) <= 3 ? cdiv(kDeepSlabChunks, 2 * net.H) : kDeepSlabQ; }
static DeepLds deep_lds(const mppo_net_t& net, bool rollout) {
  return DeepLds(net.O, net.H, net.A > 16 ? 2 : 1, net_layers(net), rollout, deep_streamed(net, rollout));
}

static bool deep_geometry(const mppo_net_t& net, const float* obs, int obs_ld, bool rollout) {
  const int L = net_layers(net);
  return L >= 1 && L <= 4 && !net.bf16 && net.H % 32 == 0 && net.H >= 32 && net.H <= 256 && net.A <= 32 && obs_ld == net.OP && (net.OP % 4) == 0 &&
         (reinterpret_cast<uintptr_t>(obs) & 15) == 0 && deep_lds(net, rollout).bytes() <= kDeepLdsMax;
}
bool deep_supported(const mppo_net_t& net, const mppo_batch_t& b) { return deep_geometry(net, b.obs, b.obs_ld, false); }
bool deep_rollout_supported(const mppo_net_t& net, const float* obs, int obs_ld) { return deep_geometry(net, obs, obs_ld, true); }

static int32_t deep_launch(bool rollout, const mppo_net_t& net, const DeepArgs& a, int ny, hipStream_t stream) {
  const size_t smem = deep_lds(net, rollout).bytes();
  MPPO_REQUIRE(smem <= kDeepLdsMax, "deep_mlp_kernel: %zu bytes of LDS (the dispatch asks deep_supported first)", smem);
  static thread_local size_t attr_for = 0;
  if (smem > 64 * 1024 && attr_for < smem) {  // (a launch above 64 KB needs the attribute)
    for (const DeepKernel& k : kDeepKernels) MPPO_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k.fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    attr_for = smem;
  }
  DeepKernelFn fn = nullptr;
  for (const DeepKernel& k : kDeepKernels)
    if (k.rollout == rollout && k.ot == (net.A > 16 ? 2 : 1) && k.xq == deep_pieces(net, rollout)) fn = k.fn;
  MPPO_REQUIRE(fn, "deep_mlp_kernel: no instantiation for this launch");
  hipLaunchKernelGGL(fn, dim3(cdiv(a.mb, kDeepRows), ny), dim3(2 * net.H), smem, stream, a);
  MPPO_CHECK_LAUNCH(rollout ? "deep_mlp_kernel<rollout>" : "deep_mlp_kernel");
  return MPPO_OK;
}

static DeepArgs deep_args(const mppo_net_t& net, const float* params, int n, int AP) {
  DeepArgs a{};
  const ParamLayout L = param_layout(net);
  a.mb = n; a.O = net.O; a.OP = net.OP; a.A = net.A; a.AP = AP; a.DP = AP + 4; a.H = net.H; a.nl = L.nl; a.use_tanh = net.use_tanh;
  a.params = params; a.log_std = L.log_std;
  for (int l = 0; l <= L.nl; ++l) { a.w[0][l] = L.a_w[l]; a.b[0][l] = L.a_b[l]; a.w[1][l] = L.c_w[l]; a.b[1][l] = L.c_b[l]; }
  return a;
}

// The row-local half of a minibatch step in one launch: both networks, grid (mb / 16 tiles, 2).  Results in the GradBufs, plain layout.
int32_t deep_forward_backward(const mppo_net_t& net, const float* params, const mppo_batch_t& batch, const int* idx, int mb, const float* adv_stat,
                              float inv_count, const mppo_loss_cfg_t& lc, const GradBufs& g, hipStream_t stream) {
  DeepArgs a = deep_args(net, params, mb, g.f.AP);
  a.bt = batch; a.idx = idx; a.adv_stat = adv_stat; a.inv_count = inv_count; a.lc = lc;
  for (int l = 0; l < a.nl; ++l) { a.h[0][l] = g.f.ha[l]; a.h[1][l] = g.f.hc[l]; a.dz[0][l] = g.dza[l]; a.dz[1][l] = g.dzc[l]; }
  a.dout = g.dout; a.xmb = g.xmb; a.partial = g.partial;
  return deep_launch(false, net, a, 2, stream);
}

// Rollout policy step on n rows in one launch: hidden layers, heads, sample + log-prob, value.  noise == nullptr: critic only (the bootstrap
// value); value == nullptr: actor only.
int32_t deep_policy_forward(const mppo_net_t& net, const float* params, int n, const float* obs, int obs_ld, const float* noise, float* action, float* log_prob,
                            float* value, float* mean_out, int AP, hipStream_t stream) {
  DeepArgs a = deep_args(net, params, n, AP);
  a.bt.obs = obs; a.bt.obs_ld = obs_ld;
  a.noise = noise; a.action = action; a.log_prob = log_prob; a.value = value; a.mean_out = mean_out;
  a.net0 = noise ? 0 : 1;
  return deep_launch(true, net, a, noise && value ? 2 : 1, stream);
}

}  // namespace mppo
