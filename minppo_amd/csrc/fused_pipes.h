// fused_pipes.h — the weight streams of fused_mlp_kernel (k_fused.hip): range-checked buffer loads through a branch-free three-deep
// register ring.  GemmPipe streams a float weight (forward [K][H] or transposed [H][K]); FragPipe streams the bf16 fragment-order
// shadow copy of one.  Both have the same interface: prefetch() requests the first two stages (one phase early), run() multiplies a
// 16-row LDS tile into the wave's two 16-column accumulators; GemmPipe::run2() does that for the two halves of a 32-row tile.
#pragma once
#include "fused_common.h"

namespace mppo {

// One 16-row x 32-column slab of A_tile . op(W) on the 16x16x4 f32 MFMA (A_tile in LDS with row stride AS, K a multiple
// of 32, zero beyond Kvalid).  The wave's 32 columns are two INTERLEAVED 16-column tiles: tile tau holds columns
// n0 + 2j + tau (j = lane&15), so that one float2 load feeds both tiles.
//   NT = false: W stored [K][H] (forward):   lane (j, kq) loads W[k][n0+2j .. +1] for its 8 k's of the stage
//   NT = true : W stored [H][K] (backward):  B(k,n) = W[n*K + k], lane loads float4 W[n][k..k+3] for both of its columns
// Stage = 32 k = 16 MFMAs; stage S+1's B fragment is fetched while stage S computes (copy-free ping-pong), so with two
// waves per SIMD a load has about 1000 cycles before its first use.  k inside a stage: 32S + 16g + 4kq + c.
// Loads are BRANCH-FREE on purpose: a conditional around a prefetch splits the loop body into basic blocks, and the
// compiler's s_waitcnt insertion then has to assume the shorter of the two histories at the join - it waited for vmcnt(0)
// before a stage whose operands had been requested two stages earlier, i.e. the ring degenerated to depth one.
template <bool NT>
struct BStage {
  float x0[8], x1[8];
  // NT = false: `wb` is a range-checked view of W[0 .. Kvalid) x H: rows of the zero-padded K tail read as 0
  __device__ __forceinline__ void load(const float* W, const BufView& wb, int H, int K, int S, int n0, int j, int kq) {
    if (NT) {
      // buffer loads like the forward pipe: the per-lane part of the address is fixed for the whole GEMM, the stage advances a
      // scalar offset (flat loads recomputed a 64-bit address per load: VALU work in the MFMA stream)
      const int lane_off = ((n0 + 2 * j) * K + 4 * kq) * 4;
#pragma unroll
      for (int g = 0; g < 2; ++g) {
#ifdef MPPO_FUSED_NT_FLAT
        const float4 q0 = *reinterpret_cast<const float4*>(W + (size_t)(n0 + 2 * j) * K + 32 * S + 16 * g + 4 * kq);
        const float4 q1 = *reinterpret_cast<const float4*>(W + (size_t)(n0 + 2 * j + 1) * K + 32 * S + 16 * g + 4 * kq);
#else
        const float4 q0 = buf_load_f4(wb, lane_off, (32 * S + 16 * g) * 4);
        const float4 q1 = buf_load_f4(wb, lane_off + K * 4, (32 * S + 16 * g) * 4);
#endif
        x0[4 * g] = q0.x; x0[4 * g + 1] = q0.y; x0[4 * g + 2] = q0.z; x0[4 * g + 3] = q0.w;
        x1[4 * g] = q1.x; x1[4 * g + 1] = q1.y; x1[4 * g + 2] = q1.z; x1[4 * g + 3] = q1.w;
      }
    } else {
      const int lane_off = (4 * kq * H + n0 + 2 * j) * 4;  // bytes; the only per-lane part of the address
#pragma unroll
      for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float2 q = buf_load_f2(wb, lane_off, (32 * S + 16 * g + c) * H * 4);
          x0[4 * g + c] = q.x; x1[4 * g + c] = q.y;
        }
    }
  }
};

// BF16: a lane's four consecutive k's (the float4 it already holds) are one operand of v_mfma_f32_16x16x16_bf16: the same
// registers, rounded to bf16, feed 4 MFMAs instead of 16 (f32 accumulate).
template <bool BF16>
__device__ __forceinline__ void stage_mfma(const float* arow, int S, const float (&x0)[8], const float (&x1)[8], f32x4& acc0, f32x4& acc1) {
  const float4 a0 = *reinterpret_cast<const float4*>(arow + 32 * S);
  const float4 a1 = *reinterpret_cast<const float4*>(arow + 32 * S + 16);
  if (BF16) {
    const bf16x4 A0 = pack_bf16x4(a0.x, a0.y, a0.z, a0.w), A1 = pack_bf16x4(a1.x, a1.y, a1.z, a1.w);
    mfma_bf16_16x16x16(A0, pack_bf16x4(x0[0], x0[1], x0[2], x0[3]), acc0);
    mfma_bf16_16x16x16(A0, pack_bf16x4(x1[0], x1[1], x1[2], x1[3]), acc1);
    mfma_bf16_16x16x16(A1, pack_bf16x4(x0[4], x0[5], x0[6], x0[7]), acc0);
    mfma_bf16_16x16x16(A1, pack_bf16x4(x1[4], x1[5], x1[6], x1[7]), acc1);
    return;
  }
  mfma_f32_16x16x4(a0.x, x0[0], acc0); mfma_f32_16x16x4(a0.x, x1[0], acc1);
  mfma_f32_16x16x4(a0.y, x0[1], acc0); mfma_f32_16x16x4(a0.y, x1[1], acc1);
  mfma_f32_16x16x4(a0.z, x0[2], acc0); mfma_f32_16x16x4(a0.z, x1[2], acc1);
  mfma_f32_16x16x4(a0.w, x0[3], acc0); mfma_f32_16x16x4(a0.w, x1[3], acc1);
  mfma_f32_16x16x4(a1.x, x0[4], acc0); mfma_f32_16x16x4(a1.x, x1[4], acc1);
  mfma_f32_16x16x4(a1.y, x0[5], acc0); mfma_f32_16x16x4(a1.y, x1[5], acc1);
  mfma_f32_16x16x4(a1.z, x0[6], acc0); mfma_f32_16x16x4(a1.z, x1[6], acc1);
  mfma_f32_16x16x4(a1.w, x0[7], acc0); mfma_f32_16x16x4(a1.w, x1[7], acc1);
}

// Three-deep register ring over the K stages: stage S+2 is fetched while stage S computes, so a weight fragment has two
// full MFMA blocks (about 2000 cycles with two waves per SIMD) to arrive from L2.  The first two stages are requested by
// prefetch(), which the kernel calls one phase EARLY (weights depend on nothing computed here): the fill latency of each
// GEMM phase hides under the barrier / epilogue / loss code of the phase before it.
template <bool NT>
struct GemmPipe {
  BStage<NT> b0, b1;
  BufView wb;
  __device__ __forceinline__ void prefetch(int K, int Kvalid, const float* W, int H, int n0, int lane) {
    const int j = lane & 15, kq = lane >> 4;
    const int last = K / 32 - 1;
    wb = make_buf(W, (unsigned)Kvalid * (unsigned)H * 4u);
    b0.load(W, wb, H, K, 0, n0, j, kq);
    b1.load(W, wb, H, K, last < 1 ? last : 1, n0, j, kq);
  }
  // invariant at the loop top: b0 = stage S, b1 = stage S+1.  Stage indices past the end are clamped to the last stage
  // (a redundant, harmless load) instead of being skipped: straight-line code, exact vmcnt bookkeeping.
  template <bool BF16>
  __device__ __forceinline__ void run(const float* At, int AS, int K, const float* W, int H, int n0, int lane, f32x4& acc0, f32x4& acc1) {
    const int j = lane & 15, kq = lane >> 4;
    const float* arow = At + j * AS + 4 * kq;
    const int nst = K / 32, last = nst - 1;
    BStage<NT> b2;
    int S = 0;
    // MPPO_SCHED_FENCE: the machine scheduler otherwise sinks a stage's loads down to their first use (it minimises
    // register pressure), which is exactly the latency exposure the ring exists to avoid
    for (; S + 2 < nst; S += 3) {
      b2.load(W, wb, H, K, S + 2, n0, j, kq);
      MPPO_SCHED_FENCE();
      stage_mfma<BF16>(arow, S, b0.x0, b0.x1, acc0, acc1);
      MPPO_SCHED_FENCE();
      b0.load(W, wb, H, K, S + 3 < last ? S + 3 : last, n0, j, kq);
      MPPO_SCHED_FENCE();
      stage_mfma<BF16>(arow, S + 1, b1.x0, b1.x1, acc0, acc1);
      MPPO_SCHED_FENCE();
      b1.load(W, wb, H, K, S + 4 < last ? S + 4 : last, n0, j, kq);
      MPPO_SCHED_FENCE();
      stage_mfma<BF16>(arow, S + 2, b2.x0, b2.x1, acc0, acc1);
      MPPO_SCHED_FENCE();
    }
    if (S < nst) stage_mfma<BF16>(arow, S, b0.x0, b0.x1, acc0, acc1);
    if (S + 1 < nst) stage_mfma<BF16>(arow, S + 1, b1.x0, b1.x1, acc0, acc1);
  }
  // Two 16-row tiles per workgroup (RT = 2: rows j and j + 16 of a 32-row activation tile): every weight stage is fetched ONCE and
  // multiplied into both tiles - twice the MFMAs per byte streamed, the same ring otherwise.
  __device__ __forceinline__ void run2(const float* At, int AS, int K, const float* W, int H, int n0, int lane, f32x4 (&acc)[2][2]) {
    const int j = lane & 15, kq = lane >> 4;
    const float* arow = At + j * AS + 4 * kq;
    const float* arow2 = arow + 16 * AS;
    const int nst = K / 32, last = nst - 1;
    BStage<NT> b2;
    int S = 0;
    for (; S + 2 < nst; S += 3) {
      b2.load(W, wb, H, K, S + 2, n0, j, kq);
      MPPO_SCHED_FENCE();
      stage_mfma<false>(arow, S, b0.x0, b0.x1, acc[0][0], acc[0][1]);
      stage_mfma<false>(arow2, S, b0.x0, b0.x1, acc[1][0], acc[1][1]);
      MPPO_SCHED_FENCE();
      b0.load(W, wb, H, K, S + 3 < last ? S + 3 : last, n0, j, kq);
      MPPO_SCHED_FENCE();
      stage_mfma<false>(arow, S + 1, b1.x0, b1.x1, acc[0][0], acc[0][1]);
      stage_mfma<false>(arow2, S + 1, b1.x0, b1.x1, acc[1][0], acc[1][1]);
      MPPO_SCHED_FENCE();
      b1.load(W, wb, H, K, S + 4 < last ? S + 4 : last, n0, j, kq);
      MPPO_SCHED_FENCE();
      stage_mfma<false>(arow, S + 2, b2.x0, b2.x1, acc[0][0], acc[0][1]);
      stage_mfma<false>(arow2, S + 2, b2.x0, b2.x1, acc[1][0], acc[1][1]);
      MPPO_SCHED_FENCE();
    }
    if (S < nst) { stage_mfma<false>(arow, S, b0.x0, b0.x1, acc[0][0], acc[0][1]); stage_mfma<false>(arow2, S, b0.x0, b0.x1, acc[1][0], acc[1][1]); }
    if (S + 1 < nst) { stage_mfma<false>(arow, S + 1, b1.x0, b1.x1, acc[0][0], acc[0][1]); stage_mfma<false>(arow2, S + 1, b1.x0, b1.x1, acc[1][0], acc[1][1]); }
  }
};

// The same ring for a bf16 network with shadow copies: the B operand comes from the fragment-order bf16 copy of the weight
// (ppo_layout.h frag_index): a lane's eight values of a column tile and stage are 16 contiguous bytes (two 16-byte buffer loads instead of eight
// 8-byte ones, half the bytes, and no float -> bf16 conversion of weights in the loop).  `W` = fragment base of the matrix.
struct FragStage {
  float4 q0, q1;  // raw bits: q0 = tile 0 (k 0..3 of group 0 | group 1), q1 = tile 1
  __device__ __forceinline__ void load(const BufView& wb, int S, int nwaves, int wave, int lane) {
    const int uni = ((S * nwaves + wave_uniform(wave)) * 64) * 32;  // bytes: (stage, wave slab) block of 2 KB; the wave index in a scalar register (else: a waterfall loop around every load)
    q0 = buf_load_f4(wb, lane * (2 * kFragLaneElems), uni);
    q1 = buf_load_f4(wb, lane * (2 * kFragLaneElems) + 2 * kFragTileElems, uni);
  }
};
__device__ __forceinline__ void frag_mfma(const float* arow, int S, const FragStage& b, f32x4& acc0, f32x4& acc1) {
  const float4 a0 = *reinterpret_cast<const float4*>(arow + 32 * S);
  const float4 a1 = *reinterpret_cast<const float4*>(arow + 32 * S + 16);
  const bf16x4 A0 = pack_bf16x4(a0.x, a0.y, a0.z, a0.w), A1 = pack_bf16x4(a1.x, a1.y, a1.z, a1.w);
  const bf16x4 t0g0 = bf16x4_from_bits(b.q0.x, b.q0.y), t0g1 = bf16x4_from_bits(b.q0.z, b.q0.w);
  const bf16x4 t1g0 = bf16x4_from_bits(b.q1.x, b.q1.y), t1g1 = bf16x4_from_bits(b.q1.z, b.q1.w);
  mfma_bf16_16x16x16(A0, t0g0, acc0);
  mfma_bf16_16x16x16(A0, t1g0, acc1);
  mfma_bf16_16x16x16(A1, t0g1, acc0);
  mfma_bf16_16x16x16(A1, t1g1, acc1);
}
struct FragPipe {
  FragStage b0, b1;
  BufView wb;
  int nw;
  // same interface as GemmPipe (K = padded depth, H = columns, n0 = 32 * wave); Kvalid is implicit (the copy is zero-padded)
  __device__ __forceinline__ void prefetch(int K, int, const float* W, int H, int n0, int lane) {
    const int last = K / 32 - 1;
    nw = H / 32;
    wb = make_buf(W, (unsigned)K * (unsigned)H * 2u);
    b0.load(wb, 0, nw, n0 >> 5, lane);
    b1.load(wb, last < 1 ? last : 1, nw, n0 >> 5, lane);
  }
  template <bool BF16>
  __device__ __forceinline__ void run(const float* At, int AS, int K, const float*, int, int n0, int lane, f32x4& acc0, f32x4& acc1) {
    const int j = lane & 15, kq = lane >> 4, wv = n0 >> 5;
    const float* arow = At + j * AS + 4 * kq;
    const int nst = K / 32, last = nst - 1;
    FragStage b2;
    int S = 0;
    for (; S + 2 < nst; S += 3) {
      b2.load(wb, S + 2, nw, wv, lane);
      MPPO_SCHED_FENCE();
      frag_mfma(arow, S, b0, acc0, acc1);
      MPPO_SCHED_FENCE();
      b0.load(wb, S + 3 < last ? S + 3 : last, nw, wv, lane);
      MPPO_SCHED_FENCE();
      frag_mfma(arow, S + 1, b1, acc0, acc1);
      MPPO_SCHED_FENCE();
      b1.load(wb, S + 4 < last ? S + 4 : last, nw, wv, lane);
      MPPO_SCHED_FENCE();
      frag_mfma(arow, S + 2, b2, acc0, acc1);
      MPPO_SCHED_FENCE();
    }
    if (S < nst) frag_mfma(arow, S, b0, acc0, acc1);
    if (S + 1 < nst) frag_mfma(arow, S + 1, b1, acc0, acc1);
  }
};
template <bool FRAG, bool NT> struct PipeSel { typedef GemmPipe<NT> type; };
template <bool NT> struct PipeSel<true, NT> { typedef FragPipe type; };

}  // namespace mppo
