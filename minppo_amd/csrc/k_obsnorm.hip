// k_obsnorm.hip - running observation normalisation: per observation column a running mean and variance, collected from the rollout's own rows
// and applied to them in place before the network reads them.  The reference has no counterpart (train.py:157 feeds the raw observation); what
// users of PPO on humanoids know as Brax's `normalize_observations` and gym's `NormalizeObservation`.  Off by default.
//
//   obs_norm_apply_kernel   once per rollout step, on the rows the step just wrote: y = (x - mean32[c]) * inv_std32[c] in float32, clamped to
//                           [-clip, clip] where clip > 0, written over x; from the raw x, before it is overwritten, d = (double)x - (double)mean32[c] goes
//                           into S1 = sum d and S2 = sum d^2.  A workgroup of 16 waves owns 128 rows: wave w walks rows 8 w .. 8 w + 7 in row order, a lane
//                           owns four neighbouring columns (one 16-byte load and store per row, all eight loads requested before the first is consumed; a
//                           layout that does not allow it takes the one-column form); the waves' sums meet in LDS and one thread per (column, sum) adds
//                           them in wave order.  Every sum has one owner and one order - no atomics, nothing that depends on which wave arrives first -
//                           so the same inputs give the same bytes.  Columns O .. obs_ld - 1 are never written (the row pass relies on the pad words
//                           staying zero).  Why 128 rows and not fewer: the partials are what the update kernel has to read - with one wave of 16 rows
//                           per workgroup 4096 x 225 made 9.2 MB of them per update, and the one workgroup that sums them in index order took 150 us.
//   obs_norm_update_kernel  once per update, ONE workgroup, one thread per column: the partials in index order, then Chan's merge of (k rows, their mean
//                           b and sum of squared deviations M2b) into the running (n, mean, M2), then the float32 table the next update applies.
//   obs_norm_rank_sums_kernel  several ranks only, once per update in front of the gather: this rank's partials in index order into its slot of [G][2][O];
//                           the update kernel then runs on the gathered slots (n_partials = G, rows = T N G).
//
// This file is compiled without floating-point contraction (minppo_amd/build.py): the merge is a dozen float64 operations whose roundings the tests restate.
#include "obsnorm.h"

#include <cmath>

namespace mppo {

template <int V>
__global__ void __launch_bounds__(kObsNormWaves * 64) obs_norm_apply_kernel(int N, int O, float* __restrict__ obs, int obs_ld, const float* __restrict__ table, int table_ld,
                                                                            float clip, double* __restrict__ partial) {
  __shared__ double red[kObsNormWaves][2][64 * V];  // the waves' sums of the 64 V columns in flight
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row0 = (int)blockIdx.x * kObsNormRows + wave * kObsNormWaveRows;
  const int nrows = N - row0 < kObsNormWaveRows ? N - row0 : kObsNormWaveRows;  // (<= 0: this wave's rows lie beyond N and contribute nothing)
  const int units = (O + V - 1) / V;
  for (int u0 = 0; u0 < units; u0 += 64) {  // (one trip for up to 256 columns; the trip count is the same in every thread: barriers inside)
    const int u = u0 + lane, c0 = u * V;
    const bool whole = c0 + V <= O;  // (the last unit of a row may reach into the pad columns: read, never written)
    double s1[V], s2[V];
#pragma unroll
    for (int k = 0; k < V; ++k) { s1[k] = 0.0; s2[k] = 0.0; }
    if (u < units && nrows > 0) {
      float m[V], s[V];
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const bool valid = c0 + k < O;
        m[k] = valid ? table[c0 + k] : 0.f;
        s[k] = valid ? table[(size_t)table_ld + c0 + k] : 1.f;
      }
      float* const col = obs + (size_t)row0 * obs_ld + c0;
      float x[kObsNormWaveRows][V];
#pragma unroll
      for (int b = 0; b < kObsNormWaveRows; ++b) {
        if (b < nrows) {
          const float* p = col + (size_t)b * obs_ld;
          if constexpr (V == 4) {
            const float4 q = *reinterpret_cast<const float4*>(p);
            x[b][0] = q.x; x[b][1] = q.y; x[b][2] = q.z; x[b][3] = q.w;
          } else {
            x[b][0] = p[0];
          }
        }
      }
#pragma unroll
      for (int b = 0; b < kObsNormWaveRows; ++b) {
        if (b < nrows) {
          float y[V];
#pragma unroll
          for (int k = 0; k < V; ++k) {
            const double d = (double)x[b][k] - (double)m[k];
            s1[k] += d;
            s2[k] += d * d;
            float v = (x[b][k] - m[k]) * s[k];
            if (clip > 0.f) v = v > clip ? clip : (v < -clip ? -clip : v);  // (a NaN stays a NaN)
            y[k] = v;
          }
          float* p = col + (size_t)b * obs_ld;
          if constexpr (V == 4) {
            if (whole) *reinterpret_cast<float4*>(p) = make_float4(y[0], y[1], y[2], y[3]);
          }
          if (V == 1 || !whole) {
#pragma unroll
            for (int k = 0; k < V; ++k) if (c0 + k < O) p[k] = y[k];
          }
        }
      }
    }
    if (partial) {  // (the same in every thread)
#pragma unroll
      for (int k = 0; k < V; ++k) { red[wave][0][lane * V + k] = s1[k]; red[wave][1][lane * V + k] = s2[k]; }
      __syncthreads();
      // one thread per (sum, column) of this trip: the waves' sums in wave order, i.e. the rows' groups of eight in row order
      for (int i = threadIdx.x; i < 2 * 64 * V; i += kObsNormWaves * 64) {
        const int which = i / (64 * V), j = i % (64 * V), c = u0 * V + j;
        if (c < O) {
          double sum = red[0][which][j];
          for (int w = 1; w < kObsNormWaves; ++w) sum += red[w][which][j];
          partial[((size_t)blockIdx.x * 2 + which) * O + c] = sum;
        }
      }
      __syncthreads();  // (the next trip overwrites `red`)
    }
  }
}

constexpr int kObsNormUpdateThreads = 256;
__global__ void __launch_bounds__(kObsNormUpdateThreads) obs_norm_update_kernel(int O, int n_partials, long long rows, const double* __restrict__ partial, double* __restrict__ stats,
                                                                                float eps, float* __restrict__ table, int table_ld) {
  const double n = stats[0];
  __syncthreads();  // every thread has read the count before thread 0 writes the new one
  const double k = (double)rows;
  for (int c = threadIdx.x; c < table_ld; c += kObsNormUpdateThreads) {
    float mean32 = 0.f, inv32 = 1.f;  // the identity: pad columns always, every column while nothing has been counted
    if (c < O) {
      double mu = stats[1 + c], M2 = stats[1 + O + c], n1 = n;
      if (rows > 0) {
        double S1 = 0.0, S2 = 0.0;
#pragma unroll 16
        for (int p = 0; p < n_partials; ++p) {  // index order: launch-major, workgroup-minor
          S1 += partial[(size_t)p * 2 * O + c];
          S2 += partial[(size_t)p * 2 * O + O + c];
        }
        const double b = (double)table[c] + S1 / k;  // the partials hold deviations from the table's mean
        double M2b = S2 - S1 * S1 / k;
        if (M2b < 0.0) M2b = 0.0;  // (rounding only: a sum of squared deviations is not negative)
        const double delta = b - mu;
        n1 = n + k;
        mu = mu + delta * k / n1;
        M2 = M2 + M2b + delta * delta * n * k / n1;
        stats[1 + c] = mu;
        stats[1 + O + c] = M2;
      }
      if (n1 > 0.0) {
        mean32 = (float)mu;
        inv32 = (float)(1.0 / sqrt(M2 / n1 + (double)eps));
      }
    }
    table[c] = mean32;
    table[(size_t)table_ld + c] = inv32;
  }
  if (threadIdx.x == 0 && rows > 0) stats[0] = n + k;
}

// Several ranks (DESIGN.md 3.7 "Across ranks"): ONE workgroup, one thread per column, adds this rank's partials in index order - the update kernel's own
// loop, from the same +0.0 - into slot `rank` of slots [world][2][O] and writes +0.0 into every other slot.  The slots are then GATHERED (peer.h
// peer_gather_f64, or a sum all-reduce in which every foreign term is +0.0: x + 0 is exact, so the transport's order does not matter) and the update kernel
// adds them in rank order.  A sum of -0.0 is published as +0.0: under the all-reduce -0.0 + 0.0 is +0.0 anyway, and both transports carry the same bits.
// world = 1: slot 0 alone, and update(n_partials = 1) on it computes 0.0 + S = S - the bytes of the update kernel on the partials themselves.
__global__ void __launch_bounds__(kObsNormUpdateThreads) obs_norm_rank_sums_kernel(int O, int n_partials, const double* __restrict__ partial, int rank, int world,
                                                                                   double* __restrict__ slots) {
  for (int c = threadIdx.x; c < O; c += kObsNormUpdateThreads) {
    double S1 = 0.0, S2 = 0.0;
#pragma unroll 16
    for (int p = 0; p < n_partials; ++p) {  // index order: launch-major, workgroup-minor
      S1 += partial[(size_t)p * 2 * O + c];
      S2 += partial[(size_t)p * 2 * O + O + c];
    }
    for (int q = 0; q < world; ++q) {
      const bool mine = q == rank;
      slots[((size_t)q * 2) * O + c] = mine && S1 != 0.0 ? S1 : 0.0;  // (a NaN stays a NaN: NaN != 0)
      slots[((size_t)q * 2 + 1) * O + c] = mine && S2 != 0.0 ? S2 : 0.0;
    }
  }
}

int32_t obs_norm_rank_sums_launch(int O, int n_partials, const double* partial, int rank, int world, double* slots, hipStream_t stream) {
  hipLaunchKernelGGL(obs_norm_rank_sums_kernel, dim3(1), dim3(kObsNormUpdateThreads), 0, stream, O, n_partials, partial, rank, world, slots);
  MPPO_CHECK_LAUNCH("obs_norm_rank_sums_kernel");
  return MPPO_OK;
}

int32_t obs_norm_apply_launch(int N, int O, float* obs, int obs_ld, const float* table, int table_ld, float clip, double* partial, hipStream_t stream) {
  const dim3 grid(obs_norm_partials(N)), block(kObsNormWaves * 64);
  const bool vec = (reinterpret_cast<uintptr_t>(obs) & 15) == 0 && obs_ld % 4 == 0;
  if (vec)
    hipLaunchKernelGGL(obs_norm_apply_kernel<4>, grid, block, 0, stream, N, O, obs, obs_ld, table, table_ld, clip, partial);
  else
    hipLaunchKernelGGL(obs_norm_apply_kernel<1>, grid, block, 0, stream, N, O, obs, obs_ld, table, table_ld, clip, partial);
  MPPO_CHECK_LAUNCH("obs_norm_apply_kernel");
  return MPPO_OK;
}

int32_t obs_norm_update_launch(int O, int n_partials, long long rows, const double* partial, double* stats, float eps, float* table, int table_ld, hipStream_t stream) {
  hipLaunchKernelGGL(obs_norm_update_kernel, dim3(1), dim3(kObsNormUpdateThreads), 0, stream, O, n_partials, rows, partial, stats, eps, table, table_ld);
  MPPO_CHECK_LAUNCH("obs_norm_update_kernel");
  return MPPO_OK;
}

}  // namespace mppo

using namespace mppo;

extern "C" int32_t mppo_obs_norm_partials(int32_t N) { return N >= 1 ? obs_norm_partials(N) : 0; }

extern "C" int32_t mppo_obs_norm_apply(int32_t N, int32_t O, float* obs, int32_t obs_ld, const float* table, int32_t table_ld, float clip, double* partial, void* stream) {
  MPPO_REQUIRE(N >= 1 && O >= 1, "mppo_obs_norm_apply: N = %d rows, O = %d columns", N, O);
  MPPO_REQUIRE(obs && table, "mppo_obs_norm_apply: null observations / table");
  MPPO_REQUIRE(obs_ld >= O && table_ld >= O, "mppo_obs_norm_apply: obs_ld %d / table_ld %d below O = %d", obs_ld, table_ld, O);
  MPPO_REQUIRE(clip >= 0.f, "mppo_obs_norm_apply: clip %g is negative (or not a number)", (double)clip);
  MPPO_REQUIRE((reinterpret_cast<uintptr_t>(obs) & 3) == 0 && (reinterpret_cast<uintptr_t>(table) & 3) == 0 && (reinterpret_cast<uintptr_t>(partial) & 7) == 0,
               "mppo_obs_norm_apply: observations / table must be 4-byte aligned, the partials 8-byte aligned");
  return obs_norm_apply_launch(N, O, obs, obs_ld, table, table_ld, clip, partial, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mppo_obs_norm_rank_sums(int32_t O, int32_t n_partials, const double* partial, int32_t rank, int32_t world, double* slots, void* stream) {
  MPPO_REQUIRE(O >= 1 && n_partials >= 1, "mppo_obs_norm_rank_sums: O = %d, %d partials", O, n_partials);
  MPPO_REQUIRE(world >= 1 && rank >= 0 && rank < world, "mppo_obs_norm_rank_sums: rank %d of %d", rank, world);
  MPPO_REQUIRE(partial && slots, "mppo_obs_norm_rank_sums: null partials / slots");
  MPPO_REQUIRE((reinterpret_cast<uintptr_t>(partial) & 7) == 0 && (reinterpret_cast<uintptr_t>(slots) & 7) == 0, "mppo_obs_norm_rank_sums: partials and slots must be 8-byte aligned");
  return obs_norm_rank_sums_launch(O, n_partials, partial, rank, world, slots, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mppo_obs_norm_update(int32_t O, int32_t n_partials, int64_t rows, const double* partial, double* stats, float eps, float* table, int32_t table_ld,
                                        void* stream) {
  MPPO_REQUIRE(O >= 1 && n_partials >= 0 && rows >= 0, "mppo_obs_norm_update: O = %d, %d partials, %lld rows", O, n_partials, (long long)rows);
  MPPO_REQUIRE(rows == 0 || (n_partials >= 1 && partial), "mppo_obs_norm_update: %lld rows but no partials", (long long)rows);
  MPPO_REQUIRE(stats && table && table_ld >= O, "mppo_obs_norm_update: null statistics / table, or table_ld %d below O = %d", table_ld, O);
  MPPO_REQUIRE(eps >= 0.f, "mppo_obs_norm_update: eps %g is negative (or not a number)", (double)eps);
  MPPO_REQUIRE((reinterpret_cast<uintptr_t>(stats) & 7) == 0 && (reinterpret_cast<uintptr_t>(partial) & 7) == 0, "mppo_obs_norm_update: statistics and partials must be 8-byte aligned");
  return obs_norm_update_launch(O, n_partials, (long long)rows, partial, stats, eps, table, table_ld, static_cast<hipStream_t>(stream));
}
