// obsnorm.h - running observation normalisation (k_obsnorm.hip), shared with the engine's rollout (engine.hip) and the evaluator (evaluator.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/minppo_hip.h"
#include "mppo_common.h"

namespace mppo {

// one apply workgroup: 16 waves of 8 rows each, a lane owns four columns; the waves' sums are added in wave order (k_obsnorm.hip).  128 rows make 32
// workgroups = 512 waves of 4096 environments, and 32 partial sums per step for the update kernel to read
constexpr int kObsNormWaves = 16, kObsNormWaveRows = 8, kObsNormRows = kObsNormWaves * kObsNormWaveRows;
inline int obs_norm_partials(int N) { return cdiv(N, kObsNormRows); }
inline size_t obs_norm_partial_doubles(int N, int O) { return (size_t)obs_norm_partials(N) * 2 * (size_t)O; }

// y = (x - mean32) * inv_std32, clamped where clip > 0, in place on obs[n, 0:O]; partial (may be null): [G][2][O] sums of d and d^2 of the raw rows
int32_t obs_norm_apply_launch(int N, int O, float* obs, int obs_ld, const float* table, int table_ld, float clip, double* partial, hipStream_t stream);
// the partials in index order, Chan's merge into stats [1 + 2 O] = n | mean | M2, then the table (columns O .. table_ld - 1: 0 / 1)
int32_t obs_norm_update_launch(int O, int n_partials, long long rows, const double* partial, double* stats, float eps, float* table, int table_ld, hipStream_t stream);
// several ranks: this rank's partials in index order -> slots[rank] of slots [world][2][O] (a -0.0 sum as +0.0), every other slot +0.0; the gathered slots are
// obs_norm_update_launch's partials (n_partials = world, rows summed over the ranks)
int32_t obs_norm_rank_sums_launch(int O, int n_partials, const double* partial, int rank, int world, double* slots, hipStream_t stream);

}  // namespace mppo
