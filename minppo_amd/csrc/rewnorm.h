// rewnorm.h - reward scaling by the running deviation of the discounted return (k_rewnorm.hip), shared with the engine's rollout (engine.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/minppo_hip.h"
#include "mppo_common.h"

namespace mppo {

// one apply workgroup: 4 waves, one thread per environment (the geometry of gae_kernel); 4096 environments are 16 workgroups and 16 partial sums
constexpr int kRewNormThreads = 256;
inline int reward_norm_partials(int N) { return cdiv(N, kRewNormThreads); }

// ret = ret * gamma + reward forward over t from carry[n]; scaled = reward * table[1], clamped where clip > 0 (scaled may be reward itself);
// partial (may be null): [G][2] sums of d = (double)ret - (double)table[0] and of d^2.  The merge is obs_norm_update_launch(1, G, T * N, ..., table_ld = 1)
int32_t reward_norm_apply_launch(int T, int N, float gamma, const float* reward, const unsigned char* done, float* carry, const float* table, float clip, float* scaled,
                                 double* partial, hipStream_t stream);

}  // namespace mppo
