// k_domrand.hip - mppo_domain_fill: the domain randomisation's draw (domrand.h) written out as the [N][4] table the environment kernel's randomised
// instantiations read.  One launch when the environments are created - nothing is drawn in a step: the parameters hold for the whole run.
#include "domrand.h"

namespace mppo {

__global__ void __launch_bounds__(256) domain_fill_kernel(DomainDraw p, int N, float* __restrict__ domain) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  domain_draw(p, (unsigned)n, domain + (size_t)n * 4);
}

int32_t domain_fill_launch(const mppo_domain_cfg_t& c, int N, float* domain, hipStream_t stream) {
  const DomainDraw p{c.friction_min, c.friction_max, c.actuator_min, c.actuator_max, c.mass_min, c.mass_max, c.seed, kStreamDomain + ((unsigned long long)c.rank << 16)};
  hipLaunchKernelGGL(domain_fill_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, p, N, domain);
  MPPO_CHECK_LAUNCH("domain_fill_kernel");
  return MPPO_OK;
}

}  // namespace mppo

extern "C" int32_t mppo_domain_fill(const mppo_domain_cfg_t* cfg, int32_t N, float* domain, void* stream) {
  using namespace mppo;
  MPPO_REQUIRE(cfg, "mppo_domain_fill: null configuration");
  MPPO_REQUIRE(domain, "mppo_domain_fill: null table (domain, [N][4] floats in device memory)");
  MPPO_REQUIRE(N >= 1, "mppo_domain_fill: N = %d", N);
  MPPO_TRY(check_domain_cfg("mppo_domain_fill", nullptr, cfg));
  return domain_fill_launch(*cfg, N, domain, static_cast<hipStream_t>(stream));
}
