// TEST INFRASTRUCTURE - gemm_bounds: mppo_gemm_batch of the emulator build (k_gemm.hip + k_gemm_lds.hip, nothing else of the library) as a
// stand-alone program for a build under the host sanitizers (tests/test_exact_products.py).  Every operand, index list and result lives in a
// heap block of exactly its size, so that a read or write one row or one element past it is a read or write past the block: the clamps of
// out-of-tile lanes (row R - 1, index kend - 1) and the predicates of the k-tails are what keeps the kernels inside.  Values are not looked
// at here.  Prints one line per launch that was refused and "ok" at the end.
#include <cstdio>
#include <cstdlib>

#include <minppo_hip.h>

namespace mppo {
char* last_error_buf() { static thread_local char buf[512]; return buf; }
}
extern "C" const char* mppo_last_error(void) { return mppo::last_error_buf(); }

static float* mat(size_t n) {
  float* p = static_cast<float*>(malloc(sizeof(float) * n));
  for (size_t i = 0; i < n; ++i) p[i] = 0.5f * (float)((int)(i % 5) - 2);
  return p;
}

int main() {
  int bad = 0, launches = 0;
  // M, N, K: full k-sets only, tails, one row / column, tiles of 32 and 64 with and without a remainder
  const int shapes[][3] = {{33, 33, 64}, {1, 65, 96}, {65, 31, 40}, {129, 64, 33}, {32, 1, 7}};
  for (const auto& s : shapes) {
    const int M = s[0], N = s[1], K = s[2];
    for (int variant = 0; variant < 3; ++variant)
      for (int bf16 = 0; bf16 < 2; ++bf16)
        for (int gathered = 0; gathered < 2; ++gathered)
          for (int pad = 0; pad < 2; ++pad) {  // pad 1: leading dimensions rounded up to 4 floats (float4 loaders, the LDS kernel's fast form)
            if ((variant == 1 || (variant == 2 && gathered)) && bf16) continue;  // refused by the launcher
            if (variant == 1 && gathered) continue;                                // (no other kernel than without)
            const int ar = variant == 2 ? K : M, ac = variant == 2 ? M : K, br = variant == 1 ? N : K, bc = variant == 1 ? K : N;
            const int lda = pad ? (ac + 3) / 4 * 4 : ac, ldb = pad ? (bc + 3) / 4 * 4 : bc, ldc = pad ? (N + 3) / 4 * 4 : N;
            const int ks = variant == 2 ? 3 : 1;
            const size_t slab = (size_t)M * ldc + N;
            float *A = mat((size_t)ar * lda), *B = mat((size_t)br * ldb), *Cm = mat(ks * slab), *aux = mat((size_t)M * N), *bias = mat(N);
            int32_t* idx = static_cast<int32_t*>(malloc(sizeof(int32_t) * ar));
            for (int i = 0; i < ar; ++i) idx[i] = ar - 1 - i;
            mppo_gemm_desc_t d{A, B, Cm, variant == 0 ? bias : nullptr, variant == 1 ? aux : nullptr, gathered ? idx : nullptr, variant == 2 ? Cm + (size_t)M * ldc : nullptr,
                               M, N, K, lda, ldb, ldc, N, 2};
            ++launches;
            if (mppo_gemm_batch(&d, 1, variant, ks, slab, bf16, nullptr) != 0) { printf("refused: %s\n", mppo_last_error()); ++bad; }
            free(A); free(B); free(Cm); free(aux); free(bias); free(idx);
          }
  }
  printf("%d launches: %s\n", launches, bad ? "FAILED" : "ok");
  return bad;
}
