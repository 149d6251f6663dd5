// bf16 128^2 prefill GEMM: gemm128_tiles of gemm_tiles.h over TileBf16,
// v_mfma_f32_16x16x32_bf16. The 256^2 one is in gemm256.hip; the bindings pick
// one with use_gemm256.

#include "gemm_tiles.h"
#include "launchers.h"

__global__ void __launch_bounds__(256, 2)
gemm_nt_kernel(const ushort_t *__restrict__ a, const ushort_t *__restrict__ b,
               ushort_t *__restrict__ c_out, int M, int N, int K) {
  __shared__ __attribute__((aligned(16))) ushort_t lds[2 * 2 * GT_IMG];
  gemm128_tiles<TileBf16>::run(a, nullptr, b, nullptr, c_out, M, N, K, lds);
}

extern "C" void launch_gemm(const ushort_t *a, const ushort_t *b, ushort_t *c,
                            int M, int N, int K, hipStream_t stream) {
  dim3 grid((N + 127) / 128, (M + 127) / 128);
  gemm_nt_kernel<<<grid, 256, 0, stream>>>(a, b, c, M, N, K);
}

