// fp8 (OCP e4m3) prefill GEMMs with row-wise scales: the two tile loops of
// gemm_tiles.h over TileE4m3, v_mfma_f32_16x16x32_fp8_fp8.
//
// BASELINE config 5: the 32k-token long-context prefill runs the projection
// GEMMs in fp8. The decode GEMVs over the same quantized weights, and the
// activation quantizers, are in gemv_fp8.hip.

#include "gemm_tiles.h"
#include "launchers.h"

__global__ void __launch_bounds__(256, 2)
gemm_fp8_kernel(const uint8_t *__restrict__ a, const float *__restrict__ asc,
                const uint8_t *__restrict__ b, const float *__restrict__ bsc,
                ushort_t *__restrict__ c_out, int M, int N, int K) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[2 * 2 * GT_IMG];
  gemm128_tiles<TileE4m3>::run(a, asc, b, bsc, c_out, M, N, K, lds);
}

__global__ void __launch_bounds__(512, 2)
gemm_fp8_256_kernel(const uint8_t *__restrict__ a,
                    const float *__restrict__ asc,
                    const uint8_t *__restrict__ b,
                    const float *__restrict__ bsc,
                    ushort_t *__restrict__ c_out, int M, int N, int K) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[2 * 4 * GT_IMG];
  gemm256_tiles<TileE4m3>::run(a, asc, b, bsc, c_out, M, N, K, lds);
}

extern "C" void launch_gemm_fp8(const uint8_t *a, const float *asc,
                                const uint8_t *b, const float *bsc,
                                ushort_t *c, int M, int N, int K,
                                hipStream_t stream) {
  dim3 grid((N + 127) / 128, (M + 127) / 128);
  gemm_fp8_kernel<<<grid, 256, 0, stream>>>(a, asc, b, bsc, c, M, N, K);
}

extern "C" void launch_gemm_fp8_256(const uint8_t *a, const float *asc,
                                    const uint8_t *b, const float *bsc,
                                    ushort_t *c, int M, int N, int K,
                                    hipStream_t stream) {
  dim3 grid((N + 255) / 256, (M + 255) / 256);
  gemm_fp8_256_kernel<<<grid, 512, 0, stream>>>(a, asc, b, bsc, c, M, N, K);
}
