// fp8 (OCP e4m3) MFMA prefill GEMM for CDNA4 (gfx950).
//
//   C[M,N] = (A8[M,K] * a_scale[M]) @ (B8[N,K] * b_scale[N])^T
//
// BASELINE config 5: the 32k-token long-context prefill runs the
// projection GEMMs on v_mfma_f32_16x16x32_fp8_fp8 with row-wise scales
// (scales factor out of the dot product, so dequantization is exact in
// the epilogue). The decode GEMVs over the same quantized weights, and the
// activation quantizers, are in gemv_fp8.hip.
//
// Same step-3 structure as gemm.hip (128x128 tile, BK=64 elements,
// double-buffered global_load_lds staging, source-XOR swizzle) with
// half-width rows: an image row is 64 B (4 x 16 B chunks), fragments are
// 8 fp8 = 8 B per lane read as the low/high half of a swizzled 16 B chunk.
//
// K contract: the binding (gemm_fp8 in bindings.hip) guarantees
// K % 16 == 0, so every row of A8 and B8 starts 16-byte aligned (the glds
// staging loads 16 B per lane) and the rowwise quantizer, which walks K in
// chunks of 8, writes every code the GEMM reads.

#include "common.h"
#include "launchers.h"

typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4v;

#define F8_M 128
#define F8_N 128
#define F8_K 64   // elements per K-step; one image row = 64 B

DEVINL void glds16_f8(const uint8_t *g, uint8_t *l) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void *)g,
      (__attribute__((address_space(3))) void *)l, 16, 0, 0);
}

// Stage a [128][64] fp8 tile (8 KiB) via glds: 8 wave-instructions of
// 1 KiB (16 rows x 64 B), 2 per wave. Global chunk XOR (row & 3) realizes
// the swizzled image with lane-linear LDS placement.
DEVINL void stage_glds_f8(const uint8_t *__restrict__ src, long row_stride,
                          uint8_t *__restrict__ img, int tid) {
  const int lane = tid & (WAVE - 1);
  const int wid = tid / WAVE;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r0 = (wid * 2 + i) * 16;
    const int row = r0 + (lane >> 2);
    const int c = lane & 3;
    const uint8_t *g = src + (size_t)row * row_stride + (size_t)(c ^ (row & 3)) * 16;
    glds16_f8(g, img + (size_t)r0 * F8_K);
  }
}

DEVINL void stage_edge_f8(const uint8_t *__restrict__ src, long row_stride,
                          int rows_left, int k_left,
                          uint8_t *__restrict__ img, int tid) {
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int piece = tid + 256 * p;   // 512 chunk-pieces of 16 B
    const int row = piece >> 2;        // 0..127
    const int c = piece & 3;           // 16B chunk
    uint8_t v[16];
    const int gk = c * 16;
    if (row < rows_left && gk < k_left) {
      const uint8_t *g = src + (size_t)row * row_stride + gk;
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = (gk + j < k_left) ? g[j] : 0;
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = 0;
    }
    uint8_t *dst = img + (size_t)row * F8_K + (size_t)(c ^ (row & 3)) * 16;
#pragma unroll
    for (int j = 0; j < 16; ++j) dst[j] = v[j];
  }
}

__global__ void __launch_bounds__(256, 2)
gemm_fp8_kernel(const uint8_t *__restrict__ a, const float *__restrict__ asc,
                const uint8_t *__restrict__ b, const float *__restrict__ bsc,
                ushort_t *__restrict__ c_out, int M, int N, int K) {
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid / WAVE;
  const int lrow = lane & 15;
  const int lhi = lane >> 4;

  const int n0 = blockIdx.x * F8_N;
  const int m0 = blockIdx.y * F8_M;
  const int wm = (wid >> 1) * 64;
  const int wn = (wid & 1) * 64;

  __shared__ __attribute__((aligned(16))) uint8_t imgA[2][F8_M * F8_K];
  __shared__ __attribute__((aligned(16))) uint8_t imgB[2][F8_N * F8_K];

  f32x4v acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4v){0.f, 0.f, 0.f, 0.f};

  const int ntiles = (K + F8_K - 1) / F8_K;
  const bool a_edge = (M - m0) < F8_M;
  const bool b_edge = (N - n0) < F8_N;

  auto stage = [&](int kt, int buf) {
    const uint8_t *asrc = a + (size_t)m0 * K + (size_t)kt * F8_K;
    const uint8_t *bsrc = b + (size_t)n0 * K + (size_t)kt * F8_K;
    const bool k_edge = (kt + 1) * F8_K > K;
    if (a_edge || k_edge) {
      stage_edge_f8(asrc, K, M - m0, K - kt * F8_K, imgA[buf], tid);
    } else {
      stage_glds_f8(asrc, K, imgA[buf], tid);
    }
    if (b_edge || k_edge) {
      stage_edge_f8(bsrc, K, N - n0, K - kt * F8_K, imgB[buf], tid);
    } else {
      stage_glds_f8(bsrc, K, imgB[buf], tid);
    }
  };

  stage(0, 0);
  __syncthreads();

  for (int kt = 0; kt < ntiles; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < ntiles) stage(kt + 1, buf ^ 1);

    // 2 k-subtiles of 32 elements: frag = 8 B per lane (low/high half of
    // a swizzled 16 B chunk)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      long afr[4], bfr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = wm + i * 16 + lrow;
        const int byte_off = s * 32 + lhi * 8;           // within the row
        const int ch = (byte_off >> 4) ^ (row & 3);      // 16B chunk
        const int half = (byte_off >> 3) & 1;
        afr[i] = ((const long *)(imgA[buf] + (size_t)row * F8_K + ch * 16))[half];
      }
#pragma unroll
      for (int j2 = 0; j2 < 4; ++j2) {
        const int row = wn + j2 * 16 + lrow;
        const int byte_off = s * 32 + lhi * 8;
        const int ch = (byte_off >> 4) ^ (row & 3);
        const int half = (byte_off >> 3) & 1;
        bfr[j2] = ((const long *)(imgB[buf] + (size_t)row * F8_K + ch * 16))[half];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j2 = 0; j2 < 4; ++j2)
          acc[i][j2] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(
              afr[i], bfr[j2], acc[i][j2], 0, 0, 0);
    }
    __syncthreads();
  }

  // epilogue: dequantize with the row scales (exact: scales factor out)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j2 = 0; j2 < 4; ++j2) {
      const int col = n0 + wn + j2 * 16 + lrow;
      if (col >= N) continue;
      const float bs = bsc[col];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm + i * 16 + lhi * 4 + r;
        if (row >= M) continue;
        c_out[(size_t)row * N + col] =
            f32_to_bf16(acc[i][j2][r] * asc[row] * bs);
      }
    }
  }
}

extern "C" void launch_gemm_fp8(const uint8_t *a, const float *asc,
                                const uint8_t *b, const float *bsc,
                                ushort_t *c, int M, int N, int K,
                                hipStream_t stream) {
  dim3 grid((N + F8_N - 1) / F8_N, (M + F8_M - 1) / F8_M);
  gemm_fp8_kernel<<<grid, 256, 0, stream>>>(a, asc, b, bsc, c, M, N, K);
}
