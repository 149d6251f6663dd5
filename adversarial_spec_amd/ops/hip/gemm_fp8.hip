// fp8 (OCP e4m3) MFMA GEMM + GEMV for CDNA4 (gfx950).
//
//   C[M,N] = (A8[M,K] * a_scale[M]) @ (B8[N,K] * b_scale[N])^T
//
// BASELINE config 5: the 32k-token long-context prefill runs the
// projection GEMMs on v_mfma_f32_16x16x32_fp8_fp8 with row-wise scales
// (scales factor out of the dot product, so dequantization is exact in
// the epilogue). fp8 also HALVES the weight bytes streamed by the
// bandwidth-bound decode GEMV — the decode path uses the same quantized
// weights.
//
// Same step-3 structure as gemm.hip (128x128 tile, BK=64 elements,
// double-buffered global_load_lds staging, source-XOR swizzle) with
// half-width rows: an image row is 64 B (4 x 16 B chunks), fragments are
// 8 fp8 = 8 B per lane read as the low/high half of a swizzled 16 B chunk.

#include "common.h"
#include "launchers.h"
#include "rope_epilogue.h"

typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4v;
typedef __attribute__((__vector_size__(2 * sizeof(float)))) float f32x2v;

// hardware fp8->f32: converts byte pair (word ? bytes 2,3 : bytes 0,1)
DEVINL float dot16_fp8(const uint4 &xv, const uint4 &wv) {
  const int *x32 = (const int *)&xv;
  const int *w32 = (const int *)&wv;
  float acc = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x2v xl = __builtin_amdgcn_cvt_pk_f32_fp8(x32[q], false);
    const f32x2v xh = __builtin_amdgcn_cvt_pk_f32_fp8(x32[q], true);
    const f32x2v wl = __builtin_amdgcn_cvt_pk_f32_fp8(w32[q], false);
    const f32x2v wh = __builtin_amdgcn_cvt_pk_f32_fp8(w32[q], true);
    acc += xl[0] * wl[0] + xl[1] * wl[1] + xh[0] * wh[0] + xh[1] * wh[1];
  }
  return acc;
}

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

// ---------------------------------------------------------------------------
// fp8 decode GEMV: y[1,N] = (x8 * xs) @ (W8[N,K] * ws[N])^T — same tiling
// as gemv.hip but HALF the streamed bytes (the decode roofline).
// ---------------------------------------------------------------------------

DEVINL float fp8_to_f32(uint8_t v) {
  // OCP e4m3fn (1s 4e 3m, bias 7) -> f32 by bit manipulation: for normals
  // the f32 exponent is e+(127-7) and the mantissa top 3 bits are m, so
  // bits = sign | (em + (120<<3)) << 20. Subnormals: m * 2^-9.
  // em == 0x7f is NaN in e4m3fn (no infinities, +-NaN only): map it to a
  // real f32 NaN so NaN-poisoned quantized weights surface on GPU exactly
  // like the CPU float8_e4m3fn reference instead of decoding to ~480.
  const uint32_t s = (uint32_t)(v & 0x80u) << 24;
  const uint32_t em = v & 0x7fu;
  uint32_t bits;
  if (em == 0x7fu) {
    bits = s | 0x7fc00000u;
  } else if (em >= 8u) {
    bits = s | ((em + 960u) << 20);
  } else {
    bits = s | __builtin_bit_cast(uint32_t, (float)em * 0.001953125f);
  }
  return __builtin_bit_cast(float, bits);
}

// MFMA-based fp8 decode GEMV: y[n0..n0+15] computed by ONE block.
// The cvt_pk dot path above is VALU/issue-bound (24 ops per 16 weight
// bytes -> 2.4-3.6 TB/s effective, round-2 profile); one
// mfma_f32_16x16x32_fp8_fp8 instead consumes 512 weight bytes per
// ~20-cycle instruction, pushing the kernel back to the weight-streaming
// bound. A operand = the x chunk broadcast to all 16 rows (only C row 0
// is real and read); the 4 waves split K and combine partials in LDS.
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4v_;

extern "C" __global__ void __launch_bounds__(256)
gemv_fp8_mfma_kernel(const uint8_t *__restrict__ x,
                     const float *__restrict__ xs,
                     const uint8_t *__restrict__ w,
                     const float *__restrict__ wsc,
                     ushort_t *__restrict__ y, int K, int N) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int col = lane & 15;          // output column within the tile
  const int ksl = lane >> 4;          // k-slice quarter: 0..3
  const int n0 = blockIdx.x * 16;
  const int n = n0 + col;

  // wave k-range: quarter of K, multiple of 32 (K % 128 == 0 dispatch)
  const int kq = K / 4;
  const int k0 = wid * kq;

  const uint8_t *wr = w + (size_t)min(n, N - 1) * K;  // clamp: tail cols
  f32x4v_ acc0 = {0.f, 0.f, 0.f, 0.f};
  f32x4v_ acc1 = {0.f, 0.f, 0.f, 0.f};
  // 2-step unroll: two independent accumulator chains cover the MFMA
  // dependent latency; loads for both steps issue together.
  for (int k = k0; k < k0 + kq; k += 64) {
    const long wv0 = *(const long *)(wr + (size_t)k + ksl * 8);
    const long xv0 = *(const long *)(x + (size_t)k + ksl * 8);
    const long wv1 = *(const long *)(wr + (size_t)k + 32 + ksl * 8);
    const long xv1 = *(const long *)(x + (size_t)k + 32 + ksl * 8);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(xv0, wv0, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(xv1, wv1, acc1, 0, 0, 0);
  }

  // C row 0 lives in lanes 0-15, register 0
  __shared__ float part[4][16];
  if (lane < 16) part[wid][lane] = acc0[0] + acc1[0];
  __syncthreads();
  if (threadIdx.x < 16 && n0 + (int)threadIdx.x < N) {
    const float s = part[0][threadIdx.x] + part[1][threadIdx.x] +
                    part[2][threadIdx.x] + part[3][threadIdx.x];
    y[n0 + threadIdx.x] =
        f32_to_bf16(s * xs[0] * wsc[n0 + threadIdx.x]);
  }
}

extern "C" __global__ void __launch_bounds__(256)
gemv_fp8_kernel(const uint8_t *__restrict__ x, const float *__restrict__ xs,
                const uint8_t *__restrict__ w, const float *__restrict__ wsc,
                ushort_t *__restrict__ y, int K, int N) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int rg = lane >> 4;
  const int sl = lane & 15;
  const int n = blockIdx.x * 16 + wid * 4 + rg;
  if (n >= N) return;

  const uint8_t *wr = w + (size_t)n * K;
  const int nc = K / 16;  // 16 B chunks of 16 fp8 (K % 16 == 0)

  float acc = 0.f;
  int c = sl;
  for (; c + 48 < nc; c += 64) {
    uint4 wv[4], xv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      wv[u] = *(const uint4 *)(wr + (size_t)(c + 16 * u) * 16);
      xv[u] = *(const uint4 *)(x + (size_t)(c + 16 * u) * 16);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc += dot16_fp8(xv[u], wv[u]);
  }
  for (; c < nc; c += 16) {
    const uint4 wv = *(const uint4 *)(wr + (size_t)c * 16);
    const uint4 xv = *(const uint4 *)(x + (size_t)c * 16);
    acc += dot16_fp8(xv, wv);
  }

#pragma unroll
  for (int off = 8; off > 0; off >>= 1) acc += __shfl_xor(acc, off, WAVE);
  if (sl == 0) y[n] = f32_to_bf16(acc * xs[0] * wsc[n]);
}

// ---------------------------------------------------------------------------
// Row-wise fp8 quantizer: in[M,K] bf16 -> out[M,K] e4m3 + scale[M] f32
// (scale = rowmax/448; allocation-free out-variant for the decode graph).
// One block per row.
// ---------------------------------------------------------------------------

DEVINL uint8_t f32_to_fp8(float f) {
  // float -> e4m3fn by the hardware packed convert (kv_fp8.hip uses the same
  // one): round-to-nearest-even, subnormal-to-normal carry included, OCP
  // encoding on gfx950. Saturates to +-448 in front of it, so a quotient
  // that rounded a hair above 448 stays finite; a NaN passes both compares
  // and converts to the e4m3fn NaN.
  if (f > 448.f) f = 448.f;
  if (f < -448.f) f = -448.f;
  return (uint8_t)(__builtin_amdgcn_cvt_pk_fp8_f32(f, 0.f, 0, false) & 0xffu);
}

extern "C" __global__ void __launch_bounds__(256)
quant_fp8_row_kernel(const ushort_t *__restrict__ x, uint8_t *__restrict__ q,
                     float *__restrict__ scale, int K) {
  __shared__ float scratch[16];
  const int row = blockIdx.x;
  const ushort_t *xr = x + (size_t)row * K;
  uint8_t *qr = q + (size_t)row * K;
  const int nv = K / 8;

  float amax = 0.f;
  for (int i = threadIdx.x; i < nv; i += blockDim.x) {
    const f32x8 v = unpack8(((const bf16x8 *)xr)[i]);
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v.v[j]));
  }
  amax = block_reduce_max(amax, scratch);
  const float s = (amax > 0.f) ? amax / 448.f : 1.f;
  const float inv = 1.f / s;
  if (threadIdx.x == 0) scale[row] = s;

  for (int i = threadIdx.x; i < nv; i += blockDim.x) {
    const f32x8 v = unpack8(((const bf16x8 *)xr)[i]);
#pragma unroll
    for (int j = 0; j < 8; ++j) qr[i * 8 + j] = f32_to_fp8(v.v[j] * inv);
  }
}

extern "C" void launch_gemm_fp8(const uint8_t *a, const float *asc,
                                const uint8_t *b, const float *bsc,
                                ushort_t *c, int M, int N, int K,
                                hipStream_t stream) {
  dim3 grid((N + F8_N - 1) / F8_N, (M + F8_M - 1) / F8_M);
  gemm_fp8_kernel<<<grid, 256, 0, stream>>>(a, asc, b, bsc, c, M, N, K);
}

// 32-lanes-per-row variant for SMALL N (same rationale as gemv.hip)
extern "C" __global__ void __launch_bounds__(256)
gemv_fp8_kernel_w32(const uint8_t *__restrict__ x, const float *__restrict__ xs,
                    const uint8_t *__restrict__ w, const float *__restrict__ wsc,
                    ushort_t *__restrict__ y, int K, int N) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int rg = lane >> 5;
  const int sl = lane & 31;
  const int n = blockIdx.x * 8 + wid * 2 + rg;
  if (n >= N) return;

  const uint8_t *wr = w + (size_t)n * K;
  const int nc = K / 16;

  float acc = 0.f;
  int c = sl;
  for (; c + 96 < nc; c += 128) {
    uint4 wv[4], xv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      wv[u] = *(const uint4 *)(wr + (size_t)(c + 32 * u) * 16);
      xv[u] = *(const uint4 *)(x + (size_t)(c + 32 * u) * 16);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc += dot16_fp8(xv[u], wv[u]);
  }
  for (; c < nc; c += 32) {
    const uint4 wv = *(const uint4 *)(wr + (size_t)c * 16);
    const uint4 xv = *(const uint4 *)(x + (size_t)c * 16);
    acc += dot16_fp8(xv, wv);
  }

#pragma unroll
  for (int off = 16; off > 0; off >>= 1) acc += __shfl_xor(acc, off, WAVE);
  if (sl == 0) y[n] = f32_to_bf16(acc * xs[0] * wsc[n]);
}

// fp8 twin of gemv_norm_rope_kv_w32_kernel (gemv.hip): gemv_fp8_kernel_w32's
// weight loop with the RoPE + KV-append store of rope_epilogue.h. Same
// preconditions: N == (hq + 2*kh)*hd, hd % 16 == 0 (so N % 8 == 0).
extern "C" __global__ void __launch_bounds__(256)
gemv_fp8_rope_kv_w32_kernel(const uint8_t *__restrict__ x,
                            const float *__restrict__ xs,
                            const uint8_t *__restrict__ w,
                            const float *__restrict__ wsc,
                            ushort_t *__restrict__ y, int K, RopeKvArgs ra) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int rg = lane >> 5;
  const int sl = lane & 31;
  const int n_even = blockIdx.x * 8 + wid * 2;
  const int n = n_even + rg;

  // epilogue operands first: their latency hides under the weight stream
  const RopeKvPre pre = rope_kv_prefetch(ra, n_even);
  const float ws_n = wsc[n];

  const uint8_t *wr = w + (size_t)n * K;
  const int nc = K / 16;

  float acc = 0.f;
  int c = sl;
  for (; c + 96 < nc; c += 128) {
    uint4 wv[4], xv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      wv[u] = *(const uint4 *)(wr + (size_t)(c + 32 * u) * 16);
      xv[u] = *(const uint4 *)(x + (size_t)(c + 32 * u) * 16);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc += dot16_fp8(xv[u], wv[u]);
  }
  for (; c < nc; c += 32) {
    const uint4 wv = *(const uint4 *)(wr + (size_t)c * 16);
    const uint4 xv = *(const uint4 *)(x + (size_t)c * 16);
    acc += dot16_fp8(xv, wv);
  }

#pragma unroll
  for (int off = 16; off > 0; off >>= 1) acc += __shfl_xor(acc, off, WAVE);
  rope_kv_store(pre, y, n_even, acc * xs[0] * ws_n, lane);
}

extern "C" void launch_gemv_fp8_rope_kv(const uint8_t *x, const float *xs,
                                        const uint8_t *w, const float *wsc,
                                        ushort_t *y, int K,
                                        const RopeKvArgs &ra,
                                        hipStream_t stream) {
  // caller checked: hd % 16 == 0, N <= 8192
  const int N = (ra.hq + 2 * ra.kh) * ra.hd;
  gemv_fp8_rope_kv_w32_kernel<<<dim3(N / 8), 256, 0, stream>>>(x, xs, w, wsc,
                                                               y, K, ra);
}

extern "C" void launch_gemv_fp8(const uint8_t *x, const float *xs,
                                const uint8_t *w, const float *wsc,
                                ushort_t *y, int K, int N,
                                hipStream_t stream) {
  // NOTE measured-and-rejected: an MFMA-based variant
  // (gemv_fp8_mfma_kernel below, fragment-layout direct loads) ran
  // SLOWER than these cvt_pk dot kernels at every decode shape
  // (1.3-3.5 TB/s vs 1.7-3.6): the B-fragment's 8-byte per-lane loads
  // scatter across 16 weight rows and the load ISSUE dominates. A
  // viable MFMA route needs the guide's M=256-projection pattern
  // (stage W and x through LDS in full 128-B lines via glds, 8-B
  // fragment reads from LDS) — future work, not a drop-in.
  if (N <= 8192) {
    gemv_fp8_kernel_w32<<<dim3((N + 7) / 8), 256, 0, stream>>>(x, xs, w, wsc,
                                                               y, K, N);
  } else {
    gemv_fp8_kernel<<<dim3((N + 15) / 16), 256, 0, stream>>>(x, xs, w, wsc, y,
                                                             K, N);
  }
}

extern "C" void launch_quant_fp8(const ushort_t *x, uint8_t *q, float *scale,
                                 int M, int K, hipStream_t stream) {
  quant_fp8_row_kernel<<<dim3(M), 256, 0, stream>>>(x, q, scale, K);
}

// ---------------------------------------------------------------------------
// fp8 decode norm/residual fusion (mirror of the bf16 gemv.hip fusion):
//   quant_norm: rmsnorm + rowwise e4m3 quantize in ONE kernel — the rms
//   scalar commutes, so one pass accumulates sum(x^2) AND amax(x*wln);
//   the quantizer scale is amax*rms/448 and the second pass writes
//   fp8(x*wln*rms/scale). Replaces the separate (add_)rmsnorm + quant
//   launches between every pair of fp8 decode GEMVs.
// ---------------------------------------------------------------------------

extern "C" __global__ void __launch_bounds__(256)
quant_norm_fp8_kernel(const ushort_t *__restrict__ x,
                      const ushort_t *__restrict__ wln,
                      uint8_t *__restrict__ q, float *__restrict__ scale,
                      int K, float eps) {
  __shared__ float scratch[16];
  const int nv = K / 8;

  float amax = 0.f, s2 = 0.f;
  for (int i = threadIdx.x; i < nv; i += blockDim.x) {
    const f32x8 v = unpack8(((const bf16x8 *)x)[i]);
    const f32x8 l = unpack8(((const bf16x8 *)wln)[i]);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      amax = fmaxf(amax, fabsf(v.v[j] * l.v[j]));
      s2 = fmaf(v.v[j], v.v[j], s2);
    }
  }
  // sequential reuse of one scratch is safe: each reduce barriers before
  // and after its scratch reads
  amax = block_reduce_max(amax, scratch);
  s2 = block_reduce_sum(s2, scratch);

  const float rms = rsqrtf(s2 / K + eps);
  const float am = amax * rms;
  const float s = (am > 0.f) ? am / 448.f : 1.f;
  const float inv = rms / s;  // one fused multiplier: x*wln*rms -> /s
  if (threadIdx.x == 0) scale[0] = s;

  for (int i = threadIdx.x; i < nv; i += blockDim.x) {
    const f32x8 v = unpack8(((const bf16x8 *)x)[i]);
    const f32x8 l = unpack8(((const bf16x8 *)wln)[i]);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      q[i * 8 + j] = f32_to_fp8(v.v[j] * l.v[j] * inv);
  }
}

// residual-add epilogue fp8 GEMV: resid[n] += (x8 . w8[n]) * xs * wsc[n]
extern "C" __global__ void __launch_bounds__(256)
gemv_fp8_res_w32_kernel(const uint8_t *__restrict__ x,
                        const float *__restrict__ xs,
                        const uint8_t *__restrict__ w,
                        const float *__restrict__ wsc,
                        ushort_t *__restrict__ resid, int K, int N) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int rg = lane >> 5;
  const int sl = lane & 31;
  const int n = blockIdx.x * 8 + wid * 2 + rg;
  if (n >= N) return;

  const uint8_t *wr = w + (size_t)n * K;
  const int nc = K / 16;
  const float r0 = bf16_to_f32(resid[n]);  // prefetch (tail-latency)
  const float ws_n = wsc[n];

  float acc = 0.f;
  int c = sl;
  for (; c + 96 < nc; c += 128) {
    uint4 wv[4], xv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      wv[u] = *(const uint4 *)(wr + (size_t)(c + 32 * u) * 16);
      xv[u] = *(const uint4 *)(x + (size_t)(c + 32 * u) * 16);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc += dot16_fp8(xv[u], wv[u]);
  }
  for (; c < nc; c += 32) {
    const uint4 wv = *(const uint4 *)(wr + (size_t)c * 16);
    const uint4 xv = *(const uint4 *)(x + (size_t)c * 16);
    acc += dot16_fp8(xv, wv);
  }

#pragma unroll
  for (int off = 16; off > 0; off >>= 1) acc += __shfl_xor(acc, off, WAVE);
  if (sl == 0) resid[n] = f32_to_bf16(r0 + acc * xs[0] * ws_n);
}

// fused fp8 gate_up GEMV + SwiGLU: act[n] = silu(g)*u with
// g = (x8 . wg[n])*xs*wsc[n], u = (x8 . wu[n])*xs*wsc[n+F]
extern "C" __global__ void __launch_bounds__(256)
gemv_fp8_gateup_kernel(const uint8_t *__restrict__ x,
                       const float *__restrict__ xs,
                       const uint8_t *__restrict__ w,
                       const float *__restrict__ wsc,
                       ushort_t *__restrict__ act, int K, int F) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int rg = lane >> 5;
  const int sl = lane & 31;
  const int n = blockIdx.x * 8 + wid * 2 + rg;
  if (n >= F) return;

  const uint8_t *wg = w + (size_t)n * K;
  const uint8_t *wu = w + (size_t)(n + F) * K;
  const int nc = K / 16;

  float ag = 0.f, au = 0.f;
  int c = sl;
  for (; c + 96 < nc; c += 128) {
    uint4 gv[4], uv[4], xv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      gv[u] = *(const uint4 *)(wg + (size_t)(c + 32 * u) * 16);
      uv[u] = *(const uint4 *)(wu + (size_t)(c + 32 * u) * 16);
      xv[u] = *(const uint4 *)(x + (size_t)(c + 32 * u) * 16);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      ag += dot16_fp8(xv[u], gv[u]);
      au += dot16_fp8(xv[u], uv[u]);
    }
  }
  for (; c < nc; c += 32) {
    const uint4 xv = *(const uint4 *)(x + (size_t)c * 16);
    ag += dot16_fp8(xv, *(const uint4 *)(wg + (size_t)c * 16));
    au += dot16_fp8(xv, *(const uint4 *)(wu + (size_t)c * 16));
  }

#pragma unroll
  for (int off = 16; off > 0; off >>= 1) {
    ag += __shfl_xor(ag, off, WAVE);
    au += __shfl_xor(au, off, WAVE);
  }
  if (sl == 0) {
    const float g = ag * xs[0] * wsc[n];
    const float u = au * xs[0] * wsc[n + F];
    const float s = g / (1.0f + __expf(-g));  // silu(gate)
    act[n] = f32_to_bf16(s * u);
  }
}

// ---------------------------------------------------------------------------
// LDS-staged fp8 fused GEMVs: the 1-block quant kernels above are SERIAL
// latency on the decode critical path (~3-4 us each, 3+/layer), exactly
// the launch-bound pattern the bf16 fusion removed. Here every GEMV block
// quantizes its own copy of the activation into LDS (redundant VALU —
// idle at the weight-streaming roofline) and dots from ds_reads, so the
// whole layer is one kernel per projection again.
// ---------------------------------------------------------------------------

// cooperative stage: xl[] = e4m3(x * [wln *] rms / s); returns the
// dequant scale s. One barrier after the writes (the reduce's barriers
// cover only the first pass).
DEVINL float fp8norm_stage(const ushort_t *__restrict__ x,
                           const ushort_t *__restrict__ wln, uint8_t *xl,
                           float *red, int K, float eps, bool norm) {
  const int nv = K / 8;
  float amax = 0.f, s2 = 0.f;
  for (int i = threadIdx.x; i < nv; i += blockDim.x) {
    const f32x8 v = unpack8(((const bf16x8 *)x)[i]);
    f32x8 l;
    if (norm) l = unpack8(((const bf16x8 *)wln)[i]);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float xv = norm ? v.v[j] * l.v[j] : v.v[j];
      amax = fmaxf(amax, fabsf(xv));
      if (norm) s2 = fmaf(v.v[j], v.v[j], s2);
    }
  }
  amax = block_reduce_max(amax, red);
  float mult = 1.f;  // applied before quantize
  if (norm) {
    s2 = block_reduce_sum(s2, red);
    mult = rsqrtf(s2 / K + eps);
  }
  const float am = amax * mult;
  const float s = (am > 0.f) ? am / 448.f : 1.f;
  const float inv = mult / s;
  for (int i = threadIdx.x; i < nv; i += blockDim.x) {
    const f32x8 v = unpack8(((const bf16x8 *)x)[i]);
    f32x8 l;
    if (norm) l = unpack8(((const bf16x8 *)wln)[i]);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float xv = norm ? v.v[j] * l.v[j] : v.v[j];
      xl[i * 8 + j] = f32_to_fp8(xv * inv);
    }
  }
  __syncthreads();  // xl visible to the dot loops
  return s;
}

// fp8 w32 dot loop against LDS-staged activation (shared by the fused
// kernels): 4-deep weight stream, uint4 ds_reads for x.
DEVINL float fp8_dot_lds_w32(const uint8_t *xl, const uint8_t *wr, int nc,
                             int sl) {
  float acc = 0.f;
  int c = sl;
  for (; c + 96 < nc; c += 128) {
    uint4 wv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      wv[u] = *(const uint4 *)(wr + (size_t)(c + 32 * u) * 16);
#pragma unroll
    for (int u = 0; u < 4; ++u)
      acc += dot16_fp8(*(const uint4 *)(xl + (size_t)(c + 32 * u) * 16),
                       wv[u]);
  }
  for (; c < nc; c += 32)
    acc += dot16_fp8(*(const uint4 *)(xl + (size_t)c * 16),
                     *(const uint4 *)(wr + (size_t)c * 16));
  return acc;
}

// y = (rmsnorm(x,wln) @ w8^T) — rmsnorm + quantize + GEMV in ONE launch
extern "C" __global__ void __launch_bounds__(256)
gemv_fp8_norm_w32_kernel(const ushort_t *__restrict__ x,
                         const ushort_t *__restrict__ wln,
                         const uint8_t *__restrict__ w,
                         const float *__restrict__ wsc,
                         ushort_t *__restrict__ y, int K, int N, float eps) {
  extern __shared__ uint8_t xl8[];
  __shared__ float red[16];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int rg = lane >> 5;
  const int sl = lane & 31;
  const int n0 = blockIdx.x * 8 + wid * 2 + rg;
  const int n = n0 < N ? n0 : N - 1;  // no early return before barriers

  const float s = fp8norm_stage(x, wln, xl8, red, K, eps, true);
  float acc = fp8_dot_lds_w32(xl8, w + (size_t)n * K, K / 16, sl);
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) acc += __shfl_xor(acc, off, WAVE);
  if (sl == 0 && n0 < N) y[n0] = f32_to_bf16(acc * s * wsc[n0]);
}

// 16-lane-group variant for LARGE N (lm_head)
extern "C" __global__ void __launch_bounds__(256)
gemv_fp8_norm_kernel(const ushort_t *__restrict__ x,
                     const ushort_t *__restrict__ wln,
                     const uint8_t *__restrict__ w,
                     const float *__restrict__ wsc,
                     ushort_t *__restrict__ y, int K, int N, float eps) {
  extern __shared__ uint8_t xl8[];
  __shared__ float red[16];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int rg = lane >> 4;
  const int sl = lane & 15;
  const int n0 = blockIdx.x * 16 + wid * 4 + rg;
  const int n = n0 < N ? n0 : N - 1;

  const float s = fp8norm_stage(x, wln, xl8, red, K, eps, true);
  const uint8_t *wr = w + (size_t)n * K;
  const int nc = K / 16;
  float acc = 0.f;
  int c = sl;
  for (; c + 48 < nc; c += 64) {
    uint4 wv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      wv[u] = *(const uint4 *)(wr + (size_t)(c + 16 * u) * 16);
#pragma unroll
    for (int u = 0; u < 4; ++u)
      acc += dot16_fp8(*(const uint4 *)(xl8 + (size_t)(c + 16 * u) * 16),
                       wv[u]);
  }
  for (; c < nc; c += 16)
    acc += dot16_fp8(*(const uint4 *)(xl8 + (size_t)c * 16),
                     *(const uint4 *)(wr + (size_t)c * 16));
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) acc += __shfl_xor(acc, off, WAVE);
  if (sl == 0 && n0 < N) y[n0] = f32_to_bf16(acc * s * wsc[n0]);
}

// resid += (x @ w8^T): quantize-in-LDS + GEMV + residual epilogue
extern "C" __global__ void __launch_bounds__(256)
gemv_fp8_resl_w32_kernel(const ushort_t *__restrict__ x,
                         const uint8_t *__restrict__ w,
                         const float *__restrict__ wsc,
                         ushort_t *__restrict__ resid, int K, int N) {
  extern __shared__ uint8_t xl8[];
  __shared__ float red[16];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int rg = lane >> 5;
  const int sl = lane & 31;
  const int n0 = blockIdx.x * 8 + wid * 2 + rg;
  const int n = n0 < N ? n0 : N - 1;

  const float r0 = bf16_to_f32(resid[n]);  // prefetch
  const float s = fp8norm_stage(x, nullptr, xl8, red, K, 0.f, false);
  float acc = fp8_dot_lds_w32(xl8, w + (size_t)n * K, K / 16, sl);
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) acc += __shfl_xor(acc, off, WAVE);
  if (sl == 0 && n0 < N) resid[n0] = f32_to_bf16(r0 + acc * s * wsc[n0]);
}

// act = swiglu(rmsnorm(x,wln) @ [Wg|Wu]^T): the whole fp8 MLP front half
extern "C" __global__ void __launch_bounds__(256)
gemv_fp8_gateup_norm_kernel(const ushort_t *__restrict__ x,
                            const ushort_t *__restrict__ wln,
                            const uint8_t *__restrict__ w,
                            const float *__restrict__ wsc,
                            ushort_t *__restrict__ act, int K, int F,
                            float eps) {
  extern __shared__ uint8_t xl8[];
  __shared__ float red[16];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int rg = lane >> 5;
  const int sl = lane & 31;
  const int n0 = blockIdx.x * 8 + wid * 2 + rg;
  const int n = n0 < F ? n0 : F - 1;

  const float s = fp8norm_stage(x, wln, xl8, red, K, eps, true);
  const uint8_t *wg = w + (size_t)n * K;
  const uint8_t *wu = w + (size_t)(n + F) * K;
  const int nc = K / 16;
  float ag = 0.f, au = 0.f;
  int c = sl;
  for (; c + 96 < nc; c += 128) {
    uint4 gv[4], uv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      gv[u] = *(const uint4 *)(wg + (size_t)(c + 32 * u) * 16);
      uv[u] = *(const uint4 *)(wu + (size_t)(c + 32 * u) * 16);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint4 xv = *(const uint4 *)(xl8 + (size_t)(c + 32 * u) * 16);
      ag += dot16_fp8(xv, gv[u]);
      au += dot16_fp8(xv, uv[u]);
    }
  }
  for (; c < nc; c += 32) {
    const uint4 xv = *(const uint4 *)(xl8 + (size_t)c * 16);
    ag += dot16_fp8(xv, *(const uint4 *)(wg + (size_t)c * 16));
    au += dot16_fp8(xv, *(const uint4 *)(wu + (size_t)c * 16));
  }
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) {
    ag += __shfl_xor(ag, off, WAVE);
    au += __shfl_xor(au, off, WAVE);
  }
  if (sl == 0 && n0 < F) {
    const float g = ag * s * wsc[n0];
    const float u = au * s * wsc[n0 + F];
    const float sg = g / (1.0f + __expf(-g));  // silu(gate)
    act[n0] = f32_to_bf16(sg * u);
  }
}

extern "C" void launch_gemv_fp8_norm(const ushort_t *x, const ushort_t *wln,
                                     const uint8_t *w, const float *wsc,
                                     ushort_t *y, int K, int N, float eps,
                                     hipStream_t stream) {
  const size_t lds = (size_t)K;  // e4m3 staging
  if (N <= 8192)
    gemv_fp8_norm_w32_kernel<<<dim3((N + 7) / 8), 256, lds, stream>>>(
        x, wln, w, wsc, y, K, N, eps);
  else
    gemv_fp8_norm_kernel<<<dim3((N + 15) / 16), 256, lds, stream>>>(
        x, wln, w, wsc, y, K, N, eps);
}

extern "C" void launch_gemv_fp8_resl(const ushort_t *x, const uint8_t *w,
                                     const float *wsc, ushort_t *resid,
                                     int K, int N, hipStream_t stream) {
  gemv_fp8_resl_w32_kernel<<<dim3((N + 7) / 8), 256, (size_t)K, stream>>>(
      x, w, wsc, resid, K, N);
}

extern "C" void launch_gemv_fp8_gateup_norm(const ushort_t *x,
                                            const ushort_t *wln,
                                            const uint8_t *w,
                                            const float *wsc, ushort_t *act,
                                            int K, int F, float eps,
                                            hipStream_t stream) {
  gemv_fp8_gateup_norm_kernel<<<dim3((F + 7) / 8), 256, (size_t)K, stream>>>(
      x, wln, w, wsc, act, K, F, eps);
}

extern "C" void launch_quant_norm_fp8(const ushort_t *x, const ushort_t *wln,
                                      uint8_t *q, float *scale, int K,
                                      float eps, hipStream_t stream) {
  quant_norm_fp8_kernel<<<dim3(1), 256, 0, stream>>>(x, wln, q, scale, K, eps);
}

extern "C" void launch_gemv_fp8_res(const uint8_t *x, const float *xs,
                                    const uint8_t *w, const float *wsc,
                                    ushort_t *resid, int K, int N,
                                    hipStream_t stream) {
  gemv_fp8_res_w32_kernel<<<dim3((N + 7) / 8), 256, 0, stream>>>(x, xs, w, wsc,
                                                                 resid, K, N);
}

extern "C" void launch_gemv_fp8_gateup(const uint8_t *x, const float *xs,
                                       const uint8_t *w, const float *wsc,
                                       ushort_t *act, int K, int F,
                                       hipStream_t stream) {
  gemv_fp8_gateup_kernel<<<dim3((F + 7) / 8), 256, 0, stream>>>(x, xs, w, wsc,
                                                                act, K, F);
}
