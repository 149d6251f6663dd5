// fp8 (OCP e4m3) decode GEMVs and the activation quantizers that feed them.
//
//   y[1,N] = (x8 * xs) @ (W8[N,K] * ws[N])^T
//
// Same tiling as gemv.hip but HALF the streamed weight bytes (the decode
// roofline); the weights are the row-wise quantized ones the prefill GEMM
// (gemm_fp8.hip) uses. Row-wise scales factor out of the dot product, so
// dequantization is one multiply in the store. The loop pair, the reduce and
// dot16_fp8 (cvt_pk fp8->f32 row dot) are row_dot / E4m3Row (gemv_rows.h).

#include "common.h"
#include "gemv_rows.h"
#include "launchers.h"
#include "rope_epilogue.h"

// ---------------------------------------------------------------------------
// Pre-quantized x: x8[K] e4m3 + xs[1], streamed from global with the weights
// ---------------------------------------------------------------------------

extern "C" __global__ void __launch_bounds__(256)
gemv_fp8_kernel(const uint8_t *__restrict__ x, const float *__restrict__ xs,
                const uint8_t *__restrict__ w, const float *__restrict__ wsc,
                ushort_t *__restrict__ y, int K, int N) {
  const RowGeom<16> g;
  if (g.n >= N) return;
  const float acc =
      row_dot<E4m3Row, 16, 4, X_GLOBAL>(x, w + (size_t)g.n * K, K, g.sl);
  if (g.sl == 0) y[g.n] = f32_to_bf16(acc * xs[0] * wsc[g.n]);
}

// 32-lanes-per-row variant for SMALL N (same rationale as gemv.hip)
extern "C" __global__ void __launch_bounds__(256)
gemv_fp8_kernel_w32(const uint8_t *__restrict__ x, const float *__restrict__ xs,
                    const uint8_t *__restrict__ w, const float *__restrict__ wsc,
                    ushort_t *__restrict__ y, int K, int N) {
  const RowGeom<32> g;
  if (g.n >= N) return;
  const float acc =
      row_dot<E4m3Row, 32, 4, X_GLOBAL>(x, w + (size_t)g.n * K, K, g.sl);
  if (g.sl == 0) y[g.n] = f32_to_bf16(acc * xs[0] * wsc[g.n]);
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
  const RowGeom<32> g;
  // epilogue operands first: their latency hides under the weight stream
  const RopeKvPre pre = rope_kv_prefetch(ra, g.n_even);
  const float ws_n = wsc[g.n];
  const float acc =
      row_dot<E4m3Row, 32, 4, X_GLOBAL>(x, w + (size_t)g.n * K, K, g.sl);
  rope_kv_store(pre, y, g.n_even, acc * xs[0] * ws_n, g.lane);
}

// residual-add epilogue fp8 GEMV: resid[n] += (x8 . w8[n]) * xs * wsc[n]
extern "C" __global__ void __launch_bounds__(256)
gemv_fp8_res_w32_kernel(const uint8_t *__restrict__ x,
                        const float *__restrict__ xs,
                        const uint8_t *__restrict__ w,
                        const float *__restrict__ wsc,
                        ushort_t *__restrict__ resid, int K, int N) {
  const RowGeom<32> g;
  if (g.n >= N) return;
  const float r0 = bf16_to_f32(resid[g.n]);  // prefetch (tail-latency)
  const float ws_n = wsc[g.n];
  const float acc =
      row_dot<E4m3Row, 32, 4, X_GLOBAL>(x, w + (size_t)g.n * K, K, g.sl);
  if (g.sl == 0) resid[g.n] = f32_to_bf16(r0 + acc * xs[0] * ws_n);
}

// fused fp8 gate_up GEMV + SwiGLU: act[n] = silu(g)*u with
// g = (x8 . wg[n])*xs*wsc[n], u = (x8 . wu[n])*xs*wsc[n+F]
extern "C" __global__ void __launch_bounds__(256)
gemv_fp8_gateup_kernel(const uint8_t *__restrict__ x,
                       const float *__restrict__ xs,
                       const uint8_t *__restrict__ w,
                       const float *__restrict__ wsc,
                       ushort_t *__restrict__ act, int K, int F) {
  const RowGeom<32> g;
  if (g.n >= F) return;
  const uint8_t *const gu[2] = {w + (size_t)g.n * K,
                                w + (size_t)(g.n + F) * K};
  float a[2];  // gate, up
  row_dot<E4m3Row, 32, 4, X_GLOBAL>(x, gu, K, g.sl, a);
  if (g.sl == 0)
    act[g.n] = f32_to_bf16(silu_mul(a[0] * xs[0] * wsc[g.n],
                                    a[1] * xs[0] * wsc[g.n + F]));
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

// y = (rmsnorm(x,wln) @ w8^T) — rmsnorm + quantize + GEMV in ONE launch
extern "C" __global__ void __launch_bounds__(256)
gemv_fp8_norm_w32_kernel(const ushort_t *__restrict__ x,
                         const ushort_t *__restrict__ wln,
                         const uint8_t *__restrict__ w,
                         const float *__restrict__ wsc,
                         ushort_t *__restrict__ y, int K, int N, float eps) {
  extern __shared__ uint8_t xl8[];
  __shared__ float red[16];
  const RowGeom<32> g;
  const int n = g.n < N ? g.n : N - 1;  // no early return before barriers
  const float s = fp8norm_stage(x, wln, xl8, red, K, eps, true);
  const float acc =
      row_dot<E4m3Row, 32, 4, X_LDS>(xl8, w + (size_t)n * K, K, g.sl);
  if (g.sl == 0 && g.n < N) y[g.n] = f32_to_bf16(acc * s * wsc[g.n]);
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
  const RowGeom<16> g;
  const int n = g.n < N ? g.n : N - 1;
  const float s = fp8norm_stage(x, wln, xl8, red, K, eps, true);
  const float acc =
      row_dot<E4m3Row, 16, 4, X_LDS>(xl8, w + (size_t)n * K, K, g.sl);
  if (g.sl == 0 && g.n < N) y[g.n] = f32_to_bf16(acc * s * wsc[g.n]);
}

// resid += (x @ w8^T): quantize-in-LDS + GEMV + residual epilogue
extern "C" __global__ void __launch_bounds__(256)
gemv_fp8_resl_w32_kernel(const ushort_t *__restrict__ x,
                         const uint8_t *__restrict__ w,
                         const float *__restrict__ wsc,
                         ushort_t *__restrict__ resid, int K, int N) {
  extern __shared__ uint8_t xl8[];
  __shared__ float red[16];
  const RowGeom<32> g;
  const int n = g.n < N ? g.n : N - 1;
  const float r0 = bf16_to_f32(resid[n]);  // prefetch
  const float s = fp8norm_stage(x, nullptr, xl8, red, K, 0.f, false);
  const float acc =
      row_dot<E4m3Row, 32, 4, X_LDS>(xl8, w + (size_t)n * K, K, g.sl);
  if (g.sl == 0 && g.n < N) resid[g.n] = f32_to_bf16(r0 + acc * s * wsc[g.n]);
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
  const RowGeom<32> g;
  const int n = g.n < F ? g.n : F - 1;
  const float s = fp8norm_stage(x, wln, xl8, red, K, eps, true);
  const uint8_t *const gu[2] = {w + (size_t)n * K, w + (size_t)(n + F) * K};
  float a[2];  // gate, up
  row_dot<E4m3Row, 32, 4, X_LDS>(xl8, gu, K, g.sl, a);
  if (g.sl == 0 && g.n < F)
    act[g.n] = f32_to_bf16(silu_mul(a[0] * s * wsc[g.n],
                                    a[1] * s * wsc[g.n + F]));
}

// ---------------------------------------------------------------------------
// Launchers
// ---------------------------------------------------------------------------

extern "C" void launch_gemv_fp8(const uint8_t *x, const float *xs,
                                const uint8_t *w, const float *wsc,
                                ushort_t *y, int K, int N,
                                hipStream_t stream) {
  // NOTE measured-and-rejected: an MFMA-based variant (one
  // mfma_f32_16x16x32_fp8_fp8 per 16-row block with x broadcast as the A
  // operand and fragment-layout direct loads of W; since deleted) ran
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

extern "C" void launch_quant_fp8(const ushort_t *x, uint8_t *q, float *scale,
                                 int M, int K, hipStream_t stream) {
  quant_fp8_row_kernel<<<dim3(M), 256, 0, stream>>>(x, q, scale, K);
}

extern "C" void launch_quant_norm_fp8(const ushort_t *x, const ushort_t *wln,
                                      uint8_t *q, float *scale, int K,
                                      float eps, hipStream_t stream) {
  quant_norm_fp8_kernel<<<dim3(1), 256, 0, stream>>>(x, wln, q, scale, K, eps);
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
