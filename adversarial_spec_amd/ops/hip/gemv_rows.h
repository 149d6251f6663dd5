// The one row-dot skeleton of the decode GEMVs (gemv.hip bf16, gemv_fp8.hip
// e4m3). Device-only.
//
// Every decode GEMV kernel is: geometry, optional early return or row clamp,
// optional epilogue prefetch, optional LDS stage of x, row_dot, store. What
// differs between them is an element type, the loop geometry (L lanes per
// row, U-deep unroll), where x lives, one or two rows per lane group, and the
// store; the first four are row_dot's template parameters, the store stays
// in the kernel. tests/gemv_exact_common.py::KERNELS tabulates (L, U, E) per
// kernel and mirrors the loop pair below.
#pragma once

#include <type_traits>

#include "common.h"

// Block = 256 threads = 4 waves; L lanes share a row, so a wave owns WAVE/L
// rows and a block 256/L. n_even is the wave's first row (even for every L
// in use): with L == 32 the wave holds rows n_even and n_even + 1, the
// interleaved pair the RoPE epilogue rotates.
template <int L>
struct RowGeom {
  int lane, sl, n_even, n;
  DEVINL RowGeom()
      : lane(threadIdx.x & (WAVE - 1)),
        sl(lane & (L - 1)),  // k-slice lane: 0..L-1
        n_even(blockIdx.x * (256 / L) + (int)(threadIdx.x / WAVE) * (WAVE / L)),
        n(n_even + (lane >> __builtin_ctz(L))) {}
};

// ---- element traits: a 16 B chunk, its element count, one dot step -------
// The two steps round differently (an fma chain through the accumulator vs
// a sum of products added to it); each stays in the form its kernels had.

struct Bf16Row {
  typedef ushort_t elem;
  typedef bf16x8 chunk;
  static constexpr int E = 8;
  static DEVINL float dot(const chunk &x, const chunk &w, float acc) {
    return dot8_bf16(x, w, acc);
  }
};

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

struct E4m3Row {
  typedef uint8_t elem;
  typedef uint4 chunk;
  static constexpr int E = 16;
  static DEVINL float dot(const chunk &x, const chunk &w, float acc) {
    acc += dot16_fp8(x, w);
    return acc;
  }
};

// x is streamed from global memory with the weights, or was staged in LDS
// (norm_stage_lds, fp8norm_stage) and is read at the point of use
enum XSrc { X_GLOBAL, X_LDS };

// acc[r] = sum over the lane group of x . w[r] for R rows sharing the x
// chunks; valid in every lane of the group on return. Lane sl takes chunks
// sl, sl + L, ..: U at a time, then one at a time.
//
// Issue order of an unrolled step: ALL its weight loads first, so U*R loads
// are in flight per lane before the first dot. Global x is loaded with them;
// LDS x is read inside the dot step, where the ds_read occupies no vmcnt slot
// and the weight stream keeps its latency hiding (see norm_stage_lds in
// gemv.hip for the measurement). The R accumulators are stepped and reduced
// interleaved.
template <class T, int L, int U, XSrc XS, int R>
DEVINL void row_dot(const typename T::elem *x,
                    const typename T::elem *const (&w)[R], int K, int sl,
                    float (&acc)[R]) {
  typedef typename T::chunk chunk;
  // An LDS x chunk feeding one row is read in place by the dot step; feeding
  // two rows it is read once into registers and shared. Each is the form its
  // kernels had: the two select different ds_read widths.
  typedef std::conditional_t<XS == X_LDS && R != 1, const chunk, const chunk &>
      xchunk;
  const chunk *xc = (const chunk *)x;
  const int nc = K / T::E;  // 16 B chunks per row (K % E == 0)

#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.f;
  int c = sl;
  for (; c + (U - 1) * L < nc; c += U * L) {
    chunk wv[R][U], xv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int r = 0; r < R; ++r) wv[r][u] = ((const chunk *)w[r])[c + L * u];
      if constexpr (XS == X_GLOBAL) xv[u] = xc[c + L * u];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      xchunk xu = XS == X_LDS ? xc[c + L * u] : xv[u];
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = T::dot(xu, wv[r][u], acc[r]);
    }
  }
  for (; c < nc; c += L) {
    xchunk xu = xc[c];
#pragma unroll
    for (int r = 0; r < R; ++r)
      acc[r] = T::dot(xu, ((const chunk *)w[r])[c], acc[r]);
  }

#pragma unroll
  for (int off = L / 2; off > 0; off >>= 1) {
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] += __shfl_xor(acc[r], off, WAVE);
  }
}

// one row
template <class T, int L, int U, XSrc XS>
DEVINL float row_dot(const typename T::elem *x, const typename T::elem *w,
                     int K, int sl) {
  const typename T::elem *const wr[1] = {w};
  float acc[1];
  row_dot<T, L, U, XS>(x, wr, K, sl, acc);
  return acc[0];
}

// silu(g) * u, the store of the four gate-up kernels
DEVINL float silu_mul(float g, float u) {
  const float s = g / (1.0f + __expf(-g));
  return s * u;
}
