// The one interface between the kernels (ops/hip/*.hip) and the torch
// bindings (bindings.hip): every host-side launch_* wrapper, declared once.
//
// Included by bindings.hip AND by every .hip that defines a launcher, so a
// definition that drifts from its declaration is a compile error
// ("conflicting declaration of C function") instead of a call that links and
// runs with garbage. Host-only safe: nothing from torch, no device code.
// Kernels (__global__) are never declared here; each stays private to the
// file that defines it and is reached only through its launcher.
//
// Conventions: bf16 tensors travel as ushort_t*, fp8 (e4m3fn) as uint8_t*;
// the stream is always the last argument (the MFMA prefill's *ok excepted);
// launchers validate nothing, the bindings do.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

typedef unsigned short ushort_t;

// RoPE + paged KV append operands of the fused qkv GEMVs. Passed by value
// into the kernels as well (rope_epilogue.h consumes it on the device).
struct RopeKvArgs {
  const float *cost, *sint;  // [max_pos, hd/2] f32
  ushort_t *kc, *vc;         // [n_pages, page, kh, hd] bf16, contiguous
  const int *page_table;
  const int *pos_ptr;        // graph mode: device position word (else null)
  int pos;                   // scalar position when pos_ptr is null
  int hq, kh, hd, page;
};

// Everything of a split-KV decode launch that is not a q/cache/out pointer.
// The grid is (kh, n_splits); ws_* are the per-cache fp32 scratch slices
// [kh*n_splits*group], same, [kh*n_splits*group*hd].
struct DecodeSplitArgs {
  const int *page_table;
  const int *pos_ptr;  // graph mode: true length is *pos_ptr + 1 (else null)
  int seq_len;         // host length, or the bound that sized the splits
  float scale;
  int kh, group, hd, page;
  int split_len, n_splits;
  float *ws_m, *ws_l, *ws_acc;
  int identity;        // page_table[i] == i promised: skip the table read
  int window;          // W >= 1: attend the last W positions only; 0 = all
};

// rope_kv / rope_kv_fp8 block size. decode (t <= 2): one wave per 64-thread
// block spreads the ~48 latency-bound slot-waves over 4x the CUs (the
// 12-block launch measured 11.6 us avg under 3-opponent concurrency).
static inline int rope_kv_block_threads(int t) { return t <= 2 ? 64 : 256; }

extern "C" {

// ---- elementwise.hip ------------------------------------------------------
// x, y [t, d]; w [d]; d % 8 == 0
void launch_rmsnorm(const ushort_t *x, const ushort_t *w, ushort_t *y, int t,
                    int d, float eps, hipStream_t stream);
// resid_out = resid + delta; y = rmsnorm(resid_out) * w
void launch_add_rmsnorm(const ushort_t *resid, const ushort_t *delta,
                        const ushort_t *w, ushort_t *resid_out, ushort_t *y,
                        int t, int d, float eps, hipStream_t stream);
// q [t, hq, hd], k [t, hk, hd] rotated in place; row strides in elements;
// pos_ptr (device int32 word) replaces pos0 when non-null
void launch_rope(ushort_t *q, ushort_t *k, const float *cost,
                 const float *sint, int t, int hq, int hk, int hd, int pos0,
                 long q_rstride, long k_rstride, const int *pos_ptr,
                 hipStream_t stream);
// rope + scatter of rotated k and v into the page pool [.., page, hk, hd]
void launch_rope_kv(ushort_t *q, ushort_t *k, const ushort_t *v,
                    const float *cost, const float *sint, ushort_t *kc,
                    ushort_t *vc, const int *page_table, int t, int hq, int hk,
                    int hd, int pos0, long q_rstride, long k_rstride,
                    long v_rstride, int page, const int *pos_ptr,
                    hipStream_t stream);
// gate, up: [t, f] views sharing row stride in_stride; out [t, f] contiguous
void launch_swiglu(const ushort_t *gate, const ushort_t *up, ushort_t *out,
                   int t, int f, int in_stride, hipStream_t stream);
// k, v [t, kh, hd] contiguous -> page pool rows pos0 .. pos0 + t - 1
void launch_kv_write(const ushort_t *k, const ushort_t *v, ushort_t *kc,
                     ushort_t *vc, const int *page_table, int pos0, int t,
                     int kh, int hd, int page, const int *pos_ptr,
                     hipStream_t stream);

// ---- sampling.hip ---------------------------------------------------------
void launch_sample(const ushort_t *logits, int vocab, float temp,
                   uint32_t seed, int *out, hipStream_t stream);
void launch_sample_state(const ushort_t *logits, int vocab,
                         const float *temp_state, uint32_t *rng_state,
                         int *tok_hist, const int *step_state,
                         long long *tok_long, hipStream_t stream);
void launch_bump(int *pos_state, int *step_state, hipStream_t stream);
// top-p / top-k filtered twins (one 1024-thread block, ~128 KB static LDS);
// top_p in (0, 1], top_k >= 0 (0 = off), vocab % 8 == 0, vocab < 2^24
void launch_sample_filtered(const ushort_t *logits, int vocab, float temp,
                            float top_p, int top_k, uint32_t seed, int *out,
                            hipStream_t stream);
void launch_sample_state_filtered(const ushort_t *logits, int vocab,
                                  const float *temp_state,
                                  const float *top_p_state,
                                  const int *top_k_state, uint32_t *rng_state,
                                  int *tok_hist, const int *step_state,
                                  long long *tok_long, hipStream_t stream);
// mask [vocab] uint8, 1 = kept, from the samplers' own cut
void launch_nucleus_mask(const ushort_t *logits, int vocab, float temp,
                         float top_p, int top_k, uint8_t *mask,
                         hipStream_t stream);

// ---- attention.hip --------------------------------------------------------
// q [hq, hd]; kc, vc [n_pages, page, kh, hd]; out [hq, hd]. Runs the combine
// pass itself when a.n_splits > 1.
void launch_attn_decode_split(const ushort_t *q, const ushort_t *kc,
                              const ushort_t *vc, const DecodeSplitArgs &a,
                              ushort_t *out, hipStream_t stream);
// merge of the per-split (m, l, acc) scratch into out; shared by the bf16
// and fp8 split launchers
void launch_attn_decode_combine(const float *ws_m, const float *ws_l,
                                const float *ws_acc, ushort_t *out,
                                int n_splits, int kh, int group, int hd,
                                hipStream_t stream);
void launch_attn_prefill_simple(const ushort_t *q, const ushort_t *k,
                                const ushort_t *v, ushort_t *out, int tq,
                                int tk, int kv_offset, float scale, int hq,
                                int kh, int hd, int causal, int window,
                                hipStream_t stream);

// ---- attn_prefill_mfma.hip ------------------------------------------------
// *ok = 0 and nothing launched when hd is not the kernel's 128. window =
// W >= 1: query position i sees keys max(0, i - W + 1) .. i; 0 = no window
// (launch_attn_prefill_simple takes the same argument, causal only).
void launch_attn_prefill_mfma(const ushort_t *q, const ushort_t *k,
                              const ushort_t *v, ushort_t *out, int tq, int tk,
                              int kv_offset, float scale, int hq, int kh,
                              int hd, int window, hipStream_t stream, int *ok);
void launch_attn_prefill_mfma_abl(const ushort_t *q, const ushort_t *k,
                                  const ushort_t *v, ushort_t *out, int tq,
                                  int tk, float scale, int hq, int kh, int abl,
                                  hipStream_t stream);
// d[16,16] f32 = a[16,32] @ b[32,16]
void launch_mfma_probe16(const ushort_t *a, const ushort_t *b, float *d,
                         hipStream_t stream);

// ---- kv_fp8.hip -----------------------------------------------------------
// as launch_attn_decode_split over an e4m3 cache; ksc, vsc [n_pages, kh, page]
void launch_attn_decode_split_fp8(const ushort_t *q, const uint8_t *kc,
                                  const uint8_t *vc, const float *ksc,
                                  const float *vsc, const DecodeSplitArgs &a,
                                  ushort_t *out, hipStream_t stream);
void launch_rope_kv_fp8(ushort_t *q, ushort_t *k, const ushort_t *v,
                        const float *cost, const float *sint, uint8_t *kc,
                        uint8_t *vc, float *ksc, float *vsc,
                        const int *page_table, int t, int hq, int hk, int hd,
                        int pos0, long q_rstride, long k_rstride,
                        long v_rstride, int page, const int *pos_ptr,
                        hipStream_t stream);
// cache positions [0, n) -> kout, vout [n, kh, hd] bf16
void launch_kv_dequant_fp8(const uint8_t *kc, const uint8_t *vc,
                           const float *ksc, const float *vsc,
                           const int *page_table, ushort_t *kout,
                           ushort_t *vout, int n, int kh, int hd, int page,
                           hipStream_t stream);

// ---- gemv.hip: y[N] = x[K] @ w[N, K]^T, K before N ------------------------
void launch_gemv(const ushort_t *x, const ushort_t *w, ushort_t *y, int K,
                 int N, hipStream_t stream);
// w = [gate rows | up rows], 2*F rows; act [F]
void launch_gemv_gateup(const ushort_t *x, const ushort_t *w, ushort_t *act,
                        int K, int F, hipStream_t stream);
void launch_gemv_norm(const ushort_t *x, const ushort_t *wln,
                      const ushort_t *w, ushort_t *y, int K, int N, float eps,
                      hipStream_t stream);
// N == (ra.hq + 2*ra.kh) * ra.hd, hd % 16 == 0, N <= 8192
void launch_gemv_norm_rope_kv(const ushort_t *x, const ushort_t *wln,
                              const ushort_t *w, ushort_t *y, int K,
                              float eps, const RopeKvArgs &ra,
                              hipStream_t stream);
void launch_gemv_res(const ushort_t *x, const ushort_t *w, ushort_t *resid,
                     int K, int N, hipStream_t stream);
void launch_gemv_gateup_norm(const ushort_t *x, const ushort_t *wln,
                             const ushort_t *w, ushort_t *act, int K, int F,
                             float eps, hipStream_t stream);

// ---- gemm.hip, gemm256.hip: c[M, N] = a[M, K] @ b[N, K]^T -----------------
void launch_gemm(const ushort_t *a, const ushort_t *b, ushort_t *c, int M,
                 int N, int K, hipStream_t stream);
void launch_gemm256(const ushort_t *a, const ushort_t *b, ushort_t *c, int M,
                    int N, int K, hipStream_t stream);

// ---- gemm_fp8.hip (128^2, 256^2): e4m3 operands + per-row f32 scales ----
void launch_gemm_fp8(const uint8_t *a, const float *asc, const uint8_t *b,
                     const float *bsc, ushort_t *c, int M, int N, int K,
                     hipStream_t stream);
void launch_gemm_fp8_256(const uint8_t *a, const float *asc, const uint8_t *b,
                         const float *bsc, ushort_t *c, int M, int N, int K,
                         hipStream_t stream);

// ---- gemv_fp8.hip: e4m3 decode GEMVs and activation quantizers ------------
// x [M, K] bf16 -> q [M, K] e4m3, scale [M]
void launch_quant_fp8(const ushort_t *x, uint8_t *q, float *scale, int M,
                      int K, hipStream_t stream);
void launch_quant_norm_fp8(const ushort_t *x, const ushort_t *wln, uint8_t *q,
                           float *scale, int K, float eps,
                           hipStream_t stream);
// pre-quantized x[K] (+ xs[1]) against w[N, K] (+ wsc[N]); K before N
void launch_gemv_fp8(const uint8_t *x, const float *xs, const uint8_t *w,
                     const float *wsc, ushort_t *y, int K, int N,
                     hipStream_t stream);
void launch_gemv_fp8_rope_kv(const uint8_t *x, const float *xs,
                             const uint8_t *w, const float *wsc, ushort_t *y,
                             int K, const RopeKvArgs &ra, hipStream_t stream);
void launch_gemv_fp8_res(const uint8_t *x, const float *xs, const uint8_t *w,
                         const float *wsc, ushort_t *resid, int K, int N,
                         hipStream_t stream);
void launch_gemv_fp8_gateup(const uint8_t *x, const float *xs,
                            const uint8_t *w, const float *wsc, ushort_t *act,
                            int K, int F, hipStream_t stream);
// bf16 x quantized in-kernel (LDS-staged)
void launch_gemv_fp8_norm(const ushort_t *x, const ushort_t *wln,
                          const uint8_t *w, const float *wsc, ushort_t *y,
                          int K, int N, float eps, hipStream_t stream);
void launch_gemv_fp8_resl(const ushort_t *x, const uint8_t *w,
                          const float *wsc, ushort_t *resid, int K, int N,
                          hipStream_t stream);
void launch_gemv_fp8_gateup_norm(const ushort_t *x, const ushort_t *wln,
                                 const uint8_t *w, const float *wsc,
                                 ushort_t *act, int K, int F, float eps,
                                 hipStream_t stream);

// ---- mfma_rate.hip --------------------------------------------------------
void launch_mfma_rate(const ushort_t *seed, float *out, int which, int blocks,
                      hipStream_t stream);

}  // extern "C"
