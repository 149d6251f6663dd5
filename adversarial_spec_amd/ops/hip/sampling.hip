// On-device sampling: fused temperature scale + softmax + inverse-CDF draw
// (and greedy argmax), one block over the vocab row.
//
// Decode emits one token at a time; sampling on-device avoids a logits
// round-trip (vocab 128256 x 2 B per step) — only a 4-byte token id ever
// reaches the host, and only every N tokens (engine/local.py async loop).
// The random draw is a counter-based hash of the host-provided seed, so
// replays (HIP graphs) stay deterministic.
//
// All passes read the logits as bf16x8 (16 B/lane): the row was just
// written by the lm_head GEMV so it is L2-resident; vectorized reads keep
// the single-workgroup scan latency-bound rather than issue-bound.
//
// sample_body is the default temperature / greedy path (reference defaults
// 0.7 / 0.3: models.py:626). Truncated sampling (top-p < 1, top-k > 0) is
// sample_filtered_body further down: a histogram selection over the 65 536
// possible bf16 values finds the cut without a sort, still in one block.

#include "common.h"
#include "launchers.h"

// logits: [vocab] bf16, vocab % 8 == 0. temp <= 0 -> greedy. Returns the
// sampled id in *out; shared body for the plain and graph-state kernels.
//
// Softmax sampling via the GUMBEL-MAX trick: argmax_i(logit_i/T + g_i) with
// g_i = -log(-log(u_i)) is an exact draw from softmax(logits/T). That
// collapses the old 3-pass (max, Z, CDF-scan) sampler into ONE pass over
// the vocab — the decode step's tail latency (the lm_head logits row is
// L2-resident when this runs). Per-element RNG is a counter-based hash of
// (seed, index), so HIP-graph replays stay deterministic for a given seed.
DEVINL void sample_body(const ushort_t *__restrict__ logits, int vocab,
                        float temp, uint32_t seed, int *__restrict__ out) {
  const int tid = threadIdx.x;
  const int nvec = vocab / 8;
  const bf16x8 *lv = (const bf16x8 *)logits;
  const bool greedy = temp <= 0.f;
  const float inv_t = greedy ? 1.0f : 1.0f / temp;

  float best = -INFINITY;
  int besti = 0;
  for (int i = tid; i < nvec; i += blockDim.x) {
    const f32x8 v = unpack8(lv[i]);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int idx = i * 8 + j;
      float val = v.v[j] * inv_t;
      if (!greedy) {
        const uint32_t h = hash_u32(seed ^ ((uint32_t)idx * 2654435761u));
        const float u = ((float)h + 1.0f) * 2.3283064e-10f;  // (0, 1]
        val -= __logf(-__logf(u) + 1e-30f);  // + Gumbel(0,1)
      }
      if (val > best || (val == best && idx < besti)) { best = val; besti = idx; }
    }
  }
  // wave argmax reduce (ties -> lowest index, replay-deterministic)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(best, off, WAVE);
    const int oi = __shfl_xor(besti, off, WAVE);
    if (ov > best || (ov == best && oi < besti)) { best = ov; besti = oi; }
  }
  __shared__ float mv[16];
  __shared__ int mi[16];
  const int wid = tid / WAVE;
  if ((tid & (WAVE - 1)) == 0) { mv[wid] = best; mi[wid] = besti; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < (int)(blockDim.x / WAVE); ++w) {
      if (mv[w] > best || (mv[w] == best && mi[w] < besti)) {
        best = mv[w]; besti = mi[w];
      }
    }
    *out = besti;
  }
}

extern "C" __global__ void __launch_bounds__(1024)
sample_kernel(const ushort_t *__restrict__ logits, int vocab, float temp,
              uint32_t seed, int *__restrict__ out) {
  sample_body(logits, vocab, temp, seed, out);
}

// HIP-graph decode variant: the RNG seed, step index, TEMPERATURE and token
// outputs all live in device words so one captured graph replays per token
// and serves every request temperature (the graph cache key must not
// include temperature — ADVICE round 1).
//   temp_state: f32[1], sampling temperature (<= 0 -> greedy)
//   rng_state:  uint32[1], advanced each call
//   step_state: int32[1], the decode step index (bumped by bump_kernel)
//   tok_hist:   int32[max_new] history the host polls every N tokens
//   tok_long:   int64[1] embedding index for the next forward — written
//               directly so the decode step drops the int32->int64 copy
//               launch torch would otherwise add per token
extern "C" __global__ void __launch_bounds__(1024)
sample_state_kernel(const ushort_t *__restrict__ logits, int vocab,
                    const float *__restrict__ temp_state,
                    uint32_t *__restrict__ rng_state,
                    int *__restrict__ tok_hist,
                    const int *__restrict__ step_state,
                    long long *__restrict__ tok_long) {
  __shared__ int picked[1];
  const uint32_t seed = *rng_state;
  sample_body(logits, vocab, *temp_state, seed, picked);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int tok = picked[0];
    tok_long[0] = (long long)tok;
    tok_hist[*step_state] = tok;
    *rng_state = hash_u32(seed ^ 0x6a09e667u) | 1u;  // never 0
  }
}

// pos/step bump — the single tail kernel of the captured decode step.
extern "C" __global__ void bump_kernel(int *__restrict__ pos_state,
                                       int *__restrict__ step_state) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    pos_state[0] += 1;
    step_state[0] += 1;
  }
}

// ---------------------------------------------------------------------------
// C-linkage launch wrappers. The samplers are single-block: sample_body
// reduces the whole vocab inside one 1024-thread block.
// ---------------------------------------------------------------------------

extern "C" void launch_sample(const ushort_t *logits, int vocab, float temp,
                              uint32_t seed, int *out, hipStream_t stream) {
  sample_kernel<<<1, 1024, 0, stream>>>(logits, vocab, temp, seed, out);
}

extern "C" void launch_sample_state(const ushort_t *logits, int vocab,
                                    const float *temp_state,
                                    uint32_t *rng_state, int *tok_hist,
                                    const int *step_state, long long *tok_long,
                                    hipStream_t stream) {
  sample_state_kernel<<<1, 1024, 0, stream>>>(logits, vocab, temp_state,
                                              rng_state, tok_hist, step_state,
                                              tok_long);
}

extern "C" void launch_bump(int *pos_state, int *step_state,
                            hipStream_t stream) {
  bump_kernel<<<1, 64, 0, stream>>>(pos_state, step_state);
}

// ---------------------------------------------------------------------------
// Filtered sampling: top-p (nucleus) and top-k, on device, capture-safe.
//
// Contract (ops/torch_ref.py nucleus_keep is the float64 statement of it):
// with p = softmax(logits / T), G(i) the total probability of the tokens
// whose logit is STRICTLY greater than token i's and C(i) their number,
// token i is kept iff G(i) < top_p and (top_k == 0 or C(i) < top_k). Equal
// logits (+0.0 and -0.0 included) are one group and are kept or dropped
// together, so the kept set is {i : logit_i >= cut}; the argmax group is
// always kept. The draw is Gumbel-max over the kept set, which is an exact
// draw from p renormalised over it.
//
// A bf16 logit maps to a 16-bit key that orders as the value does, so the
// cut is a key. Counts per key are histogrammed in LDS with integer atomics
// (order-independent); group masses are count * w(key), summed over keys in
// descending order by a fixed-shape scan. No floating-point atomics: the
// same row, T, top_p, top_k and seed give the same token on every launch.
// The histogram covers a window of NUC_W keys below the row maximum; the
// cut of a truncating setting lies in the first window, and a second pass
// over the (L2-resident) row covers the rest of the key space when it does
// not. Logits are expected finite (-inf is fine: weight 0); a NaN or +inf
// maximum degrades to "keep the maximum group".
// ---------------------------------------------------------------------------

#define NUC_THREADS 1024
#define NUC_W 32768                       // keys per histogram window (128 KB)
#define NUC_BPT (NUC_W / NUC_THREADS)     // window bins scanned per thread

// bf16 bits -> key with key(a) < key(b) <=> a < b; -0.0 joins +0.0
DEVINL uint32_t nuc_key(ushort_t b) {
  uint32_t u = b;
  if (u == 0x8000u) u = 0u;
  return (u & 0x8000u) ? (~u & 0xffffu) : (u | 0x8000u);
}

DEVINL float nuc_val(uint32_t key) {
  return bf16_to_f32((ushort_t)((key & 0x8000u) ? (key ^ 0x8000u)
                                                : (0xffffu - key)));
}

// unnormalised softmax weight of a key; one expression for the row sum and
// for the group masses, so a key has one weight everywhere
DEVINL float nuc_w(uint32_t key, float xmax, float inv_t) {
  return __expf((nuc_val(key) - xmax) * inv_t);
}

// Lowest kept key of the row; every thread returns it. blockDim.x must be
// NUC_THREADS. temp <= 0 (greedy) keeps the maximum group only; top_p >= 1
// with top_k <= 0 keeps everything (key 0).
DEVINL uint32_t nucleus_cut(const ushort_t *__restrict__ logits, int vocab,
                            float temp, float top_p, int top_k) {
  __shared__ __attribute__((aligned(16))) uint32_t hist[NUC_W];
  __shared__ uint32_t red_u[16];
  __shared__ float red_f[16];
  __shared__ int red_last[16];
  __shared__ int red_rej[16];
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid / WAVE;
  const int nvec = vocab / 8;
  const bf16x8 *lv = (const bf16x8 *)logits;

  // pass 1: the row maximum, as a key (integer max: exact, any order)
  uint32_t mk = 0;
  for (int i = tid; i < nvec; i += NUC_THREADS) {
    const bf16x8 p = lv[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) mk = max(mk, nuc_key(p.u[j]));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    mk = max(mk, (uint32_t)__shfl_xor((int)mk, off, WAVE));
  if (lane == 0) red_u[wid] = mk;
  __syncthreads();
  mk = 0;
#pragma unroll
  for (int w = 0; w < NUC_THREADS / WAVE; ++w) mk = max(mk, red_u[w]);
  __syncthreads();
  if (temp <= 0.f) return mk;
  if (top_p >= 1.f && top_k <= 0) return 0u;

  const float xmax = nuc_val(mk);
  const float inv_t = 1.0f / temp;
  uint32_t cut = mk;          // the maximum group is kept whatever follows
  int hi = (int)mk;           // top key of the current window
  float z = 0.f;              // sum of all weights (first window's pass)
  float mass_above = 0.f;     // weight of the keys above the window
  uint32_t count_above = 0;   // and their number

  for (int win = 0;; ++win) {
    uint4 *h4 = (uint4 *)hist;
    for (int q = tid; q < NUC_W / 4; q += NUC_THREADS)
      h4[q] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();

    // pass 2: count the keys in (hi - NUC_W, hi]; bin = hi - key
    float zacc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int i = tid; i < nvec; i += NUC_THREADS) {
      const bf16x8 p = lv[i];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint32_t k = nuc_key(p.u[j]);
        const uint32_t b = (uint32_t)(hi - (int)k);
        if (b < (uint32_t)NUC_W) atomicAdd(&hist[b], 1u);
        if (win == 0) zacc[j] += nuc_w(k, xmax, inv_t);
      }
    }
    if (win == 0) {
      // 8 chains of <= vocab/8192 terms per thread, then a fixed tree
      const float zt = ((zacc[0] + zacc[1]) + (zacc[2] + zacc[3])) +
                       ((zacc[4] + zacc[5]) + (zacc[6] + zacc[7]));
      z = block_reduce_sum(zt, red_f);
    } else {
      __syncthreads();
    }

    // per-thread mass and count of NUC_BPT consecutive bins (descending
    // keys), then an exclusive scan over threads in thread order
    const int b0 = tid * NUC_BPT;
    float m = 0.f;
    uint32_t c = 0;
#pragma unroll 4
    for (int j = 0; j < NUC_BPT; ++j) {
      const uint32_t cj = hist[b0 + j];
      if (cj) {
        m += (float)cj * nuc_w((uint32_t)(hi - (b0 + j)), xmax, inv_t);
        c += cj;
      }
    }
    float im = m;
    uint32_t ic = c;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
      const float om = __shfl_up(im, off, WAVE);
      const uint32_t oc = (uint32_t)__shfl_up((int)ic, off, WAVE);
      if (lane >= off) { im += om; ic += oc; }
    }
    float em = __shfl_up(im, 1, WAVE);
    uint32_t ec = (uint32_t)__shfl_up((int)ic, 1, WAVE);
    if (lane == 0) { em = 0.f; ec = 0; }
    if (lane == WAVE - 1) { red_f[wid] = im; red_u[wid] = ic; }
    __syncthreads();
    float pm = 0.f, tm = 0.f;
    uint32_t pc = 0, tc = 0;
#pragma unroll
    for (int w = 0; w < NUC_THREADS / WAVE; ++w) {
      if (w < wid) { pm += red_f[w]; pc += red_u[w]; }
      tm += red_f[w];
      tc += red_u[w];
    }

    // walk the bins again with G and C, the mass and count strictly above
    float g = mass_above + (pm + em);
    uint32_t cnt = count_above + pc + ec;
    const float lim = top_p * z;
    int last = -1, rej = 0;
#pragma unroll 4
    for (int j = 0; j < NUC_BPT; ++j) {
      const uint32_t cj = hist[b0 + j];
      if (cj) {
        const bool keep = (top_p >= 1.f || g < lim) &&
                          (top_k <= 0 || cnt < (uint32_t)top_k);
        if (keep) last = b0 + j; else rej = 1;
        g += (float)cj * nuc_w((uint32_t)(hi - (b0 + j)), xmax, inv_t);
        cnt += cj;
      }
    }
    // lowest kept key = highest kept bin; taking the maximum makes the kept
    // set a threshold set by construction
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      last = max(last, __shfl_xor(last, off, WAVE));
      rej |= __shfl_xor(rej, off, WAVE);
    }
    if (lane == 0) { red_last[wid] = last; red_rej[wid] = rej; }
    __syncthreads();
    last = -1;
    rej = 0;
#pragma unroll
    for (int w = 0; w < NUC_THREADS / WAVE; ++w) {
      last = max(last, red_last[w]);
      rej |= red_rej[w];
    }
    if (last >= 0) cut = (uint32_t)(hi - last);
    mass_above += tm;
    count_above += tc;
    // done: a group was dropped, or every token is counted, or the window
    // reached key 0 (all block-uniform, so every thread leaves together)
    if (rej || count_above >= (uint32_t)vocab || hi < NUC_W) break;
    hi -= NUC_W;
  }
  return cut;
}

// Greedy (temp <= 0) is the argmax with ties to the lowest index, as in
// sample_body. Otherwise Gumbel-max over the kept keys. The uniform is
// ((h >> 9) + 0.5) * 2^-23: 23 random bits plus the half fit a float's 24
// exactly, so u lies in [2^-24, 1 - 2^-24] and both logarithms are finite
// without an epsilon (24 bits plus the half would round up to u == 1).
DEVINL void sample_filtered_body(const ushort_t *__restrict__ logits,
                                 int vocab, float temp, float top_p, int top_k,
                                 uint32_t seed, int *__restrict__ out) {
  const int tid = threadIdx.x;
  const int nvec = vocab / 8;
  const bf16x8 *lv = (const bf16x8 *)logits;
  const bool greedy = temp <= 0.f;
  const float inv_t = greedy ? 1.0f : 1.0f / temp;
  const uint32_t cut =
      greedy ? 0u : nucleus_cut(logits, vocab, temp, top_p, top_k);

  float best = -INFINITY;
  int besti = 0;
  for (int i = tid; i < nvec; i += NUC_THREADS) {
    const bf16x8 p = lv[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (nuc_key(p.u[j]) < cut) continue;
      const int idx = i * 8 + j;
      float val = bf16_to_f32(p.u[j]) * inv_t;
      if (!greedy) {
        const uint32_t h = hash_u32(seed ^ ((uint32_t)idx * 2654435761u));
        const float u = ((float)(h >> 9) + 0.5f) * 1.1920929e-7f;  // 2^-23
        val -= __logf(-__logf(u));  // + Gumbel(0,1)
      }
      if (val > best || (val == best && idx < besti)) { best = val; besti = idx; }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(best, off, WAVE);
    const int oi = __shfl_xor(besti, off, WAVE);
    if (ov > best || (ov == best && oi < besti)) { best = ov; besti = oi; }
  }
  __shared__ float fv[16];
  __shared__ int fi[16];
  const int wid = tid / WAVE;
  if ((tid & (WAVE - 1)) == 0) { fv[wid] = best; fi[wid] = besti; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < NUC_THREADS / WAVE; ++w) {
      if (fv[w] > best || (fv[w] == best && fi[w] < besti)) {
        best = fv[w]; besti = fi[w];
      }
    }
    *out = besti;
  }
}

extern "C" __global__ void __launch_bounds__(NUC_THREADS)
sample_filtered_kernel(const ushort_t *__restrict__ logits, int vocab,
                       float temp, float top_p, int top_k, uint32_t seed,
                       int *__restrict__ out) {
  sample_filtered_body(logits, vocab, temp, top_p, top_k, seed, out);
}

// Graph-state variant: as sample_state_kernel, with top_p (f32[1]) and
// top_k (int32[1]) in device words as well, so one captured graph serves
// every filtered setting.
extern "C" __global__ void __launch_bounds__(NUC_THREADS)
sample_state_filtered_kernel(const ushort_t *__restrict__ logits, int vocab,
                             const float *__restrict__ temp_state,
                             const float *__restrict__ top_p_state,
                             const int *__restrict__ top_k_state,
                             uint32_t *__restrict__ rng_state,
                             int *__restrict__ tok_hist,
                             const int *__restrict__ step_state,
                             long long *__restrict__ tok_long) {
  __shared__ int picked[1];
  const uint32_t seed = *rng_state;
  sample_filtered_body(logits, vocab, *temp_state, *top_p_state, *top_k_state,
                       seed, picked);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int tok = picked[0];
    tok_long[0] = (long long)tok;
    tok_hist[*step_state] = tok;
    *rng_state = hash_u32(seed ^ 0x6a09e667u) | 1u;  // never 0
  }
}

// The kept set as bytes (1 = kept), from the samplers' own nucleus_cut.
// mask: [vocab] uint8, 8-byte aligned.
extern "C" __global__ void __launch_bounds__(NUC_THREADS)
nucleus_mask_kernel(const ushort_t *__restrict__ logits, int vocab, float temp,
                    float top_p, int top_k, uint8_t *__restrict__ mask) {
  const uint32_t cut = nucleus_cut(logits, vocab, temp, top_p, top_k);
  const int nvec = vocab / 8;
  const bf16x8 *lv = (const bf16x8 *)logits;
  unsigned long long *mv = (unsigned long long *)mask;
  for (int i = threadIdx.x; i < nvec; i += NUC_THREADS) {
    const bf16x8 p = lv[i];
    unsigned long long bits = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      bits |= (unsigned long long)(nuc_key(p.u[j]) >= cut) << (8 * j);
    mv[i] = bits;
  }
}

extern "C" void launch_sample_filtered(const ushort_t *logits, int vocab,
                                       float temp, float top_p, int top_k,
                                       uint32_t seed, int *out,
                                       hipStream_t stream) {
  sample_filtered_kernel<<<1, NUC_THREADS, 0, stream>>>(logits, vocab, temp,
                                                        top_p, top_k, seed, out);
}

extern "C" void launch_sample_state_filtered(
    const ushort_t *logits, int vocab, const float *temp_state,
    const float *top_p_state, const int *top_k_state, uint32_t *rng_state,
    int *tok_hist, const int *step_state, long long *tok_long,
    hipStream_t stream) {
  sample_state_filtered_kernel<<<1, NUC_THREADS, 0, stream>>>(
      logits, vocab, temp_state, top_p_state, top_k_state, rng_state, tok_hist,
      step_state, tok_long);
}

extern "C" void launch_nucleus_mask(const ushort_t *logits, int vocab,
                                    float temp, float top_p, int top_k,
                                    uint8_t *mask, hipStream_t stream) {
  nucleus_mask_kernel<<<1, NUC_THREADS, 0, stream>>>(logits, vocab, temp, top_p,
                                                     top_k, mask);
}
