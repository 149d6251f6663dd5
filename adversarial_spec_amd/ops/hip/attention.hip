// Attention kernels for CDNA4 (gfx950).
//
//  - attn_decode_split / attn_decode_combine: single-token decode over the
//    paged KV cache, flash-decoding style (split-KV online softmax with a
//    combine pass). Memory-bound by the KV read: each KV row is read ONCE
//    per kv-head and serves all `group` GQA query heads; vectorized 16 B
//    per lane; splits spread the read over the whole chip.
//
//  - attn_prefill_simple: correctness-first causal prefill over the fresh
//    contiguous K/V of the prompt (one 16-lane group per query row, online
//    softmax in registers). It is the numerics anchor; the MFMA-tiled
//    prefill (attn_prefill_mfma.hip) replaces it on the hot path.
//
// Layout contracts (ops/torch_ref.py):
//   q        [tq, hq, hd] bf16
//   k,v      [tk, kh, hd] bf16 (contiguous, prefill)
//   kc,vc    [n_pages, page, kh, hd] bf16 (decode)
//   page_table int32
// State is fp32 throughout; hd in {32, 64, 128}; group = hq/kh <= 8.

#include "attn_decode_split.h"
#include "launchers.h"

// 16-lane-group dot reduce (LPP = lanes per position = hd/8)
template <int LPP>
DEVINL float group_reduce_sum(float v) {
#pragma unroll
  for (int off = LPP / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}

// ---------------------------------------------------------------------------
// Decode split kernel, bf16 cache: attn_decode_split_tiles
// (attn_decode_split.h) over this trait. A 16-byte lane chunk is 8 elements
// and a stage buffer is [K | V].
// ---------------------------------------------------------------------------

template <int HD_>
struct KvBf16 {
  static constexpr int HD = HD_, EPL = 8, LPP = HD / EPL;
  static constexpr int TILE_E = DTILE * HD;  // elements per tensor per tile
  static constexpr int BUF_B = 2 * TILE_E * 2;
  static constexpr int LOADS_PER_TILE = LPP / 2;  // LPP/4 K + LPP/4 V pieces
  static constexpr bool SCALED = false;
  const ushort_t *kc, *vc;

  // Each wave issues LPP/4 x 1 KiB pieces for K and for V; a piece covers
  // WAVE/LPP consecutive positions; lane l handles the piece's position
  // l/LPP, chunk l%LPP. The K source chunk is pre-swizzled, V stays linear.
  template <bool IDENT>
  DEVINL void stage_tile(uint8_t *buf, int t0, const SplitWave &w) const {
    ushort_t *kimg = (ushort_t *)buf;
    ushort_t *vimg = kimg + TILE_E;
    const int sub = w.lane / LPP, sl = w.lane % LPP;
#pragma unroll
    for (int i = 0; i < LPP / 4; ++i) {  // pieces per wave per tensor
      const int prow = (w.wid * (LPP / 4) + i) * (WAVE / LPP);  // tile-local
      const int myrow = prow + sub;
      const int pp = min(t0 + myrow, w.seq_len - 1);
      const int phys = phys_page<IDENT>(w, pp);
      const size_t row = ((size_t)phys * w.page + (pp % w.page)) * w.kh * HD +
                         (size_t)w.g * HD;
      glds16(kc + row + (size_t)(sl ^ kswz<LPP>(myrow)) * 8,
             kimg + (size_t)prow * HD);
      glds16(vc + row + sl * 8, vimg + (size_t)prow * HD);
    }
  }

  // Heads outside, chunks inside (the K chunk is re-read per head): all of
  // the work is in qk_head. 4 chunk-residue accumulators cover the
  // dependent v_dot2 latency.
  struct NoPart {};
  template <int NG>
  static DEVINL NoPart qk_chunks(const uint8_t *, const ushort_t *,
                                 const SplitWave &, int) { return {}; }

  static DEVINL float qk_head(NoPart, int gi, const uint8_t *buf,
                              const ushort_t *qlds, const SplitWave &w) {
    const int gq = w.wid + 4 * gi;
    const ushort_t *kimg = (const ushort_t *)buf;
    const int myswz = kswz<LPP>(w.lane);
    float a4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < LPP; ++c) {
      const v8s kv = ((const v8s *)(kimg + (size_t)w.lane * HD))[c];
      const v8s qv = ((const v8s *)(qlds + (size_t)gq * HD))[c ^ myswz];
      a4[c & 3] = dot8_bf16(__builtin_bit_cast(bf16x8, qv),
                            __builtin_bit_cast(bf16x8, kv), a4[c & 3]);
    }
    return (a4[0] + a4[1]) + (a4[2] + a4[3]);
  }

  static DEVINL f32x8 load_v(const uint8_t *buf, int p, int sl) {
    const ushort_t *vimg = (const ushort_t *)buf + TILE_E;
    const v8s vv = ((const v8s *)(vimg + (size_t)p * HD))[sl];
    return unpack8(__builtin_bit_cast(bf16x8, vv));
  }
};

// `hd` stays in the argument list; the skeleton uses LPP * 8, which is the
// only value the launcher passes.
// The hd=32 one-head-per-wave instantiations need 62 VGPRs, two under the
// 8-waves-per-SIMD step, and hipcc's scheduler gives that step up (74 VGPRs,
// 6 waves) over source changes as small as moving the QK loop into a
// function. The second launch bound states the occupancy they run at. It
// also caps them at 64 VGPRs: an edit that needs more spills instead of
// dropping an occupancy step, so check `.private_segment_fixed_size` of
// these four symbols stays 0 whenever the skeleton changes.
template <int LPP, int MG, bool IDENT>
__global__ void __launch_bounds__(256, (LPP == 4 && MG <= 4) ? 8 : 1)
attn_decode_split_kernel(
    const ushort_t *__restrict__ q,   // [hq, hd]
    const ushort_t *__restrict__ kc, const ushort_t *__restrict__ vc,
    const int *__restrict__ page_table, int seq_len, float scale,
    int kh, int group, int hd, int page, int split_len, int window,
    float *__restrict__ ws_m, float *__restrict__ ws_l,
    float *__restrict__ ws_acc, const int *__restrict__ pos_ptr,
    ushort_t *__restrict__ out) {
  attn_decode_split_tiles<KvBf16<LPP * 8>, MG, IDENT>(
      {kc, vc}, q, page_table, seq_len, scale, kh, group, page, split_len,
      window, ws_m, ws_l, ws_acc, pos_ptr, out);
}


// ---------------------------------------------------------------------------
// Decode combine kernel: grid = (hq, hd/64), block = 256 (4 waves).
// out[h, :] = sum_splits(acc * exp(m - M)) / L_total
// A SEPARATE kernel on purpose: a fused last-block-arrives combine needs
// device-scope fences, which on the 8-XCD MI355X triggered cross-L2 traffic
// that slowed the whole device ~5x (round-1 profiles).
// Parallel walk: wave w strides splits w, w+4, ...; lane = dim. The old
// 1-thread-per-(head,dim) single-block walk measured 10.5 us at 54 splits
// (62% wave-parked) — as costly as the split pass itself.
// ---------------------------------------------------------------------------

// The combine's rescale-accumulate step with its roundings spelled out.
// Written as `L += l * sc; A += a * sc`, hipcc's fp contraction depended on
// the surrounding code: the unrolled rounds of 4 multiplied and added L in
// two roundings (packed multiply, scalar adds) and fused A, the ragged loop
// fused both. These helpers pin exactly that, so every walk over the splits
// below produces the same bits whatever the compiler makes of its shape.
DEVINL void combine_step_round(float &L, float &A, float l, float a,
                               float sc) {
  {
#pragma clang fp contract(off)
    L = L + l * sc;
  }
  A = __builtin_fmaf(a, sc, A);
}

DEVINL void combine_step_ragged(float &L, float &A, float l, float a,
                                float sc) {
  L = __builtin_fmaf(l, sc, L);
  A = __builtin_fmaf(a, sc, A);
}

extern "C" __global__ void __launch_bounds__(256)
attn_decode_combine_kernel(const float *__restrict__ ws_m,
                           const float *__restrict__ ws_l,
                           const float *__restrict__ ws_acc,
                           ushort_t *__restrict__ out, int n_splits,
                           int group, int hd) {
  const int h = blockIdx.x;
  const int g = h / group, gi = h % group;
  const int dd = blockIdx.y * 64 + (threadIdx.x & (WAVE - 1));
  const int sg = threadIdx.x / WAVE;  // split stride group: 0..3
  if (dd >= hd) return;

  __shared__ float red[4];
  __shared__ float redL[4];

  float L = 0.f, Au[4] = {0.f, 0.f, 0.f, 0.f};
  if (n_splits <= 64) {
    // ONE memory round trip: this wave's <= 16 splits (s = sg + 4*j) have
    // all of their m, l and acc words issued up front, so the kernel pays
    // the cross-XCD latency once instead of once per pass (pass 2's loads
    // used to wait behind the barrier that publishes M). Loads are
    // unconditional on a clamped split index — a per-element "load or
    // constant" select makes hipcc branch around every load and drain
    // vmcnt per element; validity is applied to the arithmetic only.
    // Arithmetic and accumulation order are those of the two-pass walk
    // below (full rounds of 4 -> Au[u], the ragged last round -> Au[0], L
    // in split order, the same combine_step_* roundings), so the output is
    // bit-identical to it.
    float mw[16], lw[16], aw[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int sc = min(sg + 4 * j, n_splits - 1);
      const size_t b = ((size_t)g * n_splits + sc) * group + gi;
      mw[j] = ws_m[b];
      lw[j] = ws_l[b];
      aw[j] = ws_acc[b * hd + dd];
    }
    float m4[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (sg + 4 * j < n_splits) m4[j & 3] = fmaxf(m4[j & 3], mw[j]);
    const float m = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
    if ((threadIdx.x & (WAVE - 1)) == 0) red[sg] = m;
    __syncthreads();
    const float M = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (sg + 16 * r + 12 < n_splits) {  // wave-uniform: a full round
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int j = 4 * r + u;
          const float sc = (mw[j] == -INFINITY) ? 0.f : exp2f(mw[j] - M);
          combine_step_round(L, Au[u], lw[j], aw[j], sc);
        }
      } else {  // the ragged last round (and the empty ones after it)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int j = 4 * r + u;
          if (sg + 4 * j < n_splits) {
            const float sc = (mw[j] == -INFINITY) ? 0.f : exp2f(mw[j] - M);
            combine_step_ragged(L, Au[0], lw[j], aw[j], sc);
          }
        }
      }
    }
  } else {
    // pass 1: global max over this wave's split stride (4 independent max
    // chains — a serial walk exposed full cross-XCD latency per entry)
    float m = -INFINITY;
    {
      float m4[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      int s = sg;
      for (; s + 12 < n_splits; s += 16) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
          m4[u] = fmaxf(m4[u],
                        ws_m[((size_t)g * n_splits + s + 4 * u) * group + gi]);
      }
      for (; s < n_splits; s += 4)
        m4[0] = fmaxf(m4[0], ws_m[((size_t)g * n_splits + s) * group + gi]);
      m = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) red[sg] = m;
    __syncthreads();
    const float M = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));

    // pass 2: strided L/acc accumulation, 4 independent accumulators per
    // wave (16 concurrent loads across the block) — the ws round-trip is
    // cross-XCD latency-bound, so ILP depth is the lever
    // ws_m holds the split kernel's LOG2-SCALED running max (m2 domain):
    // rescale factors are exp2, not exp
    int s = sg;
    for (; s + 12 < n_splits; s += 16) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const size_t b = ((size_t)g * n_splits + s + 4 * u) * group + gi;
        const float mw = ws_m[b];
        const float sc = (mw == -INFINITY) ? 0.f : exp2f(mw - M);
        combine_step_round(L, Au[u], ws_l[b], ws_acc[b * hd + dd], sc);
      }
    }
    for (; s < n_splits; s += 4) {
      const size_t b = ((size_t)g * n_splits + s) * group + gi;
      const float mw = ws_m[b];
      const float sc = (mw == -INFINITY) ? 0.f : exp2f(mw - M);
      combine_step_ragged(L, Au[0], ws_l[b], ws_acc[b * hd + dd], sc);
    }
  }
  float A = (Au[0] + Au[1]) + (Au[2] + Au[3]);

  // merge the 4 waves: A via LDS columns, L via lane-0 scalars
  __shared__ float accs[4][64];
  accs[sg][threadIdx.x & (WAVE - 1)] = A;
  if ((threadIdx.x & (WAVE - 1)) == 0) redL[sg] = L;
  __syncthreads();
  if (sg == 0) {
    A = accs[0][threadIdx.x] + accs[1][threadIdx.x] + accs[2][threadIdx.x] +
        accs[3][threadIdx.x];
    L = redL[0] + redL[1] + redL[2] + redL[3];
    out[(size_t)h * hd + dd] = f32_to_bf16(L > 0.f ? A / L : 0.f);
  }
}

// ---------------------------------------------------------------------------
// Correctness-first causal prefill.
// grid.x = hq, grid.y = ceil(tq / rows_per_block), block = 256 (4 waves).
// Each 16-lane (LPP-lane) group owns ONE query row and walks keys 0..row, or
// with a sliding window (window = W >= 1, causal only) keys row-W+1..row.
// ---------------------------------------------------------------------------

template <int LPP>
__global__ void __launch_bounds__(256) attn_prefill_simple_kernel(
    const ushort_t *__restrict__ q, const ushort_t *__restrict__ k,
    const ushort_t *__restrict__ v, ushort_t *__restrict__ out,
    int tq, int tk, int kv_offset, float scale, int hq, int kh, int hd,
    int causal, int window) {
  const int h = blockIdx.x;
  const int g = h / (hq / kh);
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int sub = lane / LPP, sl = lane % LPP;
  const int rows_per_block = 4 * (WAVE / LPP);
  const int row = blockIdx.y * rows_per_block + wid * (WAVE / LPP) + sub;
  if (row >= tq) return;

  const int limit = causal ? min(tk, kv_offset + row + 1) : tk;
  const int first = window ? max(0, kv_offset + row - window + 1) : 0;

  float qf[8];
  {
    const f32x8 qd =
        unpack8(((const bf16x8 *)(q + ((size_t)row * hq + h) * hd))[sl]);
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[j] = qd.v[j];
  }

  float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;

  for (int p = first; p < limit; ++p) {
    const size_t kr = ((size_t)p * kh + g) * hd;
    const f32x8 kd = unpack8(((const bf16x8 *)(k + kr))[sl]);
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) dot += qf[j] * kd.v[j];
    const float s = group_reduce_sum<LPP>(dot) * scale;
    const f32x8 vd = unpack8(((const bf16x8 *)(v + kr))[sl]);
    const float mn = fmaxf(m, s);
    const float alpha = __expf(m - mn);
    const float pex = __expf(s - mn);
    l = l * alpha + pex;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = acc[j] * alpha + pex * vd.v[j];
    m = mn;
  }

  const float inv = (l > 0.f) ? 1.0f / l : 0.f;
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o.u[j] = f32_to_bf16(acc[j] * inv);
  ((bf16x8 *)(out + ((size_t)row * hq + h) * hd))[sl] = o;
}

// ---------------------------------------------------------------------------
// C-linkage launch wrappers (templated LPP dispatch)
// ---------------------------------------------------------------------------

// One block per (q head, 64-wide slice of hd); the only place this grid rule
// is written: the bf16 split launcher below and the fp8 one (kv_fp8.hip)
// both come through here.
extern "C" void launch_attn_decode_combine(const float *ws_m,
                                           const float *ws_l,
                                           const float *ws_acc, ushort_t *out,
                                           int n_splits, int kh, int group,
                                           int hd, hipStream_t stream) {
  attn_decode_combine_kernel<<<dim3(kh * group, (hd + 63) / 64), 256, 0,
                               stream>>>(ws_m, ws_l, ws_acc, out, n_splits,
                                         group, hd);
}

extern "C" void launch_attn_decode_split(const ushort_t *q, const ushort_t *kc,
                                         const ushort_t *vc,
                                         const DecodeSplitArgs &a,
                                         ushort_t *out, hipStream_t stream) {
  const dim3 grid(a.kh, a.n_splits);
  dispatch_decode_split(a.hd, a.group, a.identity, [&](auto HD, auto MG,
                                                       auto IDENT) {
    attn_decode_split_kernel<decltype(HD)::value / 8, decltype(MG)::value,
                             decltype(IDENT)::value>
        <<<grid, 256, 0, stream>>>(  // all LDS is static in the kernel
            q, kc, vc, a.page_table, a.seq_len, a.scale, a.kh, a.group, a.hd,
            a.page, a.split_len, a.window, a.ws_m, a.ws_l, a.ws_acc,
            a.pos_ptr, out);
  });
  if (a.n_splits > 1) {
    launch_attn_decode_combine(a.ws_m, a.ws_l, a.ws_acc, out, a.n_splits,
                               a.kh, a.group, a.hd, stream);
  }
}

extern "C" void launch_attn_prefill_simple(
    const ushort_t *q, const ushort_t *k, const ushort_t *v, ushort_t *out,
    int tq, int tk, int kv_offset, float scale, int hq, int kh, int hd,
    int causal, int window, hipStream_t stream) {
  const int lpp = hd / 8;
  const int rows_per_block = 4 * (WAVE / lpp);
  dim3 grid(hq, (tq + rows_per_block - 1) / rows_per_block);
  switch (lpp) {
    case 4:
      attn_prefill_simple_kernel<4><<<grid, 256, 0, stream>>>(
          q, k, v, out, tq, tk, kv_offset, scale, hq, kh, hd, causal, window);
      break;
    case 8:
      attn_prefill_simple_kernel<8><<<grid, 256, 0, stream>>>(
          q, k, v, out, tq, tk, kv_offset, scale, hq, kh, hd, causal, window);
      break;
    case 16:
      attn_prefill_simple_kernel<16><<<grid, 256, 0, stream>>>(
          q, k, v, out, tq, tk, kv_offset, scale, hq, kh, hd, causal, window);
      break;
  }
}
