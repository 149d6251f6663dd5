// fp8 (OCP e4m3fn) KV cache for CDNA4 (gfx950): append, decode, dequant.
//
// Storage contract (ops/torch_ref.py):
//   kc, vc     [n_pages, page, kh, hd] uint8, e4m3fn
//   ksc, vsc   [n_pages, kh, page] f32 — head-major inside a page, so the
//              64 scales of one decode tile of one head are contiguous
//   one scale per (position, kv-head) row of hd elements:
//     scale = max(amax|x|, 1e-12) / 448;  q = e4m3fn_rne(x / scale)
//   K is quantized AFTER RoPE, from the bf16-rounded rotated values (the
//   bits rope_kv writes to a bf16 cache).
//
//  - rope_kv_fp8_kernel: fp8 twin of rope_kv_kernel (elementwise.hip).
//  - attn_decode_split_fp8_kernel: fp8 twin of the decode split kernel
//    (attn_decode_split.h) with the dequantization folded into the softmax;
//    it writes the same workspace and is followed by the same
//    attn_decode_combine_kernel.
//  - kv_dequant_fp8_kernel: gathers positions [0, n) into contiguous bf16
//    (chunked prefill only).
// hd in {32, 64, 128}; group = hq/kh <= 8.

#include "attn_decode_split.h"
#include "launchers.h"

typedef float f32x2v __attribute__((ext_vector_type(2)));

#define E4M3_MAX 448.0f

// Two floats -> two e4m3fn bytes (low half of the result) by the hardware
// packed convert: round-to-nearest-even, OCP encoding on gfx950. The clamp
// keeps a quotient that rounded a hair above 448 on the finite side.
// (ops/torch_ref.py quantize_kv_fp8 is the same rule, zero bytes included.)
DEVINL uint32_t quant_pair_e4m3(float a, float b, float scale) {
  float ya = a / scale, yb = b / scale;
  ya = fminf(fmaxf(ya, -E4M3_MAX), E4M3_MAX);
  yb = fminf(fmaxf(yb, -E4M3_MAX), E4M3_MAX);
  uint32_t r =
      (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(ya, yb, 0, false) & 0xffffu;
  // a quantized zero is always byte 0x00: RoPE leaves -0.0 in an all-zero
  // row, and the contract promises zero bytes for it
  if ((r & 0x007fu) == 0) r &= 0xff00u;
  if ((r & 0x7f00u) == 0) r &= 0x00ffu;
  return r;
}

// ---------------------------------------------------------------------------
// Fused RoPE + quantizing paged KV append. Waves map over t * (hq + 2*hk)
// slots exactly as in rope_kv_kernel:
//     slot < hq:            rotate q in place
//     hq <= slot < hq+hk:   rotate k in place, quantize the rotated row
//     slot >= hq+hk:        quantize the v row
// hd <= 128, so a row is at most 64 (even, odd) pairs: ONE pair per lane,
// the row amax is one wave reduction and each lane stores its two bytes.
// ---------------------------------------------------------------------------

extern "C" __global__ void __launch_bounds__(256)
rope_kv_fp8_kernel(ushort_t *__restrict__ q, ushort_t *__restrict__ k,
                   const ushort_t *__restrict__ v,
                   const float *__restrict__ cost,
                   const float *__restrict__ sint, uint8_t *__restrict__ kc,
                   uint8_t *__restrict__ vc, float *__restrict__ ksc,
                   float *__restrict__ vsc,
                   const int *__restrict__ page_table, int t, int hq, int hk,
                   int hd, int pos0, long q_rstride, long k_rstride,
                   long v_rstride, int page,
                   const int *__restrict__ pos_ptr) {
  if (pos_ptr) pos0 = *pos_ptr;
  const int wave_id = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int slots = hq + 2 * hk;
  const int tok = wave_id / slots;
  if (tok >= t) return;
  const int slot = wave_id % slots;
  const int pos = pos0 + tok;
  const int half = hd / 2;
  const float *crow = cost + (size_t)pos * half;
  const float *srow = sint + (size_t)pos * half;

  if (slot < hq) {  // q: rotation only
    uint32_t *base = (uint32_t *)(q + (size_t)tok * q_rstride +
                                  (size_t)slot * hd);
    if (lane < half) {
      const uint32_t pair = base[lane];  // 2 bf16: (even, odd)
      base[lane] = rope_rotate_pair(bf16_to_f32((ushort_t)(pair & 0xffffu)),
                                    bf16_to_f32((ushort_t)(pair >> 16)),
                                    crow[lane], srow[lane]);
    }
    return;
  }

  const bool is_k = slot < hq + hk;
  const int head = is_k ? slot - hq : slot - hq - hk;
  uint32_t pair = 0;  // idle lanes (lane >= half) carry zeros into the amax
  if (lane < half) {
    if (is_k) {
      uint32_t *base = (uint32_t *)(k + (size_t)tok * k_rstride +
                                    (size_t)head * hd);
      const uint32_t raw = base[lane];
      pair = rope_rotate_pair(bf16_to_f32((ushort_t)(raw & 0xffffu)),
                              bf16_to_f32((ushort_t)(raw >> 16)), crow[lane],
                              srow[lane]);
      base[lane] = pair;
    } else {
      pair = ((const uint32_t *)(v + (size_t)tok * v_rstride +
                                 (size_t)head * hd))[lane];
    }
  }
  const float ev = bf16_to_f32((ushort_t)(pair & 0xffffu));
  const float od = bf16_to_f32((ushort_t)(pair >> 16));
  const float amax = wave_reduce_max(fmaxf(fabsf(ev), fabsf(od)));
  const float scale = fmaxf(amax, 1e-12f) / E4M3_MAX;

  const int phys = page_table[pos / page];
  const int inpage = pos % page;
  uint8_t *dst = (is_k ? kc : vc) +
                 (((size_t)phys * page + inpage) * hk + head) * hd;
  float *sdst = (is_k ? ksc : vsc) + ((size_t)phys * hk + head) * page + inpage;
  if (lane < half)
    ((ushort_t *)dst)[lane] = (ushort_t)quant_pair_e4m3(ev, od, scale);
  if (lane == 0) *sdst = scale;
}

// ---------------------------------------------------------------------------
// Dequantizing gather: positions [0, n) of one layer -> contiguous bf16
// [n, kh, hd]. One thread per 4 elements of K and of V. fp8 -> f32 is exact,
// then ONE fp32 multiply and ONE round to bf16.
// ---------------------------------------------------------------------------

extern "C" __global__ void __launch_bounds__(256)
kv_dequant_fp8_kernel(const uint8_t *__restrict__ kc,
                      const uint8_t *__restrict__ vc,
                      const float *__restrict__ ksc,
                      const float *__restrict__ vsc,
                      const int *__restrict__ page_table,
                      ushort_t *__restrict__ kout, ushort_t *__restrict__ vout,
                      int n, int kh, int hd, int page) {
  const int q4 = hd / 4;  // dwords per row
  const size_t total = (size_t)n * kh * q4;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int w = (int)(i % q4);
  const int head = (int)((i / q4) % kh);
  const int pos = (int)(i / ((size_t)q4 * kh));
  const int phys = page_table[pos / page];
  const int inpage = pos % page;
  const size_t src = (((size_t)phys * page + inpage) * kh + head) * hd + w * 4;
  const size_t ssrc = ((size_t)phys * kh + head) * page + inpage;
  const size_t dst = ((size_t)pos * kh + head) * hd + w * 4;
#pragma unroll
  for (int tsr = 0; tsr < 2; ++tsr) {
    const uint32_t word = *(const uint32_t *)((tsr ? vc : kc) + src);
    const float sc = (tsr ? vsc : ksc)[ssrc];
    const f32x2v lo = __builtin_amdgcn_cvt_pk_f32_fp8(word, false);
    const f32x2v hi = __builtin_amdgcn_cvt_pk_f32_fp8(word, true);
    uint2 o;
    o.x = (uint32_t)f32_to_bf16(lo.x * sc) |
          ((uint32_t)f32_to_bf16(lo.y * sc) << 16);
    o.y = (uint32_t)f32_to_bf16(hi.x * sc) |
          ((uint32_t)f32_to_bf16(hi.y * sc) << 16);
    *(uint2 *)((tsr ? vout : kout) + dst) = o;
  }
}

// ---------------------------------------------------------------------------
// Decode split kernel, fp8 cache.
// grid.x = kh, grid.y = n_splits, block = 256 (4 waves).
//
// The tile loop of attn_decode_split_tiles (attn_decode_split.h), KEPT IN
// THE SPELLING IT HAD BEFORE THAT SKELETON EXISTED: built from the skeleton
// over an fp8 trait this kernel had the same instruction counts and, at
// hd=128, an instruction-identical tile loop, and still measured 2 % slower
// solo (17.07 vs 16.68 us at 8k) for a reason that was not found. Every
// mechanism note in the skeleton's header holds here; a change to the ring,
// the waits or the softmax is made there AND here.
//
// What the 1-byte rows change:
//   - a 16-byte lane chunk is 16 elements, a row is C16 = hd/16 chunks and a
//     tile is C16 1-KiB pieces per tensor. The 2*C16 pieces of a tile are
//     dealt over the 4 waves as whole pieces (waves 0-1 fetch K, waves 2-3
//     fetch V), C16/2 each — hd=32 has fewer pieces per tensor than waves.
//   - the tile's 64 K scales and 64 V scales ride the same DMA pipeline as
//     one 4-byte-per-lane piece each with per-lane source addresses (an
//     ordinary load in the tile loop would drain the queue at its use).
//     Every wave issues exactly one: even waves the K scales, odd waves the
//     V scales; the two waves of a parity write identical words to the same
//     image. Each wave therefore has C16/2 + 1 loads outstanding per tile,
//     a compile-time count, and the counted waits stay immediates.
//     This holds for the IDENT template (the engine's identity page table,
//     pure address math). With IDENT false the page-table entry is an
//     ordinary per-lane VMEM load inside stage_tile, for the rows and again
//     for the scales; hipcc waits vmcnt(0) at its use and so drains the DMA
//     queue once per staged tile — correct but slower, exactly as in the
//     bf16 kernel, and only non-identity tables take it.
//   - scales fold in as per-lane scalars: the raw score times the lane's K
//     scale before max/exp; the lane's p times its V scale before the shfl
//     broadcast into PV. l accumulates the unscaled p.
//   - K bytes are widened to bf16 pairs (exact: 3 mantissa bits) and dotted
//     against the bf16 q image with v_dot2_f32_bf16, fp32 accumulation.
//
// Positions >= seq_len clamp to the last valid row for the rows AND the
// scales, so nothing past the sequence is ever read.
// ---------------------------------------------------------------------------

// 4 e4m3 bytes of `w` -> two packed bf16 pairs
DEVINL void fp8x4_to_bf16x4(uint32_t w, uint32_t &p01, uint32_t &p23) {
  const f32x2v lo = __builtin_amdgcn_cvt_pk_f32_fp8(w, false);
  const f32x2v hi = __builtin_amdgcn_cvt_pk_f32_fp8(w, true);
  // bytes [2,3] of each float are its bf16 image
  p01 = __builtin_amdgcn_perm(__float_as_uint(lo.y), __float_as_uint(lo.x),
                              0x07060302u);
  p23 = __builtin_amdgcn_perm(__float_as_uint(hi.y), __float_as_uint(hi.x),
                              0x07060302u);
}

// WIN: the sliding-window range and its low-side compare are a template flag
// here. As a run-time `window` (the bf16 skeleton's form, free there) hipcc
// allocated this kernel's registers differently (hd=128 group 4: 102 -> 92
// VGPRs, +70 instructions) and the windowless 8k solo call measured 5 %
// slower (17.50 vs 16.64 us). With the flag off, `start` and `limit` are
// the windowless expressions and `window` is the LAST argument, so no other
// argument moves: every windowless instantiation is then the code it was
// before the window existed, instruction for instruction, but for the offset
// of one hidden kernel argument, and measures the same (16.66 vs 16.67 us;
// profiles/r09_sliding_window.md). Formed as `0 + split * split_len` and
// `start + split_len` with `window` in the middle of the list, the same
// register counts still measured 16.94 us.
template <int HD, int MG, bool IDENT, bool WIN>
__global__ void __launch_bounds__(256) attn_decode_split_fp8_kernel(
    const ushort_t *__restrict__ q,   // [hq, hd] bf16
    const uint8_t *__restrict__ kc, const uint8_t *__restrict__ vc,
    const float *__restrict__ ksc, const float *__restrict__ vsc,
    const int *__restrict__ page_table, int seq_len, float scale,
    int kh, int group, int page, int split_len,
    float *__restrict__ ws_m, float *__restrict__ ws_l,
    float *__restrict__ ws_acc, const int *__restrict__ pos_ptr,
    ushort_t *__restrict__ out, int window) {
  if (pos_ptr) seq_len = *pos_ptr + 1;  // graph mode, as the bf16 kernel
  constexpr int C16 = HD / 16;       // 16-B chunks per row = lanes per position
  constexpr int SUBS = WAVE / C16;   // rows per piece = positions per PV step
  constexpr int PW = C16 / 2;        // K/V pieces per wave per tile
  constexpr int NG = (MG + 3) / 4;   // GQA heads owned per wave
  const int g = blockIdx.x;          // kv head
  const int split = blockIdx.y;
  const int n_splits = gridDim.y;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int sub = lane / C16;
  const int sl = lane % C16;

  // sliding window: as the skeleton (see its header)
  int lo = 0, start, limit;
  if constexpr (WIN) {
    lo = max(0, seq_len - window);
    start = (lo & ~(DTILE - 1)) + split * split_len;
    limit = min(seq_len, start + split_len);
  } else {  // the windowless expressions, as they were before the window
    start = split * split_len;
    limit = min(seq_len, (split + 1) * split_len);
  }

  // ONE shared array: [2 stage buffers][K | V | K scales | V scales] + the
  // bf16 q image (whole 1-KiB pieces, as in the bf16 kernel).
  constexpr int TILE_B = DTILE * HD;   // bytes per tensor per tile
  constexpr int SC_B = DTILE * 4;      // bytes per scale vector per tile
  constexpr int BUF_B = 2 * TILE_B + 2 * SC_B;
  constexpr int QPIECE_E = WAVE * 8;
  constexpr int QPIECES = (MG * HD + QPIECE_E - 1) / QPIECE_E;
  __shared__ __attribute__((aligned(16)))
  uint8_t lds[2 * BUF_B + QPIECES * QPIECE_E * 2];
  ushort_t *qlds = (ushort_t *)(lds + 2 * BUF_B);

  // K chunk swizzle: a 256-B bank row holds 16/C16 image rows; XOR the
  // chunk index with the row's bank-alias class (16 lanes reading the same
  // chunk index of 16 consecutive rows then cover 16 distinct 16-B slots).
  constexpr int SWZ_DIV = 16 / C16;
  auto kswz = [&](int row) { return (row / SWZ_DIV) & (C16 - 1); };

  float m[NG], l[NG], acc[NG][16];
#pragma unroll
  for (int gi = 0; gi < NG; ++gi) {
    m[gi] = -INFINITY;
    l[gi] = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[gi][j] = 0.f;
  }

  // IDENT: no table read. Otherwise an ordinary load whose use drains the
  // DMA queue (see the header).
  auto phys_page = [&](int pp) {
    return IDENT ? (pp / page) : page_table[pp / page];
  };

  // stage one tile into buffer b: PW row pieces + 1 scale piece per wave.
  auto stage_tile = [&](int t0, int b) {
    uint8_t *buf = lds + (size_t)b * BUF_B;
#pragma unroll
    for (int i = 0; i < PW; ++i) {
      const int gp = wid * PW + i;        // piece of the tile: [K | V]
      const bool isv = gp >= C16;         // wave-uniform
      const int prow = (isv ? gp - C16 : gp) * SUBS;  // tile-local row
      const int myrow = prow + sub;
      const int pp = min(t0 + myrow, seq_len - 1);
      const size_t row =
          (((size_t)phys_page(pp) * page + (pp % page)) * kh + g) * HD;
      const int chunk = isv ? sl : (sl ^ kswz(myrow));
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void
               *)((isv ? vc : kc) + row + (size_t)chunk * 16),
          (__attribute__((address_space(3))) void *)(buf +
                                                     (isv ? TILE_B : 0) +
                                                     (size_t)prow * HD),
          16, 0, 0);
    }
    {
      const int pp = min(t0 + lane, seq_len - 1);
      const size_t si = ((size_t)phys_page(pp) * kh + g) * page + (pp % page);
      const int par = wid & 1;            // 0: K scales, 1: V scales
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void
               *)((par ? vsc : ksc) + si),
          (__attribute__((address_space(3))) void *)(buf + 2 * TILE_B +
                                                     par * SC_B),
          4, 0, 0);
    }
  };

  // q image by glds from wave 0, issued BEFORE the K/V prologue so wave
  // 0's first counted wait covers it (see the bf16 kernel).
  typedef __attribute__((__vector_size__(8 * sizeof(short)))) short v8s;
  if (wid == 0) {
#pragma unroll
    for (int i = 0; i < QPIECES; ++i) {
      if (i * QPIECE_E >= group * HD) break;  // uniform: MG may exceed group
      const int off8 = min(i * QPIECE_E + lane * 8, group * HD - 8);
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void
               *)(q + (size_t)(g * group) * HD + off8),
          (__attribute__((address_space(3))) void *)(qlds + i * QPIECE_E), 16,
          0, 0);
    }
  }

  const int ntiles = (limit - start + DTILE - 1) / DTILE;
  float pex[NG];
  if (ntiles > 0) {
    stage_tile(start, 0);
    if (ntiles > 1) stage_tile(start + DTILE, 1);

    for (int t = 0; t < ntiles; ++t) {
      // wait for tile t's DMA; tile t+1 (PW + 1 loads per wave) stays in
      // flight. Wave 0's q pieces are older than tile 0's.
      if (ntiles > t + 1) {
        if (PW == 4) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        else if (PW == 2) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_s_barrier();
      const uint8_t *kimg = lds + (size_t)(t & 1) * BUF_B;
      const uint8_t *vimg = kimg + TILE_B;
      const float *scimg = (const float *)(kimg + 2 * TILE_B);
      const int tbase = start + t * DTILE;
      const float kscale = scimg[lane];
      const float vscale = scimg[DTILE + lane];

      // ---- QK: lane-per-position full dot; the widened K chunk serves
      // every head this wave owns ----
      const bool valid =
          (!WIN || tbase + lane >= lo) && tbase + lane < limit;
      const int myswz = kswz(lane);
      float a4[NG][4];
#pragma unroll
      for (int gi = 0; gi < NG; ++gi)
#pragma unroll
        for (int j = 0; j < 4; ++j) a4[gi][j] = 0.f;
#pragma unroll
      for (int c = 0; c < C16; ++c) {
        const u32x4v kw = ((const u32x4v *)(kimg + (size_t)lane * HD))[c];
        uint32_t kb[8];
        fp8x4_to_bf16x4(kw.x, kb[0], kb[1]);
        fp8x4_to_bf16x4(kw.y, kb[2], kb[3]);
        fp8x4_to_bf16x4(kw.z, kb[4], kb[5]);
        fp8x4_to_bf16x4(kw.w, kb[6], kb[7]);
        const int qc = c ^ myswz;  // logical chunk this lane just read
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) {
          const int gq = wid + 4 * gi;
          if (gq >= group) break;  // wave-uniform
          const v8s *qp = (const v8s *)(qlds + (size_t)gq * HD) + 2 * qc;
          const v8s q0 = qp[0], q1 = qp[1];
          const bf16x2v_ *qa = (const bf16x2v_ *)&q0;
          const bf16x2v_ *qb = (const bf16x2v_ *)&q1;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            a4[gi][j] = __builtin_amdgcn_fdot2_f32_bf16(
                qa[j], __builtin_bit_cast(bf16x2v_, kb[j]), a4[gi][j], false);
            a4[gi][j] = __builtin_amdgcn_fdot2_f32_bf16(
                qb[j], __builtin_bit_cast(bf16x2v_, kb[4 + j]), a4[gi][j],
                false);
          }
        }
      }

      // ---- online softmax in the log2-scaled domain, one wave-wide
      // max/sum pair per head per tile (as the bf16 kernel) ----
      const float scale2 = scale * 1.4426950408889634f;
#pragma unroll
      for (int gi = 0; gi < NG; ++gi) {
        const int gq = wid + 4 * gi;
        if (gq >= group) break;  // wave-uniform
        const float s =
            ((a4[gi][0] + a4[gi][1]) + (a4[gi][2] + a4[gi][3])) * kscale;
        float mx = valid ? s : -INFINITY;
        mx = wave_reduce_max(mx);
        const float mx2 = mx * scale2;
        const float mn = fmaxf(m[gi], mx2);
        const float alpha = (mn == -INFINITY) ? 0.f : exp2f(m[gi] - mn);
        const float p =
            (valid && mn != -INFINITY)
                ? exp2f(__builtin_fmaf(s, scale2, -mn))
                : 0.f;
        const float ps = wave_reduce_sum(p);
        l[gi] = l[gi] * alpha + ps;
        m[gi] = mn;
        pex[gi] = p * vscale;
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[gi][j] *= alpha;
      }

      // ---- PV: dim-sliced, 16 dims per lane; P*vscale by shfl ----
#pragma unroll 4
      for (int it = 0; it < C16; ++it) {
        const int p = it * SUBS + sub;
        const u32x4v vw = ((const u32x4v *)(vimg + (size_t)p * HD))[sl];
        const uint32_t vwords[4] = {vw.x, vw.y, vw.z, vw.w};
        float vd[16];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const f32x2v lo = __builtin_amdgcn_cvt_pk_f32_fp8(vwords[w], false);
          const f32x2v hi = __builtin_amdgcn_cvt_pk_f32_fp8(vwords[w], true);
          vd[4 * w + 0] = lo.x;
          vd[4 * w + 1] = lo.y;
          vd[4 * w + 2] = hi.x;
          vd[4 * w + 3] = hi.y;
        }
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) {
          if (wid + 4 * gi >= group) break;
          const float pw = __shfl(pex[gi], p, WAVE);
#pragma unroll
          for (int j = 0; j < 16; ++j)
            acc[gi][j] = fmaf(pw, vd[j], acc[gi][j]);
        }
      }

      // issue tile t+2 into the buffer just consumed, after re-aligning
      __builtin_amdgcn_s_barrier();
      if (t + 2 < ntiles) stage_tile(tbase + 2 * DTILE, t & 1);
    }
  }

  // ---- merge the PV sub-partitions (lanes xor C16, 2*C16, ...) and write
  // this split's state; each wave owns its head(s), no cross-wave merge ----
#pragma unroll
  for (int off = C16; off < WAVE; off <<= 1)
#pragma unroll
    for (int gi = 0; gi < NG; ++gi)
#pragma unroll
      for (int j = 0; j < 16; ++j)
        acc[gi][j] += __shfl_xor(acc[gi][j], off, WAVE);

#pragma unroll
  for (int gi = 0; gi < NG; ++gi) {
    const int gq = wid + 4 * gi;
    if (gq >= group) break;
    if (n_splits == 1) {
      if (lane < C16) {
        const float inv = (l[gi] > 0.f) ? 1.0f / l[gi] : 0.f;
        bf16x8 o0, o1;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          o0.u[j] = f32_to_bf16(acc[gi][j] * inv);
          o1.u[j] = f32_to_bf16(acc[gi][8 + j] * inv);
        }
        bf16x8 *dst = (bf16x8 *)(out + (size_t)(g * group + gq) * HD) + 2 * sl;
        dst[0] = o0;
        dst[1] = o1;
      }
    } else {
      const size_t base = ((size_t)g * n_splits + split) * group + gq;
      if (lane == 0) {
        ws_m[base] = m[gi];
        ws_l[base] = l[gi];
      }
      if (lane < C16) {
#pragma unroll
        for (int j = 0; j < 16; ++j)
          ws_acc[base * HD + sl * 16 + j] = acc[gi][j];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// C-linkage launch wrappers
// ---------------------------------------------------------------------------

extern "C" void launch_attn_decode_split_fp8(const ushort_t *q,
                                             const uint8_t *kc,
                                             const uint8_t *vc,
                                             const float *ksc,
                                             const float *vsc,
                                             const DecodeSplitArgs &a,
                                             ushort_t *out,
                                             hipStream_t stream) {
  const dim3 grid(a.kh, a.n_splits);
  dispatch_decode_split(a.hd, a.group, a.identity, [&](auto HD, auto MG,
                                                       auto IDENT) {
    auto launch = [&](auto WIN) {
      attn_decode_split_fp8_kernel<decltype(HD)::value, decltype(MG)::value,
                                   decltype(IDENT)::value,
                                   decltype(WIN)::value>
          <<<grid, 256, 0, stream>>>(
              q, kc, vc, ksc, vsc, a.page_table, a.seq_len, a.scale, a.kh,
              a.group, a.page, a.split_len, a.ws_m, a.ws_l, a.ws_acc,
              a.pos_ptr, out, a.window);
    };
    if (a.window > 0) launch(std::true_type{});
    else launch(std::false_type{});
  });
  if (a.n_splits > 1) {
    // the bf16 path's combine pass (attention.hip), shared unchanged
    launch_attn_decode_combine(a.ws_m, a.ws_l, a.ws_acc, out, a.n_splits,
                               a.kh, a.group, a.hd, stream);
  }
}

extern "C" void launch_rope_kv_fp8(
    ushort_t *q, ushort_t *k, const ushort_t *v, const float *cost,
    const float *sint, uint8_t *kc, uint8_t *vc, float *ksc, float *vsc,
    const int *page_table, int t, int hq, int hk, int hd, int pos0,
    long q_rstride, long k_rstride, long v_rstride, int page,
    const int *pos_ptr, hipStream_t stream) {
  const int waves = t * (hq + 2 * hk);
  const int thr = rope_kv_block_threads(t);  // shared with rope_kv
  const int blocks = (waves * 64 + thr - 1) / thr;
  rope_kv_fp8_kernel<<<blocks, thr, 0, stream>>>(
      q, k, v, cost, sint, kc, vc, ksc, vsc, page_table, t, hq, hk, hd, pos0,
      q_rstride, k_rstride, v_rstride, page, pos_ptr);
}

extern "C" void launch_kv_dequant_fp8(
    const uint8_t *kc, const uint8_t *vc, const float *ksc, const float *vsc,
    const int *page_table, ushort_t *kout, ushort_t *vout, int n, int kh,
    int hd, int page, hipStream_t stream) {
  const size_t total = (size_t)n * kh * (hd / 4);
  if (total == 0) return;
  const int blocks = (int)((total + 255) / 256);
  kv_dequant_fp8_kernel<<<blocks, 256, 0, stream>>>(
      kc, vc, ksc, vsc, page_table, kout, vout, n, kh, hd, page);
}
