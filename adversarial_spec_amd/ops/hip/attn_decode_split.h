// Decode-attention split kernel: the tile loop, once, over a KV-format trait.
//
// attn_decode_split_kernel (attention.hip, bf16 cache) is
// `attn_decode_split_tiles<KV, MG, IDENT>` below over the KvBf16 trait.
// attn_decode_split_fp8_kernel (kv_fp8.hip, e4m3 cache + per-row scales) is
// the same loop still written out (see the note above it): over an fp8 trait
// (SCALED, 16 elements per chunk) it compiled to the same instruction counts
// and measured 2 % slower. Both launchers share dispatch_decode_split.
//
// grid.x = kh, grid.y = n_splits, block = 256 (4 waves).
//
// The KV read is staged through LDS by async global_load_lds in 64-position
// double-buffered tiles (LDS-DMA keeps a whole tile in flight behind a
// counted vmcnt — register-ring prefetch measured latency-bound).
//
// Compute is GROUP-PER-WAVE, LANE-PER-POSITION: wave w owns GQA head w (and
// w+4 at group 8); in the QK pass lane p holds position tbase+p's full dot
// (the K image is chunk-XOR-swizzled so 16-lane b128 groups reading the same
// chunk index of 16 different rows stay conflict-free), so the online-softmax
// reduce is ONE 6-level wave reduction per 64-position tile — the old
// dim-sliced layout paid 4 shfl-chain levels per position per group (64+
// chained DS ops per tile). P values reach the dim-sliced PV pass by shfl
// broadcast.
//
// What keeps the DMA pipeline full; each of these is a .s-verified failure
// mode, and each holds for every trait:
//   - no ds_write anywhere in the kernel: an LDS store makes hipcc order
//     every stage-image ds_read behind vmcnt(0).
//   - 16-byte LDS reads go through plain vector types (v8s, u32x4v): a
//     ds_read of a struct type (uint4) carries no alias info and is ordered
//     behind vmcnt(0) while a global_load_lds is in flight.
//   - everything the tile loop consumes arrives by glds — q and the fp8
//     scales too. An ordinary VMEM load whose wait lands inside the loop
//     forces hipcc to a loop-variant count, i.e. vmcnt(0) per iteration.
//   - the counted wait is a compile-time immediate (KV::LOADS_PER_TILE).
//   - ONE shared array per kernel (a second __shared__ object beside the
//     staging array brings the vmcnt(0) back).
//   This holds for the IDENT template (the engine's identity page table,
//   pure address math). With IDENT false the page-table entry is an ordinary
//   per-lane VMEM load inside stage_tile; hipcc waits vmcnt(0) at its use
//   and so drains the DMA queue once per staged tile — correct but slower,
//   and only non-identity tables take it.
//
// Positions >= seq_len clamp to the last valid row when staged (their scores
// are masked in compute), so nothing past the sequence is ever read.
//
// Sliding window (window = W >= 1): the block range moves, the ring does not.
// With lo = max(0, seq_len - W) the splits tile [lo & ~(DTILE-1), seq_len),
// so tile starts stay DTILE-aligned, and a lane is valid when lo <= position
// < limit. Rows below lo inside the first tile are real cache rows that get
// p = 0; they need no clamp. The host sizes the grid for min(bound, W + DTILE
// - 1) positions, which covers that range at every live length. window = 0
// gives lo = 0 and the walk from position 0.
//
// Workspace (fp32): ws_m, ws_l: [kh, n_splits, group]
//                   ws_acc:     [kh, n_splits, group, hd]
//
// A trait KV is instantiated on the head dim and holds the cache pointers:
//   HD, EPL           head dim; elements per 16-byte lane chunk
//   LPP               lanes per position = HD / EPL
//   BUF_B             bytes of one stage buffer, K image first
//   LOADS_PER_TILE    glds instructions EACH wave issues per staged tile
//   SCALED            per-position K and V scales ride in the stage buffer
//   stage_tile<IDENT>(buf, t0, w)    issue one tile's glds pieces into buf
//   part = qk_chunks<NG>(buf, qlds, w, group), qk_head(part, gi, buf, qlds, w)
//                     the QK pass in two hooks; the second returns the raw
//                     dot of the wave's head gi with the lane's position
//   load_v(buf, p, sl)               chunk sl of V row p as EPL floats (.v[])
// Hooks return by value (f32xN): see the note there.
//   k_scale(buf, lane), v_scale(buf, lane)       only when SCALED
#pragma once

#include <type_traits>

#include "common.h"

constexpr int DTILE = 64;  // positions staged per LDS tile (= WAVE)

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short v8s;
typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));

// N floats returned by value from a trait hook. By value on purpose: with
// a hook that fills the caller's array through a reference, hipcc scheduled
// the tile loop and the sub-partition merge of an fp8 trait differently
// (same instructions, the merge behind 5 waits instead of 2; .s-verified).
template <int N>
struct f32xN { float v[N]; };

// What a wave needs to place its share of a tile.
struct SplitWave {
  const int *page_table;
  int seq_len, kh, page;
  int g;     // kv head
  int wid, lane;
};

// One wave-wide LDS-DMA piece: lane l's `bytes` land at dst + l * bytes (the
// LDS side is lane-linear; only the global side is per-lane).
DEVINL void glds16(const void *src, void *dst) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void *)src,
      (__attribute__((address_space(3))) void *)dst, 16, 0, 0);
}
DEVINL void glds4(const void *src, void *dst) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void *)src,
      (__attribute__((address_space(3))) void *)dst, 4, 0, 0);
}

// Wait until at most N of this wave's VMEM operations (glds pieces) are
// outstanding. N is an immediate: s_waitcnt takes no register operand.
template <int N>
DEVINL void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// K chunk swizzle: a 256-B LDS bank row holds 16/LPP image rows, so
// same-chunk reads of two rows collide whenever the rows share a bank-row
// offset (p ≡ p' mod 16/LPP); XOR the chunk index with the row's bank-alias
// class to spread them. The glds SOURCE chunk is pre-swizzled with the same
// involution so the lane-linear LDS image realizes the swizzled layout.
template <int LPP>
DEVINL int kswz(int row) { return (row / (16 / LPP)) & (LPP - 1); }

// Physical page of logical position pp.
template <bool IDENT>
DEVINL int phys_page(const SplitWave &w, int pp) {
  return IDENT ? (pp / w.page) : w.page_table[pp / w.page];
}

template <class KV, int MG, bool IDENT>
DEVINL void attn_decode_split_tiles(
    const KV kv, const ushort_t *__restrict__ q,  // [hq, hd] bf16
    const int *__restrict__ page_table, int seq_len, float scale, int kh,
    int group, int page, int split_len, int window,
    float *__restrict__ ws_m, float *__restrict__ ws_l,
    float *__restrict__ ws_acc, const int *__restrict__ pos_ptr,
    ushort_t *__restrict__ out) {
  constexpr int HD = KV::HD, EPL = KV::EPL, LPP = KV::LPP;
  constexpr int SUBS = WAVE / LPP;   // concurrent positions per PV step
  constexpr int NG = (MG + 3) / 4;   // GQA heads owned per wave
  // graph mode: seq_len = *pos_ptr + 1 (attend up to and incl. the token
  // kv_write just appended at position *pos_ptr)
  if (pos_ptr) seq_len = *pos_ptr + 1;
  const int g = blockIdx.x;          // kv head
  const int split = blockIdx.y;
  const int n_splits = gridDim.y;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int sub = lane / LPP;        // PV pass: position sub-group
  const int sl = lane % LPP;         // PV pass: dim slice within position
  const SplitWave w{page_table, seq_len, kh, page, g, wid, lane};

  const int lo = window ? max(0, seq_len - window) : 0;
  const int start = (lo & ~(DTILE - 1)) + split * split_len;
  const int limit = min(seq_len, start + split_len);

  // ONE shared array: [2 stage buffers] + the bf16 q image. The q image is
  // written by whole-wave 16-B glds pieces (64 lanes x 8 elements = 512
  // elements each), so it is sized in whole pieces: MG*HD alone is under
  // one piece for most instantiations and the DMA would land past the end
  // of the array.
  constexpr int QPIECE_E = WAVE * 8;
  constexpr int QPIECES = (MG * HD + QPIECE_E - 1) / QPIECE_E;
  __shared__ __attribute__((aligned(16)))
  uint8_t lds[2 * KV::BUF_B + QPIECES * QPIECE_E * 2];
  ushort_t *qlds = (ushort_t *)(lds + 2 * KV::BUF_B);

  float m[NG], l[NG], acc[NG][EPL];
#pragma unroll
  for (int gi = 0; gi < NG; ++gi) {
    m[gi] = -INFINITY;
    l[gi] = 0.f;
#pragma unroll
    for (int j = 0; j < EPL; ++j) acc[gi][j] = 0.f;
  }

  // stage q (group*HD elements) by glds from wave 0, issued BEFORE the K/V
  // prologue, so wave 0's first counted wait covers the pieces and the
  // barrier publishes the image. The last piece clamps its source so the
  // DMA stays inside q.
  if (wid == 0) {
#pragma unroll
    for (int i = 0; i < QPIECES; ++i) {
      if (i * QPIECE_E >= group * HD) break;  // uniform: MG may exceed group
      const int off8 = min(i * QPIECE_E + lane * 8, group * HD - 8);
      glds16(q + (size_t)(g * group) * HD + off8, qlds + i * QPIECE_E);
    }
  }

  const int ntiles = (limit - start + DTILE - 1) / DTILE;
  float pex[NG];
  if (ntiles > 0) {
    kv.template stage_tile<IDENT>(lds, start, w);
    if (ntiles > 1)
      kv.template stage_tile<IDENT>(lds + KV::BUF_B, start + DTILE, w);

    for (int t = 0; t < ntiles; ++t) {
      // wait for tile t's DMA, then align. While tile t+1 stays in flight
      // this wave has exactly its LOADS_PER_TILE pieces outstanding behind
      // tile t's; wave 0's q pieces are OLDER than tile 0's, so the same
      // counted wait covers them.
      if (ntiles > t + 1) wait_vmcnt<KV::LOADS_PER_TILE>();
      else wait_vmcnt<0>();
      __builtin_amdgcn_s_barrier();
      const uint8_t *buf = lds + (size_t)(t & 1) * KV::BUF_B;
      const int tbase = start + t * DTILE;
      [[maybe_unused]] float kscale, vscale;
      if constexpr (KV::SCALED) {
        kscale = KV::k_scale(buf, lane);
        vscale = KV::v_scale(buf, lane);
      }

      // ---- QK: lane-per-position full dot against the q image. A trait
      // does the work either in qk_chunks (K chunk outside, every head at
      // once, partial sums returned) or in qk_head (one head at a time). ----
      const bool valid = tbase + lane >= lo && tbase + lane < limit;
      const auto part = KV::template qk_chunks<NG>(buf, qlds, w, group);
#pragma unroll
      for (int gi = 0; gi < NG; ++gi) {
        if (wid + 4 * gi >= group) break;  // wave-uniform
        float s = KV::qk_head(part, gi, buf, qlds, w);
        if constexpr (KV::SCALED) s *= kscale;

        // ---- online softmax for this head in the LOG2-SCALED domain (m
        // tracks m2 = max*scale*log2e; p = exp2(fma(s, scale2, -m2)) — one
        // fma+exp per element, no scale/sub passes); ONE wave-wide max/sum
        // pair per head per tile. The K scale has folded into the raw
        // score; the V scale folds into the p that PV broadcasts; l sums
        // the unscaled p. ----
        const float scale2 = scale * 1.4426950408889634f;
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
        if constexpr (KV::SCALED) pex[gi] = p * vscale;
        else pex[gi] = p;
#pragma unroll
        for (int j = 0; j < EPL; ++j) acc[gi][j] *= alpha;
      }

      // ---- PV: dim-sliced; this tile's P values arrive by shfl from the
      // lane that owns the position (no LDS write — see header) ----
#pragma unroll 4
      for (int it = 0; it < LPP; ++it) {
        const int p = it * SUBS + sub;
        const auto vd = KV::load_v(buf, p, sl);
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) {
          if (wid + 4 * gi >= group) break;
          const float pw = __shfl(pex[gi], p, WAVE);
#pragma unroll
          for (int j = 0; j < EPL; ++j)
            acc[gi][j] = fmaf(pw, vd.v[j], acc[gi][j]);
        }
      }

      // issue tile t+2 into the buffer just consumed — after re-aligning
      // so no wave still reads it
      __builtin_amdgcn_s_barrier();
      if (t + 2 < ntiles)
        kv.template stage_tile<IDENT>(lds + (size_t)(t & 1) * KV::BUF_B,
                                      tbase + 2 * DTILE, w);
    }
  }

  // ---- merge the PV sub-partitions (lanes xor LPP, 2*LPP, ...) and
  // write this split's state. m/l are already wave-uniform; each wave
  // owns its head(s), so there is NO cross-wave merge at all. ----
#pragma unroll
  for (int off = LPP; off < WAVE; off <<= 1)
#pragma unroll
    for (int gi = 0; gi < NG; ++gi)
#pragma unroll
      for (int j = 0; j < EPL; ++j)
        acc[gi][j] += __shfl_xor(acc[gi][j], off, WAVE);

#pragma unroll
  for (int gi = 0; gi < NG; ++gi) {
    const int gq = wid + 4 * gi;
    if (gq >= group) break;
    if (n_splits == 1) {
      // whole softmax state in this block: write the output directly
      if (lane < LPP) {
        const float inv = (l[gi] > 0.f) ? 1.0f / l[gi] : 0.f;
        bf16x8 o[EPL / 8];
#pragma unroll
        for (int j = 0; j < EPL; ++j)
          o[j / 8].u[j % 8] = f32_to_bf16(acc[gi][j] * inv);
        bf16x8 *dst =
            (bf16x8 *)(out + (size_t)(g * group + gq) * HD) + (EPL / 8) * sl;
#pragma unroll
        for (int h = 0; h < EPL / 8; ++h) dst[h] = o[h];
      }
    } else {
      const size_t base = ((size_t)g * n_splits + split) * group + gq;
      if (lane == 0) {
        ws_m[base] = m[gi];
        ws_l[base] = l[gi];
      }
      if (lane < LPP) {
#pragma unroll
        for (int j = 0; j < EPL; ++j)
          ws_acc[base * HD + sl * EPL + j] = acc[gi][j];
      }
    }
  }
}

// The launcher's hd x MG x identity switch: f(HD, MG, IDENT) is called once
// with std::integral_constant tags. MG = smallest supported bound >= group
// keeps the per-head state arrays (online-softmax accumulators) sized to the
// real GQA group; IDENT elides the page-table read (identity single-pool
// cache).
template <class F>
inline void dispatch_decode_split(int hd, int group, bool identity, F &&f) {
  auto with_hd = [&](auto HD) {
    auto with_mg = [&](auto MG) {
      if (identity) f(HD, MG, std::true_type{});
      else f(HD, MG, std::false_type{});
    };
    if (group <= 2) with_mg(std::integral_constant<int, 2>{});
    else if (group <= 4) with_mg(std::integral_constant<int, 4>{});
    else with_mg(std::integral_constant<int, 8>{});
  };
  switch (hd) {
    case 32: with_hd(std::integral_constant<int, 32>{}); break;
    case 64: with_hd(std::integral_constant<int, 64>{}); break;
    case 128: with_hd(std::integral_constant<int, 128>{}); break;
  }
}
