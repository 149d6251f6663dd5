// Prefill MFMA GEMM tile loops for CDNA4 (gfx950), once each, over an element
// trait: C[M,N] = A[M,K] @ B[N,K]^T with fp32 accumulation and a bf16 store.
//
//   gemm128_tiles<T>   128x128 tile, two barriers per K-step (any M, N; K a
//                      whole number of 16-B chunks)
//   gemm256_tiles<T>   256x256 tile, 8 phases, staging loads span barriers
//                      behind a counted vmcnt (K % 128 == 0, K >= 512)
//
// gemm.hip instantiates gemm128_tiles over TileBf16 (gemm_nt_kernel) and
// gemm_fp8.hip both over TileE4m3 (gemm_fp8_kernel, gemm_fp8_256_kernel), where
// C = (A8 * asc[M]) @ (B8 * bsc[N])^T: row-wise scales factor out of the dot
// product, so the dequantization in the store is exact. gemm_nt256_kernel
// (gemm256.hip) is gemm256_tiles<TileBf16> still written out; see its header.
//
// These replace library GEMMs (hipBLASLt/rocBLAS) on the prefill path: besides
// the perf headroom, Tensile's skinny-m bf16 kernels return garbage
// intermittently in recycled-memory states (round-1 debugging). In-tree,
// deterministic, workspace-free, graph-capture safe.
//
// Weights are stored ROW-MAJOR [out, in] (= HF checkpoint layout, no load-time
// transpose), so A and B stage IDENTICALLY: both are [128 rows][64 k] images
// whose fragment reads are contiguous ds_reads; no LDS transpose pass anywhere.
//
// Staging and swizzle, common to both loops: __builtin_amdgcn_global_load_lds
// of width 16 writes LDS lane-linear (wave-uniform base + lane * 16), so one
// wave-instruction lands 1 KiB = 1024 / ROW_B whole image rows, and the
// bank-conflict XOR is applied to the PER-LANE GLOBAL SOURCE address: image
// row r, 16-B chunk c is fetched from global chunk c ^ key(r). That stays
// inside the row's cacheline, so coalescing is preserved, and the fragment
// read de-swizzles with the same XOR (guide §5.4 rule 21).
//
// K contract: the bindings guarantee K % 8 == 0 for bf16 (gemm, gemm_variant)
// and K % 16 == 0 for e4m3 (gemm_fp8), i.e. K is a whole number of 16-B chunks
// for either type. So every row starts 16-byte aligned (glds loads 16 B per
// lane), a K edge always ends on a whole chunk and stage_edge copies whole
// chunks only, and the row-wise fp8 quantizer, which walks K in chunks of 8,
// writes every code the GEMM reads.
#pragma once

#include "common.h"

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short bf16x8v;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4v;
typedef uint32_t chunk16 __attribute__((ext_vector_type(4)));  // 16 B, any type

constexpr int GT_K = 64;            // elements per K-step, either type
constexpr int GT_IMG = 128 * GT_K;  // elements per [128][64] image

DEVINL void glds16(const void *g, void *l) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void *)g,
      (__attribute__((address_space(3))) void *)l, 16, 0, 0);
}

// Wait until at most N of this wave's VMEM operations (glds pieces) are
// outstanding. N is an immediate: s_waitcnt takes no register operand.
template <int N>
DEVINL void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// ---- element traits ---------------------------------------------------------
// A trait T carries
//   elem, frag     element type; one lane's MFMA operand (8 elements)
//   ROW_B, CHUNKS  bytes per image row; 16-B chunks per row
//   LOADS          glds a wave issues per 256^2 half-tile: 8 waves x LOADS KiB
//                  are one image (a 128^2 block has 4 waves: 2 * LOADS each)
//   BHI_PHASE      the 256^2 phase that reads the upper half (rows 32-63) of
//                  the wave's 64 B rows; tuned per type, part of the schedule
//   key128, key256 swizzle key of an image row in either layout
//   read           the fragment of k-slice ks (32 elements) of `row` for lane
//                  quarter lhi, de-swizzled with that row's key
//   mfma           v_mfma_f32_16x16x32 of the type
//   col_scale, out the stored value: plain, or acc * asc[row] * bsc[col]
// Results come back by value (a hook that fills the caller's array by
// reference rescheduled the decode-split tile loop; attn_decode_split.h).

struct TileBf16 {
  typedef ushort_t elem;
  typedef bf16x8v frag;  // one whole 16-B chunk
  static constexpr int ROW_B = 128, CHUNKS = 8, LOADS = 2, BHI_PHASE = 2;
  // 128-B rows, 8 chunks: chunk ^= row & 7 in both layouts.
  static DEVINL int key128(int row) { return row & 7; }
  static DEVINL int key256(int row) { return row & 7; }
  static DEVINL frag read(const elem *im, int row, int ks, int lhi, int key) {
    return ((const frag *)(im + (size_t)row * GT_K))[(ks * 4 + lhi) ^ key];
  }
  static DEVINL f32x4v mfma(frag a, frag b, f32x4v c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
  static DEVINL float col_scale(const float *, int) { return 1.f; }
  static DEVINL float out(float acc, const float *, int, float) { return acc; }
};

struct TileE4m3 {
  typedef uint8_t elem;
  typedef long frag;  // the low or high half of a swizzled 16-B chunk
  static constexpr int ROW_B = 64, CHUNKS = 4, LOADS = 1, BHI_PHASE = 1;
  // 64-B rows repeat a 256-B bank row every 4 rows, so rows {r, r+4, r+8,
  // r+12} of a 16-lane read group alias the same banks at the same chunk. The
  // low-bit XOR leaves that 4-way conflict in place; the two-barrier 128^2
  // loop gets away with it, its stage stall hiding the LDS reads. In the
  // 8-phase schedule the LDS read IS the critical path (guide §5.5 T2 regime
  // gate), so the 256^2 key is row bits 2-3: the four aliasing rows get four
  // different chunks.
  static DEVINL int key128(int row) { return row & 3; }
  static DEVINL int key256(int row) { return (row >> 2) & 3; }
  static DEVINL frag read(const elem *im, int row, int ks, int lhi, int key) {
    const int ch = (ks * 2 + (lhi >> 1)) ^ key;
    return *(const frag *)(im + (size_t)row * GT_K + ch * 16 + (lhi & 1) * 8);
  }
  static DEVINL f32x4v mfma(frag a, frag b, f32x4v c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, c, 0, 0, 0);
  }
  static DEVINL float col_scale(const float *bsc, int col) { return bsc[col]; }
  static DEVINL float out(float acc, const float *asc, int row, float bs) {
    return acc * asc[row] * bs;
  }
};

template <class T>
struct TileGeom {
  static constexpr int EPC = 16 / (int)sizeof(typename T::elem);  // per chunk
  static constexpr int RPP = 1024 / T::ROW_B;  // image rows per glds piece
  static_assert(T::CHUNKS * 16 == T::ROW_B &&
                GT_K * sizeof(typename T::elem) == T::ROW_B);
  static_assert(8 * T::LOADS * RPP == 128, "8 waves x LOADS KiB = one image");
};

// Guarded store of a wave's MI x 4 grid of 16x16 D tiles whose corner is
// (row0, col0): D frag lane l -> col l%16, rows (l/16)*4 + 0..3.
template <class T, int MI>
DEVINL void store_tiles(const f32x4v (&acc)[MI][4], int row0, int col0, int M,
                        int N, const float *__restrict__ asc,
                        const float *__restrict__ bsc,
                        ushort_t *__restrict__ c_out, int lrow, int lhi) {
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int col = col0 + ni * 16 + lrow;
      if (col >= N) continue;
      const float bs = T::col_scale(bsc, col);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + mi * 16 + lhi * 4 + r;
        if (row >= M) continue;
        c_out[(size_t)row * N + col] =
            f32_to_bf16(T::out(acc[mi][ni][r], asc, row, bs));
      }
    }
  }
}

// ---- 128^2: double-buffered, one barrier per K-step -------------------------
// The cdna_hip_programming.md "step 3" ladder (~900 TF/s at 4096^3 bf16):
// block 256 threads = 4 waves in a 2x2 quadrant grid, each wave owns a 64x64
// output quadrant = 4x4 MFMA tiles. Interior tiles stage by glds; edge tiles
// (M/N/K not tile-aligned) take a guarded register-staging path into the same
// swizzled image, so the MFMA loop is shared.
template <class T>
struct gemm128_tiles {
  typedef typename T::elem elem;
  typedef TileGeom<T> G;
  static constexpr int ISSUES = 2 * T::LOADS;  // per wave, and per thread below

  static DEVINL void stage_glds(const elem *__restrict__ src, long row_stride,
                                elem *__restrict__ img, int tid) {
    const int lane = tid & (WAVE - 1);
    const int wid = tid / WAVE;
#pragma unroll
    for (int i = 0; i < ISSUES; ++i) {
      const int r0 = (wid * ISSUES + i) * G::RPP;
      const int row = r0 + lane / T::CHUNKS;
      const int c = lane & (T::CHUNKS - 1);
      glds16(src + (size_t)row * row_stride +
                 (size_t)(c ^ T::key128(row)) * G::EPC,
             img + (size_t)r0 * GT_K);
    }
  }

  // 128 rows x CHUNKS whole 16-B chunks, ISSUES per thread; rows past the
  // M/N edge and chunks past K are zero.
  static DEVINL void stage_edge(const elem *__restrict__ src, long row_stride,
                                int rows_left, int k_left,
                                elem *__restrict__ img, int tid) {
#pragma unroll
    for (int p = 0; p < ISSUES; ++p) {
      const int piece = tid + 256 * p;
      const int row = piece / T::CHUNKS;
      const int c = piece & (T::CHUNKS - 1);
      const int gk = c * G::EPC;
      chunk16 v = {0, 0, 0, 0};
      if (row < rows_left && gk < k_left)
        v = *(const chunk16 *)(src + (size_t)row * row_stride + gk);
      ((chunk16 *)(img + (size_t)row * GT_K))[c ^ T::key128(row)] = v;
    }
  }

  // lds: [A buf 0][A buf 1][B buf 0][B buf 1], GT_IMG elements each.
  static DEVINL void run(const elem *__restrict__ a,
                         const float *__restrict__ asc,
                         const elem *__restrict__ b,
                         const float *__restrict__ bsc,
                         ushort_t *__restrict__ c_out, int M, int N, int K,
                         elem *__restrict__ lds) {
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wid = tid / WAVE;
    const int lrow = lane & 15;
    const int lhi = lane >> 4;

    const int n0 = blockIdx.x * 128;
    const int m0 = blockIdx.y * 128;
    const int wm = (wid >> 1) * 64;  // wave quadrant
    const int wn = (wid & 1) * 64;

    f32x4v acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4v){0.f, 0.f, 0.f, 0.f};

    const int ntiles = (K + GT_K - 1) / GT_K;
    // block-uniform edge predicates: only edge blocks (and the last K tile
    // when K % 64 != 0) pay the guarded register-staging path
    const bool a_edge = (M - m0) < 128;
    const bool b_edge = (N - n0) < 128;

    auto stage = [&](int kt, int buf) {
      const elem *asrc = a + (size_t)m0 * K + (size_t)kt * GT_K;
      const elem *bsrc = b + (size_t)n0 * K + (size_t)kt * GT_K;
      elem *imgA = lds + (size_t)buf * GT_IMG;
      elem *imgB = lds + (size_t)(2 + buf) * GT_IMG;
      const bool k_edge = (kt + 1) * GT_K > K;
      if (a_edge || k_edge) {
        stage_edge(asrc, K, M - m0, K - kt * GT_K, imgA, tid);
      } else {
        stage_glds(asrc, K, imgA, tid);
      }
      if (b_edge || k_edge) {
        stage_edge(bsrc, K, N - n0, K - kt * GT_K, imgB, tid);
      } else {
        stage_glds(bsrc, K, imgB, tid);
      }
    };

    stage(0, 0);
    __syncthreads();  // drains the glds queue (vmcnt0 inside the barrier)

    for (int kt = 0; kt < ntiles; ++kt) {
      const int buf = kt & 1;
      if (kt + 1 < ntiles) stage(kt + 1, buf ^ 1);  // prefetch next tile
      const elem *imgA = lds + (size_t)buf * GT_IMG;
      const elem *imgB = lds + (size_t)(2 + buf) * GT_IMG;

      // 2 k-subtiles of 32: 8 frag reads + 16 MFMAs each
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        typename T::frag afr[4], bfr[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = wm + i * 16 + lrow;
          afr[i] = T::read(imgA, row, s, lhi, T::key128(row));
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int row = wn + j * 16 + lrow;
          bfr[j] = T::read(imgB, row, s, lhi, T::key128(row));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = T::mfma(afr[i], bfr[j], acc[i][j]);
      }
      __syncthreads();  // compute done + prefetch glds drained
    }

    store_tiles<T, 4>(acc, m0 + wm, n0 + wn, M, N, asc, bsc, c_out, lrow, lhi);
  }
};

// ---- 256^2: 8 phases, counted vmcnt -----------------------------------------
// The 8-phase structure from cdna_hip_programming.md §5 ("The 256^2 8-phase
// template"). The 128^2 loop ceilings at ~900 TF/s because the
// workgroup-release inside its __syncthreads drains the glds queue (vmcnt(0))
// every K-step. Here the staging loads SPAN barriers behind a counted wait:
//
//   - tile 256x256, BK=64, 8 waves (2M x 4N), 512 threads;
//   - LDS = 2 buffers x 4 half-images [128][64]
//     (h0 A rows 0-127, h1 A rows 128-255, h2 B rows 0-127, h3 B rows 128-255);
//   - 4 phases per K-tile; each phase: {ds_read a fragment subtile,
//     glds-prefetch ONE half-image of a future K-tile, raw s_barrier,
//     lgkmcnt(0) if it read, setprio(1), 16 MFMA (one C-quadrant x K=64),
//     setprio(0), raw s_barrier};
//   - the ONLY vmcnt in the main loop is a counted vmcnt(2 * LOADS) once per
//     K-tile; the last boundary drains (vmcnt 0) and the epilogue stores.
//
// Schedule invariant (why vmcnt(2 * LOADS) is correct): a stage is LOADS glds
// per wave, and stages issue one half-image per phase in the order S = 4 *
// tile + half: phase 0 of tile t stages (t+1, h2), phase 1 (t+1, h3), phase 2
// (t+2, h0), phase 3 (t+2, h1), i.e. 6 phases ahead of first use. The wait at
// the end of tile t's phase 3 must cover every half of tile t+1. (t+1, h3) is
// issued at phase 4t+1, and exactly two stages, (t+2, h0) and (t+2, h1),
// follow it before the wait, so "all but the newest 2 * LOADS loads" == "tile
// t+1 fully landed". Image overwrite is safe because a barrier separates the
// last read of an image from its restage: a buffer's A images are last READ
// in phase 1 of their tile and first REWRITTEN by the stage of phase 2, its B
// images are last read in phase BHI_PHASE <= 2 and first rewritten by phase 0
// of the next tile, and a phase's reads have landed (lgkmcnt(0)) before the
// barrier that closes it. The tail tiles are peeled as template
// specializations so the main loop carries NO stage guards: a guarded variant
// spilled 3 VGPRs and hipcc's spill-reload wait (vmcnt(0)) drained the
// pipeline every iteration.
//
// Edge handling: M/N edges CLAMP the per-lane source row (reads stay in
// bounds; garbage rows only feed C rows/cols that the guarded store never
// writes). K must be a multiple of 128 and >= 512: use_gemm256 in bindings.hip
// sends everything else to the 128^2 loop.
//
// The kernel declares ONE __shared__ array and passes it in (a second
// __shared__ object de-pipelines glds; guide §5 ".s-level traps" (a)).
template <class T>
struct gemm256_tiles {
  typedef typename T::elem elem;
  typedef typename T::frag frag;
  typedef TileGeom<T> G;

  // sbase[H][i]: this lane's source pointer at k=0 for issue i of half-image
  // H (see run()). brow0: first row of the wave's N quarter inside its B
  // half-image.
  typedef const elem *const (&Sbase)[4][T::LOADS];

  // Stage half-image H of K-tile u.
  template <int H>
  static DEVINL void stage(Sbase sbase, int u, elem *__restrict__ lds,
                           int wid) {
    elem *img = lds + (size_t)((u & 1) * 4 + H) * GT_IMG;
    const long kb = (long)u * GT_K;
#pragma unroll
    for (int i = 0; i < T::LOADS; ++i)
      glds16(sbase[H][i] + kb,
             img + (size_t)(wid * T::LOADS + i) * G::RPP * GT_K);
  }

  // Phase Q of K-tile t: MFMA quadrant (mi 4*(Q&1).., ni 2*(Q>>1)..). Reads
  // A rows 0-63 and B rows 0-31 of the wave's quarter in phase 0, A rows
  // 64-127 in phase 1, B rows 32-63 in BHI_PHASE; the waits on those reads
  // exist only in a phase that has some.
  template <int Q, bool STAGE, int WAITK>
  static DEVINL void phase(const elem *__restrict__ imA,
                           const elem *__restrict__ imB, int t, Sbase sbase,
                           elem *__restrict__ lds, int wid, int lrow, int lhi,
                           int brow0, frag (&afr)[8][2], frag (&bfr)[4][2],
                           f32x4v (&acc)[8][4]) {
    constexpr int MI0 = (Q & 1) * 4, NI0 = (Q >> 1) * 2;
    constexpr bool READ_A = Q < 2;
    constexpr int RB0 = (Q == 0) ? 0 : 2;  // first B fragment row read here
    constexpr bool READ_B = Q == 0 || Q == T::BHI_PHASE;
    if (READ_A) {
#pragma unroll
      for (int mi = MI0; mi < MI0 + 4; ++mi) {
        const int row = mi * 16 + lrow;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
          afr[mi][ks] = T::read(imA, row, ks, lhi, T::key256(row));
      }
    }
    if (READ_B) {
#pragma unroll
      for (int ni = RB0; ni < RB0 + 2; ++ni) {
        const int row = brow0 + ni * 16 + lrow;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
          bfr[ni][ks] = T::read(imB, row, ks, lhi, T::key256(row));
      }
    }
    if (STAGE) stage<(Q + 2) & 3>(sbase, t + 1 + (Q >> 1), lds, wid);
    __builtin_amdgcn_s_barrier();
    if (READ_A || READ_B) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int mi = MI0; mi < MI0 + 4; ++mi)
#pragma unroll
      for (int ni = NI0; ni < NI0 + 2; ++ni)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
          acc[mi][ni] = T::mfma(afr[mi][ks], bfr[ni][ks], acc[mi][ni]);
    __builtin_amdgcn_s_setprio(0);
    if (Q == 3 && WAITK >= 0) wait_vmcnt<(WAITK >= 0 ? WAITK : 0)>();
    __builtin_amdgcn_s_barrier();
  }

  // One K-tile. The first NSTAGE phases each issue a stage; WAITK is the
  // vmcnt immediate at the tile boundary (-1: none).
  template <int NSTAGE, int WAITK>
  static DEVINL void tile(const elem *__restrict__ imA,
                          const elem *__restrict__ imB, int t, Sbase sbase,
                          elem *__restrict__ lds, int wid, int lrow, int lhi,
                          int brow0, frag (&afr)[8][2], frag (&bfr)[4][2],
                          f32x4v (&acc)[8][4]) {
    phase<0, (NSTAGE > 0), WAITK>(imA, imB, t, sbase, lds, wid, lrow, lhi,
                                  brow0, afr, bfr, acc);
    phase<1, (NSTAGE > 1), WAITK>(imA, imB, t, sbase, lds, wid, lrow, lhi,
                                  brow0, afr, bfr, acc);
    phase<2, (NSTAGE > 2), WAITK>(imA, imB, t, sbase, lds, wid, lrow, lhi,
                                  brow0, afr, bfr, acc);
    phase<3, (NSTAGE > 3), WAITK>(imA, imB, t, sbase, lds, wid, lrow, lhi,
                                  brow0, afr, bfr, acc);
  }

  static DEVINL void run(const elem *a,
                         const float *asc,
                         const elem *b,
                         const float *bsc,
                         ushort_t *c_out, int M, int N, int K,
                         elem *lds) {
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wid = tid / WAVE;  // 0..7
    const int lrow = lane & 15;
    const int lhi = lane >> 4;
    const int wm = wid >> 2;     // wave M half: rows wm*128 .. +127
    const int wn = wid & 3;      // wave N quarter: cols wn*64 .. +63

    const int n0 = blockIdx.x * 256;
    const int m0 = blockIdx.y * 256;
    const int nt = K / GT_K;

    // Per-lane stage source pointers at k=0, one per (half-image, issue): row
    // clamped into bounds, chunk index XOR-swizzled within the row.
    const elem *sbase[4][T::LOADS];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const elem *src = (h < 2) ? a : b;
      const int row0 = (h < 2) ? (m0 + h * 128) : (n0 + (h - 2) * 128);
      const int rmax = ((h < 2) ? M : N) - 1;
#pragma unroll
      for (int i = 0; i < T::LOADS; ++i) {
        const int rl = (wid * T::LOADS + i) * G::RPP + lane / T::CHUNKS;
        const int grow = min(row0 + rl, rmax);
        const int c = lane & (T::CHUNKS - 1);
        sbase[h][i] =
            src + (size_t)grow * K + (size_t)(c ^ T::key256(rl)) * G::EPC;
      }
    }

    f32x4v acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4v){0.f, 0.f, 0.f, 0.f};

    // prologue: stage tile 0 + halves h0/h1 of tile 1; wait for tile 0
    stage<0>(sbase, 0, lds, wid);
    stage<1>(sbase, 0, lds, wid);
    stage<2>(sbase, 0, lds, wid);
    stage<3>(sbase, 0, lds, wid);
    stage<0>(sbase, 1, lds, wid);
    stage<1>(sbase, 1, lds, wid);
    wait_vmcnt<2 * T::LOADS>();
    __builtin_amdgcn_s_barrier();

    // per-wave image base offsets (within a buffer)
    const size_t offA = (size_t)wm * GT_IMG;
    const size_t offB = (size_t)(2 + (wn >> 1)) * GT_IMG;
    const int brow0 = (wn & 1) * 64;  // rows in B image

    frag afr[8][2];
    frag bfr[4][2];

    int t = 0;
    for (; t + 2 < nt; ++t) {
      const elem *imA = lds + (size_t)(t & 1) * 4 * GT_IMG + offA;
      const elem *imB = lds + (size_t)(t & 1) * 4 * GT_IMG + offB;
      tile<4, 2 * T::LOADS>(imA, imB, t, sbase, lds, wid, lrow, lhi, brow0,
                            afr, bfr, acc);
    }
    {  // tile nt-2: only h2/h3 of tile nt-1 remain to stage; full drain
      const elem *imA = lds + (size_t)(t & 1) * 4 * GT_IMG + offA;
      const elem *imB = lds + (size_t)(t & 1) * 4 * GT_IMG + offB;
      tile<2, 0>(imA, imB, t, sbase, lds, wid, lrow, lhi, brow0, afr, bfr,
                 acc);
      ++t;
    }
    {  // tile nt-1: nothing in flight, nothing to stage
      const elem *imA = lds + (size_t)(t & 1) * 4 * GT_IMG + offA;
      const elem *imB = lds + (size_t)(t & 1) * 4 * GT_IMG + offB;
      tile<0, -1>(imA, imB, t, sbase, lds, wid, lrow, lhi, brow0, afr, bfr,
                  acc);
    }

    store_tiles<T, 8>(acc, m0 + wm * 128, n0 + wn * 64, M, N, asc, bsc, c_out,
                      lrow, lhi);
  }
};
