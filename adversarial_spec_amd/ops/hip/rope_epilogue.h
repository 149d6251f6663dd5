// RoPE + paged KV append as the epilogue of the w32 decode GEMVs
// (gemv.hip bf16, gemv_fp8.hip fp8).
//
// In the w32 geometry wave `wid` of a block owns output rows
// blockIdx.x*8 + wid*2 + {0,1}: lanes 0..31 reduce the even row, lanes
// 32..63 the odd one, i.e. every wave holds exactly one interleaved RoPE
// pair of the fused qkv row vector [q heads | k heads | v heads]. One
// cross-half shfl hands lane 0 both values; it rotates with rope_kv_kernel's
// own rope_rotate_pair (common.h) and f32 table rows on the bf16-ROUNDED
// projection, so the result is bit-identical to the GEMV followed by
// rope_kv, and writes
//   q pair -> y
//   k pair -> y and the cache row of `pos`
//   v pair -> y and the cache row of `pos` (unrotated).
#pragma once

#include "common.h"
#include "launchers.h"  // RopeKvArgs: the launchers take it, the kernels too

struct RopeKvPre {
  float c, s;          // this pair's cos/sin at pos
  ushort_t *cache;     // cache address of the pair (null for q rows)
  bool rotate;         // q and k rows
};

// Everything the epilogue needs from memory, issued BEFORE the weight loop
// so the pos -> page entry -> table-row chain hides under the weight stream
// (a dependent load after the loop lands on the kernel tail). n_even is the
// wave's even output row; all values are wave-uniform. `pos` indexes the
// page table and the cos/sin tables unchecked when it comes from pos_ptr,
// the same trust rope_kv_kernel places in the device word (the host checks
// a scalar pos). cos/sin are loaded for v rows too, which never use them:
// the index is in range and an unconditional load keeps the prefetch
// branch-free.
DEVINL RopeKvPre rope_kv_prefetch(const RopeKvArgs &a, int n_even) {
  const int pos = a.pos_ptr ? *a.pos_ptr : a.pos;
  const int half = a.hd / 2;
  const int slot = n_even / a.hd;  // head slot in [q | k | v]
  const int d = n_even - slot * a.hd;
  const int phys = a.page_table[pos / a.page];
  const size_t cache_row =
      ((size_t)phys * a.page + (pos % a.page)) * a.kh * a.hd;
  RopeKvPre r;
  r.c = a.cost[(size_t)pos * half + (d >> 1)];
  r.s = a.sint[(size_t)pos * half + (d >> 1)];
  r.rotate = slot < a.hq + a.kh;
  if (slot < a.hq)
    r.cache = nullptr;
  else if (r.rotate)
    r.cache = a.kc + cache_row + (size_t)(slot - a.hq) * a.hd + d;
  else
    r.cache = a.vc + cache_row + (size_t)(slot - a.hq - a.kh) * a.hd + d;
  return r;
}

// `val` is the finished fp32 projection of the lane's row (valid in every
// lane of its 32-lane half after the xor reduce). Rounds to bf16 first, as
// the unfused GEMV's store does.
DEVINL void rope_kv_store(const RopeKvPre &pre, ushort_t *__restrict__ y,
                          int n_even, float val, int lane) {
  const uint32_t mine = f32_to_bf16(val);
  const uint32_t other = (uint32_t)__shfl_xor((int)mine, 32, WAVE);
  if (lane != 0) return;
  uint32_t pair = mine | (other << 16);  // (even, odd)
  if (pre.rotate) {
    const float ev = bf16_to_f32((ushort_t)mine);
    const float od = bf16_to_f32((ushort_t)other);
    pair = rope_rotate_pair(ev, od, pre.c, pre.s);
  }
  *(uint32_t *)(y + n_even) = pair;
  if (pre.cache) *(uint32_t *)pre.cache = pair;
}
