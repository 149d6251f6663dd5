// Torch extension bindings for the gfx950 kernels.
//
// Contracts mirror ops/torch_ref.py exactly (shapes/dtypes documented
// there). All activations are bf16, RoPE tables f32, workspace fp32.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "launchers.h"

static hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

// --------------------------------------------------------------------------
// Persistent workspace for the split-KV decode attention, keyed by the KV
// CACHE pointer: one engine owns one cache, and the engine's generate lock
// serializes all work touching it (eager kernels and graph replays alike),
// so a per-cache scratch set is race-free — and unlike stream-keyed
// scratch it cannot alias when torch's 32-entry stream pool hands two
// engines the same underlying stream. Grown buffers retire the old tensor
// into a keep-alive list because a previously captured graph may still
// replay with the old pointer.
struct CacheWS {
  torch::Tensor attn_ws;   // fp32 scratch: decode-attention m/l/acc
  std::vector<torch::Tensor> retired;
};
static std::mutex g_ws_mu;
static std::unordered_map<void*, CacheWS> g_ws;

// The m | l | acc scratch of a decode call on cache `kc`: khnsg * (2 + hd)
// floats (khnsg = kh * n_splits * group), grown on demand.
static float* decode_workspace(const torch::Tensor& kc, int64_t khnsg, int hd,
                               const torch::Device& dev) {
  const int64_t elems = khnsg * (2 + hd);
  std::lock_guard<std::mutex> lk(g_ws_mu);
  CacheWS& w = g_ws[kc.data_ptr()];
  if (!w.attn_ws.defined() || w.attn_ws.numel() < elems) {
    if (w.attn_ws.defined()) w.retired.push_back(w.attn_ws);
    w.attn_ws =
        torch::empty({std::max<int64_t>(elems, 64)},
                     torch::TensorOptions().dtype(at::kFloat).device(dev));
  }
  return w.attn_ws.data_ptr<float>();
}

#define CHECK_BF16_CUDA(t)                                                 \
  TORCH_CHECK((t).is_cuda(), #t " must be on GPU");                        \
  TORCH_CHECK((t).scalar_type() == at::kBFloat16, #t " must be bf16");

static const ushort_t* uptr(const torch::Tensor& t) {
  return reinterpret_cast<const ushort_t*>(t.data_ptr());
}
static ushort_t* uptr_mut(torch::Tensor& t) {
  return reinterpret_cast<ushort_t*>(t.data_ptr());
}

// --------------------------------------------------------------------------
// Argument checkers shared by every op that takes these tensors, host-
// position and graph-mode (pos_state) calls alike. Tensor metadata only:
// nothing here reads the device, synchronizes, allocates or launches, so
// nothing is added to a captured graph.

using OptTensor = c10::optional<torch::Tensor>;

// Graph mode keeps the position in a device int32 word; returns its address,
// or nullptr for a host-position call.
static const int* check_pos_state(const char* who, const OptTensor& pos_state) {
  if (!pos_state.has_value()) return nullptr;
  TORCH_CHECK(pos_state->is_cuda() && pos_state->scalar_type() == at::kInt &&
                  pos_state->numel() >= 1,
              who, ": pos_state must be a device int32 word");
  return pos_state->data_ptr<int>();
}

// A host position range [pos0, pos0 + t) must lie inside the cos/sin tables
// (when given) and inside what the page table maps. A device position is
// trusted: checking it would mean reading it.
static void check_host_pos(const char* who, int64_t pos0, int64_t t,
                           const torch::Tensor* cost,
                           const torch::Tensor* page_table, int64_t page) {
  TORCH_CHECK(pos0 >= 0 && (!cost || pos0 + t <= cost->size(0)) &&
                  (!page_table || pos0 + t <= page_table->numel() * page),
              who, ": pos inside the rope table and the page table");
}

static void check_rope_tables(const char* who, const torch::Tensor& cost,
                              const torch::Tensor& sint, int hd) {
  TORCH_CHECK(cost.is_cuda() && sint.is_cuda() &&
                  cost.scalar_type() == at::kFloat &&
                  sint.scalar_type() == at::kFloat,
              who, ": cos/sin tables f32 on GPU");
  TORCH_CHECK(cost.dim() == 2 && cost.is_contiguous() &&
                  sint.is_contiguous() && cost.sizes() == sint.sizes() &&
                  cost.size(1) == hd / 2,
              who, ": cos/sin tables [max_pos, hd/2] contiguous");
}

// q [t, hq, hd], k [t, hk, hd] and (when given) v [t, hk, hd]: bf16, possibly
// strided VIEWS of the fused QKV output — an arbitrary row stride, but
// contiguous head and dim dims.
static void check_qkv_views(const char* who, const torch::Tensor& q,
                            const torch::Tensor& k, const torch::Tensor* v) {
  for (const torch::Tensor* x : {&q, &k, v}) {
    if (!x) continue;
    TORCH_CHECK(x->is_cuda() && x->scalar_type() == at::kBFloat16 &&
                    x->dim() == 3,
                who, ": q/k/v bf16 [t, heads, hd] on GPU");
    TORCH_CHECK(x->stride(2) == 1, who, ": dim contiguous");
    TORCH_CHECK(x->stride(1) == x->size(2), who, ": head dim contiguous");
    TORCH_CHECK(x->size(0) == q.size(0) && x->size(2) == q.size(2), who,
                ": q/k/v row and head shapes");
  }
  TORCH_CHECK(!v || v->size(1) == k.size(1), who,
              ": q/k/v row and head shapes");
}

// bf16 paged cache: kc/vc [n_pages, page, kh, hd] + int32 page table.
static void check_kv_cache(const char* who, const torch::Tensor& kc,
                           const torch::Tensor& vc,
                           const torch::Tensor& page_table) {
  TORCH_CHECK(kc.is_cuda() && vc.is_cuda() && page_table.is_cuda(), who,
              ": cache and page table must be on GPU");
  TORCH_CHECK(kc.scalar_type() == at::kBFloat16 &&
                  vc.scalar_type() == at::kBFloat16,
              who, ": cache must be bf16");
  TORCH_CHECK(kc.dim() == 4 && kc.is_contiguous() && vc.is_contiguous() &&
                  kc.sizes() == vc.sizes(),
              who, ": caches contiguous [n_pages, page, kh, hd], same shape");
  TORCH_CHECK(page_table.scalar_type() == at::kInt && page_table.dim() == 1 &&
                  page_table.is_contiguous(),
              who, ": page_table int32 [n_logical_pages]");
}

// fp8 (e4m3fn) paged cache: kc/vc uint8 [n_pages, page, kh, hd], ksc/vsc f32
// [n_pages, kh, page] (kv_fp8.hip).
static void check_fp8_cache(const char* who, const torch::Tensor& kc,
                            const torch::Tensor& vc, const torch::Tensor& ksc,
                            const torch::Tensor& vsc,
                            const torch::Tensor& page_table) {
  TORCH_CHECK(kc.is_cuda() && vc.is_cuda() && ksc.is_cuda() && vsc.is_cuda() &&
                  page_table.is_cuda(),
              who, ": cache, scales and page table must be on GPU");
  TORCH_CHECK(kc.scalar_type() == at::kByte && vc.scalar_type() == at::kByte,
              who, ": fp8 cache must be uint8 (e4m3fn bytes)");
  TORCH_CHECK(ksc.scalar_type() == at::kFloat &&
                  vsc.scalar_type() == at::kFloat,
              who, ": cache scales must be f32");
  TORCH_CHECK(kc.dim() == 4 && kc.is_contiguous() && vc.is_contiguous() &&
                  kc.sizes() == vc.sizes(),
              who, ": caches contiguous [n_pages, page, kh, hd], same shape");
  TORCH_CHECK(ksc.dim() == 3 && ksc.is_contiguous() && vsc.is_contiguous() &&
                  ksc.sizes() == vsc.sizes() && ksc.size(0) == kc.size(0) &&
                  ksc.size(1) == kc.size(2) && ksc.size(2) == kc.size(1),
              who, ": scales contiguous [n_pages, kh, page]");
  const int64_t hd = kc.size(3);
  TORCH_CHECK(hd == 32 || hd == 64 || hd == 128, who, ": hd in {32, 64, 128}");
  TORCH_CHECK(page_table.scalar_type() == at::kInt && page_table.dim() == 1 &&
                  page_table.is_contiguous(),
              who, ": page_table int32 [n_logical_pages]");
}

// k (and v) rows must fit the cache they are appended to.
static void check_cache_matches(const char* who, const torch::Tensor& kc,
                                const torch::Tensor& k) {
  TORCH_CHECK(kc.size(2) == k.size(1) && kc.size(3) == k.size(2), who,
              ": cache [.., kh, hd] must match k");
}

// --------------------------------------------------------------------------

torch::Tensor rmsnorm(torch::Tensor x, torch::Tensor w, double eps,
                      OptTensor out) {
  CHECK_BF16_CUDA(x);
  CHECK_BF16_CUDA(w);
  auto xc = x.contiguous();
  auto wc = w.contiguous();
  const int d = xc.size(-1);
  const int t = xc.numel() / d;
  TORCH_CHECK(d % 8 == 0, "rmsnorm: d must be a multiple of 8");
  auto y = out.has_value() ? *out : torch::empty_like(xc);
  launch_rmsnorm(uptr(xc), uptr(wc), uptr_mut(y), t, d, (float)eps,
                 cur_stream());
  return y;
}

std::tuple<torch::Tensor, torch::Tensor> add_rmsnorm(
    torch::Tensor resid, torch::Tensor delta, torch::Tensor w, double eps,
    OptTensor out_resid, OptTensor out_y) {
  CHECK_BF16_CUDA(resid);
  CHECK_BF16_CUDA(delta);
  CHECK_BF16_CUDA(w);
  auto rc = resid.contiguous();
  auto dc = delta.contiguous();
  auto wc = w.contiguous();
  const int d = rc.size(-1);
  const int t = rc.numel() / d;
  TORCH_CHECK(d % 8 == 0, "add_rmsnorm: d must be a multiple of 8");
  auto r_out = out_resid.has_value() ? *out_resid : torch::empty_like(rc);
  auto y = out_y.has_value() ? *out_y : torch::empty_like(rc);
  launch_add_rmsnorm(uptr(rc), uptr(dc), uptr(wc), uptr_mut(r_out),
                     uptr_mut(y), t, d, (float)eps, cur_stream());
  return {r_out, y};
}

// RoPE in place on q/k (interleaved pairs, table-driven). pos_state (int32[1]
// on device) replaces pos0 in graph mode.
void rope_inplace(torch::Tensor q, torch::Tensor k, torch::Tensor cost,
                  torch::Tensor sint, int64_t pos0,
                  const OptTensor& pos_state) {
  check_qkv_views("rope", q, k, nullptr);
  const int t = q.size(0), hq = q.size(1), hd = q.size(2);
  const int hk = k.size(1);
  TORCH_CHECK(hd % 2 == 0, "rope: hd even");
  check_rope_tables("rope", cost, sint, hd);
  const int* pp = check_pos_state("rope", pos_state);
  if (!pp) check_host_pos("rope", pos0, t, &cost, nullptr, 0);
  launch_rope(uptr_mut(q), uptr_mut(k), cost.data_ptr<float>(),
              sint.data_ptr<float>(), t, hq, hk, hd, (int)pos0,
              q.stride(0), k.stride(0), pp, cur_stream());
}

// Fused RoPE + paged KV scatter: rotate q/k in place AND write the rotated
// k plus v into the page pool in one launch (saves a kernel + a K re-read
// per layer on the kernel-count-bound decode path).
void rope_kv(torch::Tensor q, torch::Tensor k, torch::Tensor v,
             torch::Tensor cost, torch::Tensor sint, torch::Tensor kc,
             torch::Tensor vc, torch::Tensor page_table, int64_t pos0,
             const OptTensor& pos_state) {
  check_qkv_views("rope_kv", q, k, &v);
  check_kv_cache("rope_kv", kc, vc, page_table);
  check_cache_matches("rope_kv", kc, k);
  const int t = q.size(0), hq = q.size(1), hd = q.size(2);
  const int hk = k.size(1);
  const int page = kc.size(1);
  TORCH_CHECK(hd % 16 == 0, "rope_kv: hd % 16 == 0");
  check_rope_tables("rope_kv", cost, sint, hd);
  const int* pp = check_pos_state("rope_kv", pos_state);
  if (!pp) check_host_pos("rope_kv", pos0, t, &cost, &page_table, page);
  launch_rope_kv(uptr_mut(q), uptr_mut(k), uptr(v), cost.data_ptr<float>(),
                 sint.data_ptr<float>(), uptr_mut(kc), uptr_mut(vc),
                 page_table.data_ptr<int>(), t, hq, hk, hd, (int)pos0,
                 q.stride(0), k.stride(0), v.stride(0), page, pp,
                 cur_stream());
}

torch::Tensor swiglu(torch::Tensor gate, torch::Tensor up, OptTensor out_opt) {
  CHECK_BF16_CUDA(gate);
  CHECK_BF16_CUDA(up);
  TORCH_CHECK(gate.dim() == 2 && up.dim() == 2);
  TORCH_CHECK(gate.stride(1) == 1 && up.stride(1) == 1,
              "swiglu: last dim must be contiguous");
  TORCH_CHECK(gate.stride(0) == up.stride(0),
              "swiglu: gate/up must share a row stride (gate_up halves)");
  const int t = gate.size(0), f = gate.size(1);
  TORCH_CHECK(f % 8 == 0);
  auto out = out_opt.has_value() ? *out_opt : torch::empty({t, f}, gate.options());
  launch_swiglu(uptr(gate), uptr(up), uptr_mut(out), t, f,
                (int)gate.stride(0), cur_stream());
  return out;
}

// Paged KV scatter of t fresh rows k, v [t, kh, hd] at pos0 (pos_state in
// graph mode).
void kv_write(torch::Tensor kc, torch::Tensor vc, torch::Tensor page_table,
              int64_t pos0, torch::Tensor k, torch::Tensor v,
              const OptTensor& pos_state) {
  check_kv_cache("kv_write", kc, vc, page_table);
  CHECK_BF16_CUDA(k);
  CHECK_BF16_CUDA(v);
  TORCH_CHECK(k.dim() == 3 && k.sizes() == v.sizes(),
              "kv_write: k, v [t, kh, hd], same shape");
  check_cache_matches("kv_write", kc, k);
  auto kq = k.contiguous();
  auto vq = v.contiguous();
  const int t = kq.size(0), kh = kq.size(1), hd = kq.size(2);
  const int page = kc.size(1);
  TORCH_CHECK((kh * hd) % 8 == 0, "kv_write: kh*hd % 8 == 0");
  const int* pp = check_pos_state("kv_write", pos_state);
  if (!pp) check_host_pos("kv_write", pos0, t, nullptr, &page_table, page);
  launch_kv_write(uptr(kq), uptr(vq), uptr_mut(kc), uptr_mut(vc),
                  page_table.data_ptr<int>(), (int)pos0, t, kh, hd,
                  page, pp, cur_stream());
}

torch::Tensor attn_prefill(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                           double scale, bool causal, int64_t kv_offset,
                           int64_t window) {
  CHECK_BF16_CUDA(q);
  CHECK_BF16_CUDA(k);
  CHECK_BF16_CUDA(v);
  auto qc = q.contiguous();
  auto kc = k.contiguous();
  auto vc = v.contiguous();
  const int tq = qc.size(0), hq = qc.size(1), hd = qc.size(2);
  const int tk = kc.size(0), kh = kc.size(1);
  TORCH_CHECK(hq % kh == 0, "GQA: hq % kh == 0");
  TORCH_CHECK(hd == 32 || hd == 64 || hd == 128, "hd in {32,64,128}");
  TORCH_CHECK(window >= 0 && window <= INT32_MAX,
              "attn_prefill: window >= 0");
  TORCH_CHECK(causal || window == 0,
              "attn_prefill: a sliding window needs causal=True");
  auto out = torch::empty_like(qc);
  // hd=128 causal takes the MFMA-tiled kernel; other head dims and the
  // non-causal path use the simple online-softmax kernel.
  int used_mfma = 0;
  if (hd == 128 && causal) {
    launch_attn_prefill_mfma(uptr(qc), uptr(kc), uptr(vc), uptr_mut(out), tq,
                             tk, (int)kv_offset, (float)scale, hq, kh, hd,
                             (int)window, cur_stream(), &used_mfma);
  }
  if (!used_mfma) {
    launch_attn_prefill_simple(uptr(qc), uptr(kc), uptr(vc), uptr_mut(out), tq,
                               tk, (int)kv_offset, (float)scale, hq, kh, hd,
                               causal ? 1 : 0, (int)window, cur_stream());
  }
  return out;
}

// Force the non-MFMA prefill (A/B + numerics anchor for tests).
torch::Tensor attn_prefill_simple(torch::Tensor q, torch::Tensor k,
                                  torch::Tensor v, double scale, bool causal,
                                  int64_t kv_offset) {
  CHECK_BF16_CUDA(q);
  auto qc = q.contiguous();
  auto kc = k.contiguous();
  auto vc = v.contiguous();
  const int tq = qc.size(0), hq = qc.size(1), hd = qc.size(2);
  const int tk = kc.size(0), kh = kc.size(1);
  auto out = torch::empty_like(qc);
  launch_attn_prefill_simple(uptr(qc), uptr(kc), uptr(vc), uptr_mut(out), tq,
                             tk, (int)kv_offset, (float)scale, hq, kh, hd,
                             causal ? 1 : 0, 0, cur_stream());
  return out;
}

// prefill-attention ablation launcher (perf diagnosis only)
torch::Tensor attn_prefill_ablate(torch::Tensor q, torch::Tensor k,
                                  torch::Tensor v, double scale,
                                  int64_t abl) {
  CHECK_BF16_CUDA(q);
  auto qc = q.contiguous();
  auto kc = k.contiguous();
  auto vc = v.contiguous();
  const int tq = qc.size(0), hq = qc.size(1), hd = qc.size(2);
  const int tk = kc.size(0), kh = kc.size(1);
  TORCH_CHECK(hd == 128, "ablation probe is hd=128 only");
  auto out = torch::empty_like(qc);
  launch_attn_prefill_mfma_abl(uptr(qc), uptr(kc), uptr(vc), uptr_mut(out),
                               tq, tk, (float)scale, hq, kh, (int)abl,
                               cur_stream());
  return out;
}

// MFMA fragment-map probe: D[16,16] = A[16,32] @ B[32,16].
torch::Tensor mfma_probe16(torch::Tensor a, torch::Tensor b) {
  CHECK_BF16_CUDA(a);
  CHECK_BF16_CUDA(b);
  auto ac = a.contiguous();
  auto bc = b.contiguous();
  TORCH_CHECK(ac.size(0) == 16 && ac.size(1) == 32);
  TORCH_CHECK(bc.size(0) == 32 && bc.size(1) == 16);
  auto d = torch::empty({16, 16}, torch::TensorOptions()
                                      .dtype(at::kFloat)
                                      .device(a.device()));
  launch_mfma_probe16(uptr(ac), uptr(bc), d.data_ptr<float>(), cur_stream());
  return d;
}

// Decode-attention split geometry. The split kernel's cost is dominated
// by per-wave SERIAL iterations (shfl-reduce + online-softmax chains), not
// KV bytes, so occupancy (total blocks) is the lever; ADVSPEC_SPLIT_BLOCKS
// overrides the target block count for A/B tuning on hardware.
// With a sliding window the kernel walks at most window + 63 positions (the
// window plus the part of its first 64-position tile below it), so the
// geometry is sized for that: it then depends on (bound, window, kh, target)
// and never on the live position.
static void split_geometry(long seq, int kh, int target_blocks, long window,
                           int* n_splits, int* split_len) {
  if (window > 0) seq = std::min(seq, window + 63);
  // Target-block precedence: ADVSPEC_SPLIT_BLOCKS env (explicit A/B
  // override) > per-call target_blocks (the engine picks by its live
  // concurrency: solo decode wants ~512 blocks of self-occupancy, several
  // co-resident opponents want 256 — bench A/B under 3-way bf16
  // concurrency: 256-target 0.594 critiques/s vs 512-target 0.581; fp8
  // prefers 512) > compiled default 256.
  static const int env_blocks = [] {
    const char* e = getenv("ADVSPEC_SPLIT_BLOCKS");
    return e ? atoi(e) : 0;
  }();
  const int cap_blocks =
      env_blocks > 0 ? env_blocks : (target_blocks > 0 ? target_blocks : 256);
  const int target = std::max(1, cap_blocks / kh);
  int ns = std::max(1, std::min((int)((seq + 63) / 64), target));
  int sl = (int)((seq + ns - 1) / ns + 63) / 64 * 64;
  *n_splits = (int)((seq + sl - 1) / sl);
  *split_len = sl;
}

// Geometry query for tests: the (n_splits, split_len) a decode call with
// these arguments launches (ADVSPEC_SPLIT_BLOCKS override included), so a
// test can assert the tile/split path it claims to exercise.
py::tuple decode_split_geometry(int64_t seq, int64_t kh,
                                int64_t split_blocks, int64_t window) {
  TORCH_CHECK(seq >= 1 && kh >= 1, "decode_split_geometry: seq, kh >= 1");
  TORCH_CHECK(window >= 0, "decode_split_geometry: window >= 0");
  int n_splits, split_len;
  split_geometry(seq, (int)kh, (int)split_blocks, window, &n_splits,
                 &split_len);
  return py::make_tuple(n_splits, split_len);
}

// Everything of a decode-attention call that is not the kernel launch, shared
// by the bf16 and fp8 entries (the caller has already run its cache checker):
// q and out handling, the split geometry, the per-cache workspace and the
// bound-versus-coverage check. `bound` is seq_len: the host length, or with
// pos_state the static bound (max_seq) that sizes the splits so the launch
// geometry is replay-stable; the true length is then *pos_state + 1
// in-kernel.
struct DecodeCall {
  torch::Tensor qc, out;
  DecodeSplitArgs a;
};
static DecodeCall decode_prepare(const char* who, const torch::Tensor& q,
                                 const torch::Tensor& kc,
                                 const torch::Tensor& page_table,
                                 int64_t bound, double scale,
                                 const OptTensor& pos_state,
                                 const OptTensor& out_opt, bool identity,
                                 int64_t split_blocks, int64_t window) {
  CHECK_BF16_CUDA(q);
  TORCH_CHECK(q.dim() == 2, who, ": q [hq, hd]");
  DecodeCall c;
  c.qc = q.contiguous();
  const int hq = c.qc.size(0), hd = c.qc.size(1);
  const int page = kc.size(1), kh = kc.size(2);
  TORCH_CHECK(kc.size(3) == hd, who, ": q and cache head dims differ");
  TORCH_CHECK(hd == 32 || hd == 64 || hd == 128, who, ": hd in {32, 64, 128}");
  TORCH_CHECK(hq % kh == 0 && hq / kh <= 8, who, ": GQA group <= 8");
  const int group = hq / kh;
  const int64_t covered =
      (identity ? kc.size(0) : page_table.numel()) * (int64_t)page;
  TORCH_CHECK(bound >= 1 && bound <= covered, who,
              ": seq_len outside the cache");
  TORCH_CHECK(window >= 0, who, ": window >= 0");
  // a window of the whole bound or more is no window; this also keeps the
  // kernel's int32 argument in range
  if (window >= bound) window = 0;
  const int* pos_ptr = check_pos_state(who, pos_state);
  if (out_opt.has_value()) {
    c.out = *out_opt;
    TORCH_CHECK(c.out.is_cuda() && c.out.scalar_type() == at::kBFloat16 &&
                    c.out.is_contiguous() &&
                    c.out.numel() == (int64_t)hq * hd,
                who, ": out must be contiguous bf16 [hq, hd]");
  } else {
    c.out = torch::empty({hq, hd}, c.qc.options());
  }
  int n_splits, split_len;
  split_geometry(bound, kh, (int)split_blocks, window, &n_splits,
                 &split_len);
  const long khnsg = (long)kh * n_splits * group;
  float* ws = decode_workspace(kc, khnsg, hd, q.device());
  c.a = {page_table.data_ptr<int>(), pos_ptr, (int)bound, (float)scale, kh,
         group, hd, page, split_len, n_splits, ws, ws + khnsg,
         ws + 2 * khnsg, identity ? 1 : 0, (int)window};
  return c;
}

torch::Tensor attn_decode_paged(torch::Tensor q, torch::Tensor kc,
                                torch::Tensor vc, torch::Tensor page_table,
                                int64_t seq_len, double scale,
                                const OptTensor& pos_state,
                                const OptTensor& out, bool identity,
                                int64_t split_blocks, int64_t window) {
  check_kv_cache("attn_decode_paged", kc, vc, page_table);
  DecodeCall c =
      decode_prepare("attn_decode_paged", q, kc, page_table, seq_len, scale,
                     pos_state, out, identity, split_blocks, window);
  launch_attn_decode_split(uptr(c.qc), uptr(kc), uptr(vc), c.a,
                           uptr_mut(c.out), cur_stream());
  return c.out;
}

// Same over an fp8 cache; the dequantization is folded into the split kernel.
torch::Tensor attn_decode_paged_fp8(torch::Tensor q, torch::Tensor kc,
                                    torch::Tensor vc, torch::Tensor ksc,
                                    torch::Tensor vsc,
                                    torch::Tensor page_table, int64_t seq_len,
                                    double scale, const OptTensor& pos_state,
                                    const OptTensor& out, bool identity,
                                    int64_t split_blocks, int64_t window) {
  check_fp8_cache("attn_decode_paged_fp8", kc, vc, ksc, vsc, page_table);
  DecodeCall c =
      decode_prepare("attn_decode_paged_fp8", q, kc, page_table, seq_len,
                     scale, pos_state, out, identity, split_blocks, window);
  launch_attn_decode_split_fp8(uptr(c.qc), kc.data_ptr<uint8_t>(),
                               vc.data_ptr<uint8_t>(), ksc.data_ptr<float>(),
                               vsc.data_ptr<float>(), c.a, uptr_mut(c.out),
                               cur_stream());
  return c.out;
}

// Async variant: write the sampled token id into out[idx] (int32, on
// device) without any host synchronization — the decode loop stays on the
// GPU and the host checks stop conditions every N tokens.
void sample_to(torch::Tensor logits, double temp, int64_t seed,
               torch::Tensor out, int64_t idx) {
  CHECK_BF16_CUDA(logits);
  TORCH_CHECK(out.scalar_type() == at::kInt && out.is_cuda());
  auto lc = logits.contiguous();
  launch_sample(uptr(lc), (int)lc.numel(), (float)temp, (uint32_t)seed,
                out.data_ptr<int>() + idx, cur_stream());
}

// Decode GEMV: y = x @ w for batch-1 x. Streams w once at HBM rate
// (hipBLASLt batch-1 measured 0.9-1.7 TB/s; this path targets ~5 TB/s).
torch::Tensor gemv(torch::Tensor x, torch::Tensor w,
                   OptTensor out_opt) {
  // y = x @ w^T with w stored row-major [N, K] (HF layout)
  CHECK_BF16_CUDA(x);
  CHECK_BF16_CUDA(w);
  TORCH_CHECK(w.dim() == 2 && w.is_contiguous());
  const int N = w.size(0), K = w.size(1);
  TORCH_CHECK((long)x.numel() == (long)K, "gemv: x numel == K");
  TORCH_CHECK(K % 8 == 0, "gemv: K % 8 == 0");
  auto xc = x.contiguous();
  auto y = out_opt.has_value()
               ? *out_opt
               : torch::empty(x.dim() == 2 ? std::vector<int64_t>{1, N}
                                           : std::vector<int64_t>{N},
                              x.options());
  launch_gemv(uptr(xc), uptr(w), uptr_mut(y), K, N, cur_stream());
  return y;
}

// Fused decode gate_up GEMV + SwiGLU: act = silu(x@Wg^T) * (x@Wu^T) with
// W = [gate | up] rows (the fused w_gate_up layout). Allocation-free.
void gemv_gateup(torch::Tensor x, torch::Tensor w, torch::Tensor act) {
  CHECK_BF16_CUDA(x);
  CHECK_BF16_CUDA(w);
  CHECK_BF16_CUDA(act);
  TORCH_CHECK(w.dim() == 2 && w.is_contiguous());
  const int K = w.size(1), F2 = w.size(0);
  TORCH_CHECK(F2 % 2 == 0 && (long)x.numel() == (long)K && K % 8 == 0);
  TORCH_CHECK((long)act.numel() == (long)(F2 / 2));
  auto xc = x.contiguous();
  launch_gemv_gateup(uptr(xc), uptr(w), uptr_mut(act), K, F2 / 2,
                     cur_stream());
}

// rmsnorm fused into the GEMV prologue: y = rms(x) * ((x*wln) @ w^T).
// Replaces the separate (add_)rmsnorm launch before every consuming decode
// GEMV (see gemv.hip fusion comment).
torch::Tensor gemv_norm(torch::Tensor x, torch::Tensor wln, torch::Tensor w,
                        double eps, OptTensor out_opt) {
  CHECK_BF16_CUDA(x);
  CHECK_BF16_CUDA(wln);
  CHECK_BF16_CUDA(w);
  TORCH_CHECK(w.dim() == 2 && w.is_contiguous());
  const int N = w.size(0), K = w.size(1);
  TORCH_CHECK((long)x.numel() == (long)K, "gemv_norm: x numel == K");
  TORCH_CHECK((long)wln.numel() == (long)K, "gemv_norm: wln numel == K");
  TORCH_CHECK(K % 8 == 0, "gemv_norm: K % 8 == 0");
  TORCH_CHECK(K <= 32768, "gemv_norm: LDS xl staging caps K at 32768");
  auto xc = x.contiguous();
  auto lc = wln.contiguous();
  auto y = out_opt.has_value()
               ? *out_opt
               : torch::empty(x.dim() == 2 ? std::vector<int64_t>{1, N}
                                           : std::vector<int64_t>{N},
                              x.options());
  TORCH_CHECK((long)y.numel() == (long)N, "gemv_norm: out numel == N");
  launch_gemv_norm(uptr(xc), uptr(lc), uptr(w), uptr_mut(y), K, N,
                   (float)eps, cur_stream());
  return y;
}

// Preconditions shared by the two qkv GEMVs whose epilogue rotates and
// appends to the KV cache (rope_epilogue.h). Returns the epilogue operands;
// a shape outside them belongs on the gemv + rope_kv pair.
static RopeKvArgs check_rope_kv_epilogue(
    const char* op, int N, int64_t hq, int64_t kh, const torch::Tensor& cost,
    const torch::Tensor& sint, torch::Tensor& kc, torch::Tensor& vc,
    const torch::Tensor& page_table, int64_t pos0, const OptTensor& pos_state,
    const torch::Tensor& y) {
  TORCH_CHECK(hq >= 1 && kh >= 1 && N % (hq + 2 * kh) == 0, op,
              ": N == (hq + 2*kh)*hd");
  const int hd = N / (int)(hq + 2 * kh);
  TORCH_CHECK(hd % 16 == 0, op, ": hd % 16 == 0");
  TORCH_CHECK(N <= 8192, op, ": w32 geometry only (N <= 8192)");
  check_rope_tables(op, cost, sint, hd);
  check_kv_cache(op, kc, vc, page_table);
  TORCH_CHECK(kc.size(2) == kh && kc.size(3) == hd, op,
              ": caches [n_pages, page, kh, hd]");
  const int page = kc.size(1);
  const int* pp = check_pos_state(op, pos_state);
  if (!pp) check_host_pos(op, pos0, 1, &cost, &page_table, page);
  CHECK_BF16_CUDA(y);
  TORCH_CHECK(y.is_contiguous() && (long)y.numel() == (long)N, op,
              ": out contiguous, numel == N");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(y.data_ptr()) % 4 == 0, op,
              ": out 4-byte aligned (pairs are stored as one word)");
  return {cost.data_ptr<float>(), sint.data_ptr<float>(), uptr_mut(kc),
          uptr_mut(vc), page_table.data_ptr<int>(), pp, (int)pos0, (int)hq,
          (int)kh, hd, page};
}

// qkv projection + RoPE + KV append in one launch (bf16 weights):
//   y = rmsnorm(x, wln) @ w^T, then q/k pairs rotated at pos, rotated k and
//   v written to the cache row of pos — bit-identical to gemv_norm followed
//   by rope_kv on the q/k/v views of y.
torch::Tensor gemv_norm_rope_kv(
    torch::Tensor x, torch::Tensor wln, torch::Tensor w, double eps,
    torch::Tensor cost, torch::Tensor sint, torch::Tensor kc, torch::Tensor vc,
    torch::Tensor page_table, int64_t pos0, int64_t hq, int64_t kh,
    const OptTensor& pos_state,
    OptTensor out_opt) {
  CHECK_BF16_CUDA(x);
  CHECK_BF16_CUDA(wln);
  CHECK_BF16_CUDA(w);
  TORCH_CHECK(w.dim() == 2 && w.is_contiguous());
  const int N = w.size(0), K = w.size(1);
  TORCH_CHECK((long)x.numel() == (long)K, "gemv_norm_rope_kv: x numel == K");
  TORCH_CHECK((long)wln.numel() == (long)K,
              "gemv_norm_rope_kv: wln numel == K");
  TORCH_CHECK(K % 8 == 0, "gemv_norm_rope_kv: K % 8 == 0");
  TORCH_CHECK(K <= 32768, "gemv_norm_rope_kv: LDS xl staging caps K at 32768");
  auto xc = x.contiguous();
  auto lc = wln.contiguous();
  auto y = out_opt.has_value() ? *out_opt : torch::empty({1, N}, x.options());
  const RopeKvArgs ra = check_rope_kv_epilogue(
      "gemv_norm_rope_kv", N, hq, kh, cost, sint, kc, vc, page_table, pos0,
      pos_state, y);
  launch_gemv_norm_rope_kv(uptr(xc), uptr(lc), uptr(w), uptr_mut(y), K,
                           (float)eps, ra, cur_stream());
  return y;
}

// fp8 twin: pre-quantized x8/xs (quant_norm_fp8) against rowwise-e4m3 w8 —
// bit-identical to gemv_fp8_q followed by rope_kv.
void gemv_fp8_q_rope_kv(torch::Tensor x8, torch::Tensor xs, torch::Tensor w8,
                        torch::Tensor wsc, torch::Tensor out,
                        torch::Tensor cost, torch::Tensor sint,
                        torch::Tensor kc, torch::Tensor vc,
                        torch::Tensor page_table, int64_t pos0, int64_t hq,
                        int64_t kh,
                        const OptTensor& pos_state) {
  TORCH_CHECK(w8.dim() == 2 && w8.is_contiguous() && w8.is_cuda() &&
              w8.scalar_type() == at::kByte);
  const int N = w8.size(0), K = w8.size(1);
  TORCH_CHECK(K % 16 == 0, "gemv_fp8_q_rope_kv: K % 16 == 0");
  TORCH_CHECK(x8.is_cuda() && x8.numel() >= K &&
              x8.scalar_type() == at::kByte && x8.is_contiguous());
  TORCH_CHECK(xs.is_cuda() && xs.numel() >= 1 &&
              xs.scalar_type() == at::kFloat);
  TORCH_CHECK(wsc.is_cuda() && wsc.numel() >= N &&
              wsc.scalar_type() == at::kFloat && wsc.is_contiguous());
  const RopeKvArgs ra = check_rope_kv_epilogue(
      "gemv_fp8_q_rope_kv", N, hq, kh, cost, sint, kc, vc, page_table, pos0,
      pos_state, out);
  launch_gemv_fp8_rope_kv(x8.data_ptr<uint8_t>(), xs.data_ptr<float>(),
                          w8.data_ptr<uint8_t>(), wsc.data_ptr<float>(),
                          uptr_mut(out), K, ra, cur_stream());
}

// residual-add fused into the GEMV epilogue: resid += x @ w^T (in place).
// NOT valid under TP (the all-reduce needs the raw partial product).
void gemv_res(torch::Tensor x, torch::Tensor w, torch::Tensor resid) {
  CHECK_BF16_CUDA(x);
  CHECK_BF16_CUDA(w);
  CHECK_BF16_CUDA(resid);
  TORCH_CHECK(w.dim() == 2 && w.is_contiguous());
  const int N = w.size(0), K = w.size(1);
  TORCH_CHECK((long)x.numel() == (long)K && K % 8 == 0);
  TORCH_CHECK((long)resid.numel() == (long)N, "gemv_res: resid numel == N");
  TORCH_CHECK(resid.is_contiguous());
  TORCH_CHECK(N <= 8192, "gemv_res: w32 kernel only (hidden <= 8192)");
  auto xc = x.contiguous();
  launch_gemv_res(uptr(xc), uptr(w), uptr_mut(resid), K, N, cur_stream());
}

// rmsnorm + gate_up GEMV + SwiGLU in one launch (decode MLP front half).
void gemv_gateup_norm(torch::Tensor x, torch::Tensor wln, torch::Tensor w,
                      double eps, torch::Tensor act) {
  CHECK_BF16_CUDA(x);
  CHECK_BF16_CUDA(wln);
  CHECK_BF16_CUDA(w);
  CHECK_BF16_CUDA(act);
  TORCH_CHECK(w.dim() == 2 && w.is_contiguous());
  const int K = w.size(1), F2 = w.size(0);
  TORCH_CHECK(F2 % 2 == 0 && (long)x.numel() == (long)K && K % 8 == 0);
  TORCH_CHECK((long)wln.numel() == (long)K);
  TORCH_CHECK((long)act.numel() == (long)(F2 / 2));
  TORCH_CHECK(K <= 32768, "gemv_gateup_norm: LDS xl staging caps K at 32768");
  auto xc = x.contiguous();
  auto lc = wln.contiguous();
  launch_gemv_gateup_norm(uptr(xc), uptr(lc), uptr(w), uptr_mut(act), K,
                          F2 / 2, (float)eps, cur_stream());
}

// The 8-phase 256^2 tile loop for prefill-sized shapes (its counted-vmcnt
// schedule needs K % 128 == 0 and K >= 512, and it
// pays off when the M/N tiles fill); the 128^2 loop covers everything else.
// One rule for the bf16 and the fp8 GEMM.
static bool use_gemm256(int M, int N, int K) {
  return M > 128 && N >= 256 && K >= 512 && (K % 128) == 0;
}

// Operands of the bf16 prefill GEMMs, checked before anything is allocated
// or launched. The kernels stage A and B in 16-byte chunks of 8 elements, so
// K % 8 == 0 keeps every row 16-byte aligned and leaves no sub-chunk tail
// (gemm_tiles.h, "K contract": stage_edge has no element-wise arm).
static void check_gemm_operands(const char* who, const torch::Tensor& a,
                                const torch::Tensor& b) {
  TORCH_CHECK(a.is_cuda() && a.scalar_type() == at::kBFloat16 && a.dim() == 2,
              who, ": a bf16 [M, K] on GPU");
  TORCH_CHECK(b.is_cuda() && b.scalar_type() == at::kBFloat16 && b.dim() == 2,
              who, ": b bf16 [N, K] (row-major weights) on GPU");
  TORCH_CHECK(a.size(1) == b.size(1), who, ": K mismatch");
  TORCH_CHECK(a.size(1) % 8 == 0, who, ": K % 8 == 0");
}

// Tiled MFMA GEMM: C = A @ B, bf16, fp32 accumulation. Replaces library
// GEMMs on the prefill path (deterministic, workspace-free; see gemm_tiles.h).
torch::Tensor gemm(torch::Tensor a, torch::Tensor b) {
  // C = a @ b^T with b stored row-major [N, K] (HF layout)
  check_gemm_operands("gemm", a, b);
  auto ac = a.contiguous();
  auto bc = b.contiguous();
  const int M = ac.size(0), K = ac.size(1), N = bc.size(0);
  auto c = torch::empty({M, N}, ac.options());
  if (use_gemm256(M, N, K)) {
    launch_gemm256(uptr(ac), uptr(bc), uptr_mut(c), M, N, K, cur_stream());
  } else {
    launch_gemm(uptr(ac), uptr(bc), uptr_mut(c), M, N, K, cur_stream());
  }
  return c;
}

// Force a specific GEMM kernel (128 = two-barrier tile, 256 = 8-phase
// deep-pipelined) — A/B microbenches and the race screen; production code
// uses gemm()'s dispatcher.
torch::Tensor gemm_variant(torch::Tensor a, torch::Tensor b, int64_t which) {
  check_gemm_operands("gemm_variant", a, b);
  TORCH_CHECK(which == 128 || which == 256,
              "gemm_variant: which is 128 or 256");
  TORCH_CHECK(which == 128 || (a.size(1) >= 512 && a.size(1) % 128 == 0),
              "gemm256 needs K%128==0, K>=512");
  auto ac = a.contiguous();
  auto bc = b.contiguous();
  const int M = ac.size(0), K = ac.size(1), N = bc.size(0);
  auto c = torch::empty({M, N}, ac.options());
  if (which == 256) {
    launch_gemm256(uptr(ac), uptr(bc), uptr_mut(c), M, N, K, cur_stream());
  } else {
    launch_gemm(uptr(ac), uptr(bc), uptr_mut(c), M, N, K, cur_stream());
  }
  return c;
}

// MFMA issue-rate microbench (bf16 vs non-scaled fp8 16x16x32): the
// config-5 fp8-attention decision evidence (see mfma_rate.hip header).
void mfma_rate(torch::Tensor seed, torch::Tensor out, int64_t which,
               int64_t blocks) {
  CHECK_BF16_CUDA(seed);
  launch_mfma_rate(uptr(seed), out.data_ptr<float>(), (int)which,
                   (int)blocks, cur_stream());
}

// Row-quantize bf16 [M,K] to OCP e4m3 + per-row scale (scale = rowmax/448).
void quant_fp8(torch::Tensor x, torch::Tensor q, torch::Tensor scale) {
  CHECK_BF16_CUDA(x);
  TORCH_CHECK(q.scalar_type() == at::kByte && scale.scalar_type() == at::kFloat);
  auto xc = x.contiguous();
  const int K = xc.size(-1), M = xc.numel() / K;
  TORCH_CHECK(K % 8 == 0, "quant_fp8: K % 8 == 0");
  launch_quant_fp8(uptr(xc), q.data_ptr<uint8_t>(), scale.data_ptr<float>(),
                   M, K, cur_stream());
}

// Operands shared by the fp8 GEMM and the fp8 decode GEMVs, checked before
// any launch. The kernels stream w8 and x8 in 16-byte chunks of 16 codes
// (nc = K / 16), so a K that is no multiple of 16 would silently drop the row
// tails (and, in the GEMM, leave its 16-byte loads only 8-byte aligned;
// gemm_tiles.h, "K contract": stage_edge copies whole chunks, no byte loop).
static void check_fp8_weight(const char* who, const torch::Tensor& w8,
                             const torch::Tensor& wsc) {
  TORCH_CHECK(w8.is_cuda() && w8.scalar_type() == at::kByte && w8.dim() == 2 &&
                  w8.is_contiguous(),
              who, ": w8 contiguous uint8 [N, K] (e4m3fn bytes) on GPU");
  TORCH_CHECK(w8.size(1) % 16 == 0, who, ": K % 16 == 0");
  TORCH_CHECK(wsc.is_cuda() && wsc.scalar_type() == at::kFloat &&
                  wsc.is_contiguous() && wsc.numel() >= w8.size(0),
              who, ": wsc contiguous f32, one scale per weight row, on GPU");
}

// fp8 GEMM: C = (x quantized rowwise) @ (w8 * wsc)^T; w8 row-major [N,K]
// e4m3 + per-row scale. x is quantized in here (eager prefill path).
torch::Tensor gemm_fp8(torch::Tensor x, torch::Tensor w8, torch::Tensor wsc) {
  CHECK_BF16_CUDA(x);
  TORCH_CHECK(x.dim() == 2, "gemm_fp8: x bf16 [M, K]");
  check_fp8_weight("gemm_fp8", w8, wsc);
  TORCH_CHECK(w8.size(1) == x.size(1), "gemm_fp8: K mismatch");
  auto xc = x.contiguous();
  const int M = xc.size(0), K = xc.size(1), N = w8.size(0);
  auto opts8 = torch::TensorOptions().dtype(at::kByte).device(x.device());
  auto optsf = torch::TensorOptions().dtype(at::kFloat).device(x.device());
  auto x8 = torch::empty({M, (long)K}, opts8);
  auto xs = torch::empty({M}, optsf);
  launch_quant_fp8(uptr(xc), x8.data_ptr<uint8_t>(), xs.data_ptr<float>(),
                   M, K, cur_stream());
  auto c = torch::empty({M, N}, xc.options());
  if (use_gemm256(M, N, K)) {
    launch_gemm_fp8_256(x8.data_ptr<uint8_t>(), xs.data_ptr<float>(),
                        w8.data_ptr<uint8_t>(), wsc.data_ptr<float>(),
                        uptr_mut(c), M, N, K, cur_stream());
  } else {
    launch_gemm_fp8(x8.data_ptr<uint8_t>(), xs.data_ptr<float>(),
                    w8.data_ptr<uint8_t>(), wsc.data_ptr<float>(),
                    uptr_mut(c), M, N, K, cur_stream());
  }
  return c;
}

// The quantized activation: x8 holds at least K codes (the decode workspace
// sizes it for the widest projection), xs[0] is its scale.
static void check_fp8_act(const char* who, const torch::Tensor& x8,
                          const torch::Tensor& xs, int64_t K) {
  TORCH_CHECK(x8.is_cuda() && x8.scalar_type() == at::kByte &&
                  x8.is_contiguous() && x8.numel() >= K,
              who, ": x8 contiguous uint8 on GPU, numel >= K");
  TORCH_CHECK(xs.is_cuda() && xs.scalar_type() == at::kFloat &&
                  xs.numel() >= 1,
              who, ": xs f32 on GPU, numel >= 1");
}

static void check_bf16_dst(const char* who, const torch::Tensor& dst,
                           int64_t n) {
  TORCH_CHECK(dst.is_cuda() && dst.scalar_type() == at::kBFloat16 &&
                  dst.is_contiguous() && dst.numel() == n,
              who, ": destination contiguous bf16 on GPU, one element per row");
}

// fp8 decode GEMV (allocation-free: caller provides the x8/xs scratch and
// the output — all preallocated in the DecodeWorkspace for graph capture).
void gemv_fp8(torch::Tensor x, torch::Tensor w8, torch::Tensor wsc,
              torch::Tensor x8, torch::Tensor xs, torch::Tensor out) {
  CHECK_BF16_CUDA(x);
  check_fp8_weight("gemv_fp8", w8, wsc);
  const int N = w8.size(0), K = w8.size(1);
  TORCH_CHECK((long)x.numel() == (long)K, "gemv_fp8: x numel == K");
  check_fp8_act("gemv_fp8", x8, xs, K);
  check_bf16_dst("gemv_fp8", out, N);
  auto xc = x.contiguous();
  launch_quant_fp8(uptr(xc), x8.data_ptr<uint8_t>(), xs.data_ptr<float>(),
                   1, K, cur_stream());
  launch_gemv_fp8(x8.data_ptr<uint8_t>(), xs.data_ptr<float>(),
                  w8.data_ptr<uint8_t>(), wsc.data_ptr<float>(),
                  uptr_mut(out), K, N, cur_stream());
}

// fp8 decode fusion (mirror of the bf16 gemv_norm/gemv_res fusion):

// rmsnorm + rowwise e4m3 quantize in one launch: x8 = fp8(rmsnorm(x,wln)),
// xs = the rowwise scale. Replaces (add_)rmsnorm + quant_fp8 on the fp8
// decode path.
void quant_norm_fp8(torch::Tensor x, torch::Tensor wln, torch::Tensor x8,
                    torch::Tensor xs, double eps) {
  CHECK_BF16_CUDA(x);
  CHECK_BF16_CUDA(wln);
  auto xc = x.contiguous();
  const int K = xc.numel();
  TORCH_CHECK((long)wln.numel() == (long)K && K % 8 == 0);
  TORCH_CHECK(x8.numel() >= K && x8.scalar_type() == at::kByte);
  TORCH_CHECK(xs.numel() >= 1 && xs.scalar_type() == at::kFloat);
  launch_quant_norm_fp8(uptr(xc), uptr(wln), x8.data_ptr<uint8_t>(),
                        xs.data_ptr<float>(), K, (float)eps, cur_stream());
}

// pre-quantized fp8 GEMV (x8/xs from quant_norm_fp8): out = x8 @ w8^T
void gemv_fp8_q(torch::Tensor x8, torch::Tensor xs, torch::Tensor w8,
                torch::Tensor wsc, torch::Tensor out) {
  check_fp8_weight("gemv_fp8_q", w8, wsc);
  const int N = w8.size(0), K = w8.size(1);
  check_fp8_act("gemv_fp8_q", x8, xs, K);
  check_bf16_dst("gemv_fp8_q", out, N);
  launch_gemv_fp8(x8.data_ptr<uint8_t>(), xs.data_ptr<float>(),
                  w8.data_ptr<uint8_t>(), wsc.data_ptr<float>(),
                  uptr_mut(out), K, N, cur_stream());
}

// quantize + residual-epilogue fp8 GEMV: resid += (x @ w8^T) (in place).
// NOT valid under TP (the all-reduce needs the raw partial product).
void gemv_fp8_res(torch::Tensor x, torch::Tensor w8, torch::Tensor wsc,
                  torch::Tensor x8, torch::Tensor xs, torch::Tensor resid) {
  CHECK_BF16_CUDA(x);
  check_fp8_weight("gemv_fp8_res", w8, wsc);
  const int N = w8.size(0), K = w8.size(1);
  TORCH_CHECK((long)x.numel() == (long)K, "gemv_fp8_res: x numel == K");
  check_fp8_act("gemv_fp8_res", x8, xs, K);
  check_bf16_dst("gemv_fp8_res", resid, N);
  TORCH_CHECK(N <= 8192, "gemv_fp8_res: w32 kernel only (hidden <= 8192)");
  auto xc = x.contiguous();
  launch_quant_fp8(uptr(xc), x8.data_ptr<uint8_t>(), xs.data_ptr<float>(),
                   1, K, cur_stream());
  launch_gemv_fp8_res(x8.data_ptr<uint8_t>(), xs.data_ptr<float>(),
                      w8.data_ptr<uint8_t>(), wsc.data_ptr<float>(),
                      uptr_mut(resid), K, N, cur_stream());
}

// pre-quantized fused fp8 gate_up GEMV + SwiGLU
void gemv_fp8_gateup(torch::Tensor x8, torch::Tensor xs, torch::Tensor w8,
                     torch::Tensor wsc, torch::Tensor act) {
  check_fp8_weight("gemv_fp8_gateup", w8, wsc);
  const int K = w8.size(1), F2 = w8.size(0);
  TORCH_CHECK(F2 % 2 == 0, "gemv_fp8_gateup: w8 = [gate rows | up rows]");
  check_fp8_act("gemv_fp8_gateup", x8, xs, K);
  check_bf16_dst("gemv_fp8_gateup", act, F2 / 2);
  launch_gemv_fp8_gateup(x8.data_ptr<uint8_t>(), xs.data_ptr<float>(),
                         w8.data_ptr<uint8_t>(), wsc.data_ptr<float>(),
                         uptr_mut(act), K, F2 / 2, cur_stream());
}

// LDS-staged single-launch fp8 fused GEMVs (each block quantizes its own
// activation copy into LDS — removes the serial 1-block quant kernels
// from the decode critical path):

// y = rmsnorm(x, wln) @ w8^T (quantize + GEMV fused)
void gemv_fp8_norm(torch::Tensor x, torch::Tensor wln, torch::Tensor w8,
                   torch::Tensor wsc, double eps, torch::Tensor out) {
  CHECK_BF16_CUDA(x);
  CHECK_BF16_CUDA(wln);
  auto xc = x.contiguous();
  const int N = w8.size(0), K = w8.size(1);
  TORCH_CHECK((long)xc.numel() == (long)K && K % 16 == 0);
  TORCH_CHECK((long)wln.numel() == (long)K);
  TORCH_CHECK((long)out.numel() == (long)N);
  TORCH_CHECK(K <= 65536, "gemv_fp8_norm: LDS staging caps K at 65536");
  launch_gemv_fp8_norm(uptr(xc), uptr(wln), w8.data_ptr<uint8_t>(),
                       wsc.data_ptr<float>(), uptr_mut(out), K, N,
                       (float)eps, cur_stream());
}

// resid += x @ w8^T (quantize + GEMV + residual epilogue, in place).
// NOT valid under TP (the all-reduce needs the raw partial product).
void gemv_fp8_resl(torch::Tensor x, torch::Tensor w8, torch::Tensor wsc,
                   torch::Tensor resid) {
  CHECK_BF16_CUDA(x);
  CHECK_BF16_CUDA(resid);
  auto xc = x.contiguous();
  const int N = w8.size(0), K = w8.size(1);
  TORCH_CHECK((long)xc.numel() == (long)K && K % 16 == 0);
  TORCH_CHECK((long)resid.numel() == (long)N && resid.is_contiguous());
  TORCH_CHECK(N <= 8192, "gemv_fp8_resl: w32 kernel only (hidden <= 8192)");
  TORCH_CHECK(K <= 65536, "gemv_fp8_resl: LDS staging caps K at 65536");
  launch_gemv_fp8_resl(uptr(xc), w8.data_ptr<uint8_t>(),
                       wsc.data_ptr<float>(), uptr_mut(resid), K, N,
                       cur_stream());
}

// act = swiglu(rmsnorm(x, wln) @ [Wg|Wu]^T) — fp8 MLP front half, 1 launch
void gemv_fp8_gateup_norm(torch::Tensor x, torch::Tensor wln,
                          torch::Tensor w8, torch::Tensor wsc, double eps,
                          torch::Tensor act) {
  CHECK_BF16_CUDA(x);
  CHECK_BF16_CUDA(wln);
  CHECK_BF16_CUDA(act);
  auto xc = x.contiguous();
  const int K = w8.size(1), F2 = w8.size(0);
  TORCH_CHECK(F2 % 2 == 0 && (long)xc.numel() == (long)K && K % 16 == 0);
  TORCH_CHECK((long)wln.numel() == (long)K);
  TORCH_CHECK((long)act.numel() == (long)(F2 / 2));
  TORCH_CHECK(K <= 65536, "gemv_fp8_gateup_norm: LDS caps K at 65536");
  launch_gemv_fp8_gateup_norm(uptr(xc), uptr(wln), w8.data_ptr<uint8_t>(),
                              wsc.data_ptr<float>(), uptr_mut(act), K,
                              F2 / 2, (float)eps, cur_stream());
}

int64_t sample(torch::Tensor logits, double temp, double top_p, int64_t seed) {
  CHECK_BF16_CUDA(logits);
  TORCH_CHECK(top_p >= 1.0, "kernel sample handles top_p == 1 (nucleus is a cold path)");
  auto lc = logits.contiguous();
  const int vocab = lc.numel();
  auto out = torch::empty({1}, torch::TensorOptions()
                                   .dtype(at::kInt)
                                   .device(logits.device()));
  launch_sample(uptr(lc), vocab, (float)temp, (uint32_t)seed,
                out.data_ptr<int>(), cur_stream());
  return out.cpu().item<int>();
}

void sample_state(torch::Tensor logits, torch::Tensor temp_state,
                  torch::Tensor rng_state, torch::Tensor tok_hist,
                  torch::Tensor step_state, torch::Tensor tok_long) {
  CHECK_BF16_CUDA(logits);
  TORCH_CHECK(temp_state.scalar_type() == at::kFloat && temp_state.is_cuda(),
              "sample_state: temp_state must be a device f32 word");
  TORCH_CHECK(tok_long.scalar_type() == at::kLong,
              "sample_state: tok_long must be int64 (the embedding index)");
  auto lc = logits.contiguous();
  launch_sample_state(
      uptr(lc), (int)lc.numel(), temp_state.data_ptr<float>(),
      reinterpret_cast<uint32_t*>(rng_state.data_ptr<int>()),
      tok_hist.data_ptr<int>(), step_state.data_ptr<int>(),
      reinterpret_cast<long long*>(tok_long.data_ptr<int64_t>()),
      cur_stream());
}

// ---- top-p / top-k filtered sampling --------------------------------------
// Host-side argument checks shared by the three entries; the kernels index
// the row as bf16x8 vectors and count tokens in float-exact integers.
static int check_filtered_row(const char* who, const torch::Tensor& logits) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kBFloat16,
              who, ": logits must be a bf16 device tensor");
  const int64_t vocab = logits.numel();
  TORCH_CHECK(vocab > 0 && vocab % 8 == 0 && vocab < (1 << 24), who,
              ": vocab must be a positive multiple of 8 below 2^24, got ",
              vocab);
  return (int)vocab;
}

static void check_filter_args(const char* who, double top_p, int64_t top_k) {
  TORCH_CHECK(top_p > 0.0 && top_p <= 1.0, who, ": top_p must be in (0, 1], got ",
              top_p);
  TORCH_CHECK(top_k >= 0 && top_k <= INT32_MAX, who,
              ": top_k must be >= 0, got ", top_k);
}

int64_t sample_filtered(torch::Tensor logits, double temp, double top_p,
                        int64_t top_k, int64_t seed) {
  const int vocab = check_filtered_row("sample_filtered", logits);
  check_filter_args("sample_filtered", top_p, top_k);
  auto lc = logits.contiguous();
  auto out = torch::empty({1}, torch::TensorOptions()
                                   .dtype(at::kInt)
                                   .device(logits.device()));
  launch_sample_filtered(uptr(lc), vocab, (float)temp, (float)top_p,
                         (int)top_k, (uint32_t)seed, out.data_ptr<int>(),
                         cur_stream());
  return out.cpu().item<int>();
}

void sample_state_filtered(torch::Tensor logits, torch::Tensor temp_state,
                           torch::Tensor top_p_state, torch::Tensor top_k_state,
                           torch::Tensor rng_state, torch::Tensor tok_hist,
                           torch::Tensor step_state, torch::Tensor tok_long) {
  const int vocab = check_filtered_row("sample_state_filtered", logits);
  TORCH_CHECK(logits.is_contiguous(),
              "sample_state_filtered: logits must be contiguous (no copy is "
              "made inside a captured step)");
  TORCH_CHECK(temp_state.scalar_type() == at::kFloat && temp_state.is_cuda() &&
                  temp_state.numel() >= 1,
              "sample_state_filtered: temp_state must be a device f32 word");
  TORCH_CHECK(top_p_state.scalar_type() == at::kFloat && top_p_state.is_cuda() &&
                  top_p_state.numel() >= 1,
              "sample_state_filtered: top_p_state must be a device f32 word");
  TORCH_CHECK(top_k_state.scalar_type() == at::kInt && top_k_state.is_cuda() &&
                  top_k_state.numel() >= 1,
              "sample_state_filtered: top_k_state must be a device int32 word");
  TORCH_CHECK(rng_state.scalar_type() == at::kInt && rng_state.is_cuda() &&
                  rng_state.numel() >= 1,
              "sample_state_filtered: rng_state must be a device int32 word");
  TORCH_CHECK(step_state.scalar_type() == at::kInt && step_state.is_cuda() &&
                  step_state.numel() >= 1,
              "sample_state_filtered: step_state must be a device int32 word");
  TORCH_CHECK(tok_hist.scalar_type() == at::kInt && tok_hist.is_cuda() &&
                  tok_hist.is_contiguous() && tok_hist.numel() >= 1,
              "sample_state_filtered: tok_hist must be device int32");
  TORCH_CHECK(tok_long.scalar_type() == at::kLong && tok_long.is_cuda() &&
                  tok_long.numel() >= 1,
              "sample_state_filtered: tok_long must be int64 (the embedding "
              "index)");
  launch_sample_state_filtered(
      uptr(logits), vocab, temp_state.data_ptr<float>(),
      top_p_state.data_ptr<float>(), top_k_state.data_ptr<int>(),
      reinterpret_cast<uint32_t*>(rng_state.data_ptr<int>()),
      tok_hist.data_ptr<int>(), step_state.data_ptr<int>(),
      reinterpret_cast<long long*>(tok_long.data_ptr<int64_t>()),
      cur_stream());
}

// The kept set of a row as uint8 [vocab] (1 = kept), by the samplers' cut.
torch::Tensor nucleus_mask(torch::Tensor logits, double temp, double top_p,
                           int64_t top_k) {
  const int vocab = check_filtered_row("nucleus_mask", logits);
  check_filter_args("nucleus_mask", top_p, top_k);
  auto lc = logits.contiguous();
  auto mask = torch::empty({vocab}, torch::TensorOptions()
                                        .dtype(at::kByte)
                                        .device(logits.device()));
  launch_nucleus_mask(uptr(lc), vocab, (float)temp, (float)top_p, (int)top_k,
                      mask.data_ptr<uint8_t>(), cur_stream());
  return mask;
}

// Release the decode-attention scratch entries whose keys (per-layer KV
// cache base pointers) lie inside a dropped cache allocation, and free the
// retired grown tensors. Call ONLY after every captured graph referencing
// the cache has been destroyed (engine/local.py drops _graph_state first);
// without this, long-lived processes leak scratch per cache growth and can
// inherit a stale entry when the allocator reuses a freed cache address
// (ADVICE round 1).
void ws_release(torch::Tensor kc_all) {
  char* base = reinterpret_cast<char*>(kc_all.data_ptr());
  const size_t bytes = (size_t)kc_all.numel() * kc_all.element_size();
  std::lock_guard<std::mutex> lk(g_ws_mu);
  for (auto it = g_ws.begin(); it != g_ws.end();) {
    char* p = reinterpret_cast<char*>(it->first);
    if (p >= base && p < base + bytes) {
      it = g_ws.erase(it);
    } else {
      ++it;
    }
  }
}

// fp8 twin of rope_kv: rotate q/k in place (bit-identical to rope_kv) and
// append the rowwise-quantized rotated k and v plus their scales.
void rope_kv_fp8(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                 torch::Tensor cost, torch::Tensor sint, torch::Tensor kc,
                 torch::Tensor vc, torch::Tensor ksc, torch::Tensor vsc,
                 torch::Tensor page_table, int64_t pos0,
                 const OptTensor& pos_state) {
  check_qkv_views("rope_kv_fp8", q, k, &v);
  check_fp8_cache("rope_kv_fp8", kc, vc, ksc, vsc, page_table);
  check_cache_matches("rope_kv_fp8", kc, k);
  const int t = q.size(0), hq = q.size(1), hd = q.size(2);
  const int hk = k.size(1);
  const int page = kc.size(1);
  check_rope_tables("rope_kv_fp8", cost, sint, hd);
  const int* pp = check_pos_state("rope_kv_fp8", pos_state);
  if (!pp) check_host_pos("rope_kv_fp8", pos0, t, &cost, &page_table, page);
  if (t == 0) return;
  launch_rope_kv_fp8(uptr_mut(q), uptr_mut(k), uptr(v), cost.data_ptr<float>(),
                     sint.data_ptr<float>(), kc.data_ptr<uint8_t>(),
                     vc.data_ptr<uint8_t>(), ksc.data_ptr<float>(),
                     vsc.data_ptr<float>(), page_table.data_ptr<int>(), t, hq,
                     hk, hd, (int)pos0, q.stride(0), k.stride(0), v.stride(0),
                     page, pp, cur_stream());
}

// Positions [0, n) of one layer's fp8 cache -> contiguous bf16 [n, kh, hd]
// (k, v), through the page table. Chunked prefill only.
std::tuple<torch::Tensor, torch::Tensor> kv_dequant_fp8(
    torch::Tensor kc, torch::Tensor vc, torch::Tensor ksc, torch::Tensor vsc,
    torch::Tensor page_table, int64_t n) {
  check_fp8_cache("kv_dequant_fp8", kc, vc, ksc, vsc, page_table);
  const int page = kc.size(1), kh = kc.size(2), hd = kc.size(3);
  TORCH_CHECK(n >= 0 && n <= page_table.numel() * (int64_t)page,
              "kv_dequant_fp8: n outside the page table");
  auto opts = torch::TensorOptions().dtype(at::kBFloat16).device(kc.device());
  auto kout = torch::empty({n, kh, hd}, opts);
  auto vout = torch::empty({n, kh, hd}, opts);
  launch_kv_dequant_fp8(kc.data_ptr<uint8_t>(), vc.data_ptr<uint8_t>(),
                        ksc.data_ptr<float>(), vsc.data_ptr<float>(),
                        page_table.data_ptr<int>(), uptr_mut(kout),
                        uptr_mut(vout), (int)n, kh, hd, page, cur_stream());
  return {kout, vout};
}

void bump(torch::Tensor pos_state, torch::Tensor step_state) {
  launch_bump(pos_state.data_ptr<int>(), step_state.data_ptr<int>(),
              cur_stream());
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("rmsnorm", &rmsnorm, "fused RMSNorm (bf16, gfx950)",
        py::arg("x"), py::arg("w"), py::arg("eps"),
        py::arg("out") = py::none());
  m.def("add_rmsnorm", &add_rmsnorm, "fused residual add + RMSNorm",
        py::arg("resid"), py::arg("delta"), py::arg("w"), py::arg("eps"),
        py::arg("out_resid") = py::none(), py::arg("out_y") = py::none());
  m.def("rope_inplace", &rope_inplace, "RoPE (interleaved pairs, table-driven)",
        py::arg("q"), py::arg("k"), py::arg("cost"), py::arg("sint"),
        py::arg("pos0"), py::arg("pos_state") = py::none());
  m.def("swiglu", &swiglu, "fused silu(gate)*up",
        py::arg("gate"), py::arg("up"), py::arg("out") = py::none());
  m.def("kv_write", &kv_write, "paged KV scatter",
        py::arg("kc"), py::arg("vc"), py::arg("page_table"), py::arg("pos0"),
        py::arg("k"), py::arg("v"), py::arg("pos_state") = py::none());
  m.def("attn_prefill", &attn_prefill, "causal prefill attention",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("scale"),
        py::arg("causal"), py::arg("kv_offset"), py::arg("window") = 0);
  m.def("attn_prefill_simple", &attn_prefill_simple, "non-MFMA prefill (anchor)");
  m.def("attn_prefill_ablate", &attn_prefill_ablate,
        "prefill attention perf-ablation variants");
  m.def("mfma_probe16", &mfma_probe16, "MFMA 16x16x32 fragment-map probe");
  m.def("attn_decode_paged", &attn_decode_paged, "paged decode attention",
        py::arg("q"), py::arg("kc"), py::arg("vc"), py::arg("page_table"),
        py::arg("seq_len"), py::arg("scale"),
        py::arg("pos_state") = py::none(), py::arg("out") = py::none(),
        py::arg("identity") = false, py::arg("split_blocks") = 0,
        py::arg("window") = 0);
  m.def("decode_split_geometry", &decode_split_geometry,
        "decode split geometry query -> (n_splits, split_len)",
        py::arg("seq"), py::arg("kh"), py::arg("split_blocks") = 0,
        py::arg("window") = 0);
  m.def("sample", &sample, "fused temperature softmax sample");
  m.def("sample_to", &sample_to, "async on-device sample into out[idx]");
  m.def("gemv", &gemv, "batch-1 decode GEMV (weight streaming)",
        py::arg("x"), py::arg("w"), py::arg("out") = py::none());
  m.def("gemv_gateup", &gemv_gateup, "fused gate_up GEMV + SwiGLU (decode)");
  m.def("gemv_norm", &gemv_norm, "rmsnorm-prologue GEMV (decode fusion)",
        py::arg("x"), py::arg("wln"), py::arg("w"), py::arg("eps"),
        py::arg("out") = py::none());
  m.def("gemv_res", &gemv_res, "residual-add-epilogue GEMV (decode fusion)");
  m.def("gemv_gateup_norm", &gemv_gateup_norm,
        "rmsnorm + gate_up GEMV + SwiGLU (decode fusion)");
  m.def("gemm", &gemm, "tiled MFMA GEMM (bf16, fp32 accum)");
  m.def("gemm_variant", &gemm_variant, "force GEMM kernel 128/256 (A/B)");
  m.def("gemm_fp8", &gemm_fp8, "fp8 e4m3 MFMA GEMM (rowwise scales)");
  m.def("gemv_fp8", &gemv_fp8, "fp8 decode GEMV (rowwise scales)");
  m.def("quant_norm_fp8", &quant_norm_fp8,
        "fused rmsnorm + rowwise e4m3 quantize (fp8 decode fusion)");
  m.def("gemv_fp8_q", &gemv_fp8_q, "pre-quantized fp8 decode GEMV");
  m.def("gemv_fp8_res", &gemv_fp8_res,
        "fp8 GEMV with residual-add epilogue (fp8 decode fusion)");
  m.def("gemv_fp8_gateup", &gemv_fp8_gateup,
        "pre-quantized fp8 gate_up GEMV + SwiGLU (fp8 decode fusion)");
  m.def("gemv_fp8_norm", &gemv_fp8_norm,
        "rmsnorm + quantize + fp8 GEMV, one launch (LDS-staged)");
  m.def("gemv_fp8_resl", &gemv_fp8_resl,
        "quantize + fp8 GEMV + residual epilogue, one launch (LDS-staged)");
  m.def("gemv_fp8_gateup_norm", &gemv_fp8_gateup_norm,
        "rmsnorm + quantize + fp8 gate_up GEMV + SwiGLU, one launch");
  m.def("quant_fp8", &quant_fp8, "rowwise bf16 -> e4m3 quantizer");
  m.def("mfma_rate", &mfma_rate, "MFMA issue-rate microbench (bf16/fp8)");
  m.def("rope_kv", &rope_kv, "fused RoPE + paged KV scatter",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("cost"),
        py::arg("sint"), py::arg("kc"), py::arg("vc"), py::arg("page_table"),
        py::arg("pos0"), py::arg("pos_state") = py::none());
  m.def("gemv_norm_rope_kv", &gemv_norm_rope_kv,
        "rmsnorm + qkv GEMV + RoPE + KV append, one launch (decode fusion)",
        py::arg("x"), py::arg("wln"), py::arg("w"), py::arg("eps"),
        py::arg("cost"), py::arg("sint"), py::arg("kc"), py::arg("vc"),
        py::arg("page_table"), py::arg("pos0"), py::arg("hq"), py::arg("kh"),
        py::arg("pos_state") = py::none(), py::arg("out") = py::none());
  m.def("gemv_fp8_q_rope_kv", &gemv_fp8_q_rope_kv,
        "pre-quantized fp8 qkv GEMV + RoPE + KV append, one launch",
        py::arg("x8"), py::arg("xs"), py::arg("w8"), py::arg("wsc"),
        py::arg("out"), py::arg("cost"), py::arg("sint"), py::arg("kc"),
        py::arg("vc"), py::arg("page_table"), py::arg("pos0"), py::arg("hq"),
        py::arg("kh"), py::arg("pos_state") = py::none());
  m.def("sample_state", &sample_state, "graph-mode on-device sampling");
  m.def("bump", &bump, "graph-mode pos/step bump");
  m.def("sample_filtered", &sample_filtered,
        "top-p / top-k filtered on-device sample",
        py::arg("logits"), py::arg("temp"), py::arg("top_p"),
        py::arg("top_k"), py::arg("seed"));
  m.def("sample_state_filtered", &sample_state_filtered,
        "graph-mode top-p / top-k filtered sampling",
        py::arg("logits"), py::arg("temp_state"), py::arg("top_p_state"),
        py::arg("top_k_state"), py::arg("rng_state"), py::arg("tok_hist"),
        py::arg("step_state"), py::arg("tok_long"));
  m.def("nucleus_mask", &nucleus_mask,
        "kept set of a logits row under top-p / top-k, uint8 [vocab]",
        py::arg("logits"), py::arg("temp"), py::arg("top_p"),
        py::arg("top_k"));
  m.def("rope_kv_fp8", &rope_kv_fp8,
        "fused RoPE + rowwise-e4m3 quantizing paged KV append",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("cost"),
        py::arg("sint"), py::arg("kc"), py::arg("vc"), py::arg("ksc"),
        py::arg("vsc"), py::arg("page_table"), py::arg("pos0"),
        py::arg("pos_state") = py::none());
  m.def("kv_dequant_fp8", &kv_dequant_fp8,
        "fp8 KV cache positions [0, n) -> contiguous bf16 (k, v)",
        py::arg("kc"), py::arg("vc"), py::arg("ksc"), py::arg("vsc"),
        py::arg("page_table"), py::arg("n"));
  m.def("attn_decode_paged_fp8", &attn_decode_paged_fp8,
        "paged decode attention over an fp8 KV cache",
        py::arg("q"), py::arg("kc"), py::arg("vc"), py::arg("ksc"),
        py::arg("vsc"), py::arg("page_table"), py::arg("seq_len"),
        py::arg("scale"), py::arg("pos_state") = py::none(),
        py::arg("out") = py::none(), py::arg("identity") = false,
        py::arg("split_blocks") = 0, py::arg("window") = 0);
  m.def("ws_release", &ws_release,
        "drop decode-attention scratch for a dead KV cache");
}
