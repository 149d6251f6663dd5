"""Minimal decode-attention run (split + combine), for rocprofv3
(kernel-trace or PMC) or timed on its own.

    attn_split_solo.py [seq] [iters] [--kv-dtype bf16|fp8] [--identity]
                       [--split-blocks N] [--window W]

After 10 eager warm-up calls the kernels run from HIP-GRAPH REPLAY: 20 calls
are captured once and the graph is replayed, so a profiler sees graph-launched
kernels and `iters` is rounded down to a multiple of 20 (at least 20). The
mean time per call (HIP events around the replays) is printed, so the bf16
and fp8 KV paths can be compared without a profiler. `kv_bytes` is what one
call reads from the cache: K and V rows, plus the scale tensors for fp8
(`scale_bytes`, about 3 % of the fp8 total at hd=128); with `--window` only
the rows the windowed call stages are counted.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from adversarial_spec_amd import ops  # noqa: E402
from adversarial_spec_amd.ops import torch_ref  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("seq", nargs="?", type=int, default=8192)
ap.add_argument("iters", nargs="?", type=int, default=200)
ap.add_argument("--kv-dtype", choices=["bf16", "fp8"], default="bf16")
ap.add_argument("--identity", action="store_true",
                help="identity page table (the engine's single-pool cache)")
ap.add_argument("--split-blocks", type=int, default=0)
ap.add_argument("--window", type=int, default=0,
                help="sliding window: attend the last W positions only")
args = ap.parse_args()

torch.manual_seed(7)
kh, group, hd, page = 8, 4, 128, 256
seq, iters = args.seq, args.iters
npages = (seq + page - 1) // page + 1
kc = torch.randn(npages, page, kh, hd, device="cuda").bfloat16()
vc = torch.randn(npages, page, kh, hd, device="cuda").bfloat16()
pt = torch.arange(npages, device="cuda", dtype=torch.int32)
q = torch.randn(kh * group, hd, device="cuda").bfloat16()
pos = torch.tensor([seq - 1], dtype=torch.int32, device="cuda")
out = torch.empty(kh * group, hd, device="cuda").bfloat16()
kw = dict(pos_state=pos, out=out, identity=args.identity,
          split_blocks=args.split_blocks, window=args.window)
if args.kv_dtype == "fp8":
    kc, ks = torch_ref.quantize_kv_fp8(kc)
    vc, vs = torch_ref.quantize_kv_fp8(vc)
    ks = ks.permute(0, 2, 1).contiguous()  # [n_pages, kh, page]
    vs = vs.permute(0, 2, 1).contiguous()

    def call():
        ops.attn_decode_paged_fp8(q, kc, vc, ks, vs, pt, seq, None, **kw)
else:
    def call():
        ops.attn_decode_paged(q, kc, vc, pt, seq, None, **kw)

for _ in range(10):
    call()
torch.cuda.synchronize()
# time replays of a captured batch of calls: back-to-back eager launches of
# a ~10 us kernel pair measure the host's launch rate, not the kernels
BATCH = 20
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
    for _ in range(BATCH):
        call()
graph.replay()
torch.cuda.synchronize()
t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
reps = max(1, iters // BATCH)
iters = reps * BATCH
t0.record()
for _ in range(reps):
    graph.replay()
t1.record()
torch.cuda.synchronize()
# rows one call stages: with a window, from the 64-aligned tile that holds
# position seq - W (at most W + 63 rows), else the whole context
rows = seq
if 0 < args.window < seq:
    rows = seq - (seq - args.window) // 64 * 64
scale_bytes = 2 * rows * kh * 4 if args.kv_dtype == "fp8" else 0
kv_bytes = 2 * rows * kh * hd * kc.element_size() + scale_bytes
print(f"done {seq} {iters} kv_dtype={args.kv_dtype} identity={args.identity} "
      f"window={args.window} "
      f"kv_bytes={kv_bytes} scale_bytes={scale_bytes} us_per_call={t0.elapsed_time(t1) * 1e3 / iters:.2f}")
