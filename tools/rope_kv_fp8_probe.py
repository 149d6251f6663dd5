"""rope_kv_fp8 launch against the rope_kv launch it mirrors (Llama-3-8B
heads, page 256, position 8192), timed from graph replay. Figures in
profiles/r04_fp8_kv.md."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from adversarial_spec_amd import ops
from adversarial_spec_amd.ops import torch_ref
hq, kh, hd, page, pos = 32, 8, 128, 256, 8192
npg = 40
cos, sin = torch_ref.rope_tables(hd, 16384, 500000.0, "cuda")
qkv = torch.randn(1, (hq + 2 * kh) * hd, device="cuda").bfloat16()
q = qkv[:, :hq*hd].view(1, hq, hd); k = qkv[:, hq*hd:(hq+kh)*hd].view(1, kh, hd); v = qkv[:, (hq+kh)*hd:].view(1, kh, hd)
pt = torch.arange(npg, device="cuda", dtype=torch.int32)
kc = torch.zeros(npg, page, kh, hd, device="cuda", dtype=torch.bfloat16); vc = torch.zeros_like(kc)
k8 = torch.zeros(npg, page, kh, hd, device="cuda", dtype=torch.uint8); v8 = torch.zeros_like(k8)
ks = torch.zeros(npg, kh, page, device="cuda"); vs = torch.zeros_like(ks)
ps = torch.tensor([pos], dtype=torch.int32, device="cuda")
def timeit(fn, name):
    for _ in range(5): fn()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        for _ in range(50): fn()
    g.replay(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(40): g.replay()
    b.record(); torch.cuda.synchronize()
    print(f"{name}: {a.elapsed_time(b) * 1e3 / 2000:.2f} us/launch")
timeit(lambda: ops.rope_kv(q, k, v, cos, sin, kc, vc, pt, 0, pos_state=ps), "rope_kv (bf16 cache)")
timeit(lambda: ops.rope_kv_fp8(q, k, v, cos, sin, k8, v8, ks, vs, pt, 0, pos_state=ps), "rope_kv_fp8")
