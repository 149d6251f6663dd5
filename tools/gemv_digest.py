"""One sha256 per decode GEMV op over its output bytes, on seeded random
operands that are NOT fp32-exact.

tests/test_gemv_exact_gpu.py feeds the kernels small integers, for which any
summation order and any fma contraction give the same bits. This prints the
other half: run it on two builds and compare the lines; a digest that differs
means the arithmetic of that op changed (order of the adds, a fused or
unfused multiply, a different scale read).

Shapes: K is the `both_loops` lane split of the op's kernel
(tests/gemv_exact_common.py), N is 9, plus 8200 for the four ops whose
launcher switches kernels above N == 8192; the two RoPE ops take N == 48 and
are digested over the output and the appended cache rows.
"""
import hashlib
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from adversarial_spec_amd import ops  # noqa: E402
from gemv_exact_common import (  # noqa: E402
    BF16, EPS, OPS, SWITCHING_OPS, is_fp8, is_gateup, is_norm, has_resid,
    k_cases, rope_geometry)

DEV = "cuda:0"
ROPE_OPS = {"gemv_norm_rope_kv": "gemv_norm_rope_kv_w32_kernel",
            "gemv_fp8_q_rope_kv": "gemv_fp8_rope_kv_w32_kernel"}


def operands(op, K, N, seed):
    """Seeded CPU operands in the dtypes the op reads."""
    g = torch.Generator().manual_seed(seed)
    rows = 2 * N if is_gateup(op) else N
    d = {"x": torch.randn(1, K, generator=g).to(BF16)}
    w = torch.randn(rows, K, generator=g) * K ** -0.5
    if is_fp8(op):
        d["w8"], d["wsc"] = ops.quantize_fp8_rowwise(w)
        x8, xs = ops.quantize_fp8_rowwise(d["x"])
        d["x8"], d["xs"] = x8, xs
    else:
        d["w"] = w.to(BF16)
    if is_norm(op):
        d["wln"] = (1.0 + 0.1 * torch.randn(K, generator=g)).to(BF16)
    d["resid"] = torch.randn(1, N, generator=g).to(BF16)
    d["angle"] = torch.rand(4, 8, generator=g) * 6.28
    return d


def run(op, K, N, seed):
    d = {k: v.to(DEV) for k, v in operands(op, K, N, seed).items()}
    out = d["resid"].clone() if has_resid(op) else torch.zeros(
        1, N, dtype=BF16, device=DEV)
    parts = [out]
    if op in ROPE_OPS:
        hq, kh, hd, n = rope_geometry(N)
        assert n == N and hd == 16
        cos, sin = torch.cos(d["angle"]), torch.sin(d["angle"])
        kc = torch.zeros(2, 2, kh, hd, dtype=BF16, device=DEV)
        vc = torch.zeros_like(kc)
        table = torch.tensor([1, 0], dtype=torch.int32, device=DEV)
        parts += [kc, vc]
    x8s = torch.zeros(1, K, dtype=torch.uint8, device=DEV)
    xss = torch.zeros(1, dtype=torch.float32, device=DEV)

    if op == "gemv":
        ops.gemv(d["x"], d["w"], out=out)
    elif op == "gemv_res":
        ops.gemv_res(d["x"], d["w"], out)
    elif op == "gemv_gateup":
        ops.gemv_gateup(d["x"], d["w"], out)
    elif op == "gemv_norm":
        ops.gemv_norm(d["x"], d["wln"], d["w"], EPS, out=out)
    elif op == "gemv_gateup_norm":
        ops.gemv_gateup_norm(d["x"], d["wln"], d["w"], EPS, out)
    elif op == "gemv_norm_rope_kv":
        ops.gemv_norm_rope_kv(d["x"], d["wln"], d["w"], EPS, cos, sin, kc, vc,
                              table, 1, hq, kh, out=out)
    elif op == "gemv_fp8":
        ops.gemv_fp8(d["x"], d["w8"], d["wsc"], x8s, xss, out)
    elif op == "gemv_fp8_q":
        ops.gemv_fp8_q(d["x8"], d["xs"], d["w8"], d["wsc"], out)
    elif op == "gemv_fp8_q_rope_kv":
        ops.gemv_fp8_q_rope_kv(d["x8"], d["xs"], d["w8"], d["wsc"], out, cos,
                               sin, kc, vc, table, 1, hq, kh)
    elif op == "gemv_fp8_res":
        ops.gemv_fp8_res(d["x"], d["w8"], d["wsc"], x8s, xss, out)
    elif op == "gemv_fp8_gateup":
        ops.gemv_fp8_gateup(d["x8"], d["xs"], d["w8"], d["wsc"], out)
    elif op == "gemv_fp8_norm":
        ops.gemv_fp8_norm(d["x"], d["wln"], d["w8"], d["wsc"], EPS, out)
    elif op == "gemv_fp8_resl":
        ops.gemv_fp8_resl(d["x"], d["w8"], d["wsc"], out)
    elif op == "gemv_fp8_gateup_norm":
        ops.gemv_fp8_gateup_norm(d["x"], d["wln"], d["w8"], d["wsc"], EPS, out)
    else:
        raise AssertionError(op)
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in parts:
        assert torch.isfinite(t.float()).all(), op
        h.update(t.cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    assert ops.hip_available(), "HIP extension not built"
    cases = []
    for op, (small, large) in OPS.items():
        if op in ROPE_OPS:
            continue
        cases.append((op, small, 9))
        if op in SWITCHING_OPS:
            cases.append((op, large, 8200))
    cases += [(op, kernel, 48) for op, kernel in ROPE_OPS.items()]
    for seed, (op, kernel, N) in enumerate(cases):
        K = k_cases(kernel)["both_loops"]
        print(f"{op:22s} {kernel:30s} K={K:5d} N={N:5d} "
              f"{run(op, K, N, seed)}", flush=True)


if __name__ == "__main__":
    main()
