"""One sha256 per prefill-GEMM case over the bytes of the output, on seeded
uniform-random operands that are NOT fp32-exact.

tests/test_gemm_exact_gpu.py holds the four kernels bit-exactly on inputs
whose fp32 accumulation is exact in any order. This prints the other half:
run it on two builds and compare the lines; a digest that differs means the
arithmetic of that kernel changed (the order of the K sum, which MFMA takes
which k-slice, the order of the two scale products in the fp8 store).

Shapes are the lists of tests/gemm_exact_common.py: SHAPES_128 and SHAPES_256
through gemm_variant (which forces the kernel), SHAPES_128_FP8 and
SHAPES_256_FP8 through gemm_fp8 (dispatch256 is asserted to send each where
its list says). One grid per kernel adds interior and edge blocks together
with more than three K-tiles: BIG for three of them, BIG_128_FP8 for the 128^2
fp8 kernel, whose K must stay off the 256^2 rule (1040 = 16 * 65 also ends on
a K edge).
"""
import hashlib
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from gemm_exact_common import (  # noqa: E402
    SHAPES_128, SHAPES_128_FP8, SHAPES_256, SHAPES_256_FP8, dispatch256)

from adversarial_spec_amd import ops  # noqa: E402

DEV = "cuda:0"
BIG = (385, 511, 1024)
BIG_128_FP8 = (385, 511, 1040)


def operands(M, N, K):
    """A [M, K] uniform in [-1, 1), B [N, K] uniform in [-0.05, 0.05), bf16."""
    g = torch.Generator().manual_seed((M * 1009 + N) * 1009 + K)
    a = (torch.rand(M, K, generator=g) * 2 - 1).bfloat16()
    b = ((torch.rand(N, K, generator=g) * 2 - 1) * 0.05).bfloat16()
    return a.to(DEV), b.to(DEV)


def digest(out, shape):
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == shape[:2]
    assert torch.isfinite(out.float()).all()
    return hashlib.sha256(
        out.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    hip = ops._require_hip()
    for which, shapes in ((128, SHAPES_128 + (BIG,)), (256, SHAPES_256)):
        assert which == 128 or BIG in shapes
        for s in shapes:
            a, b = operands(*s)
            print(f"bf16 {which} M={s[0]} N={s[1]} K={s[2]} "
                  f"{digest(hip.gemm_variant(a, b, which), s)}", flush=True)
    assert BIG in SHAPES_256_FP8
    for which, shapes in ((128, SHAPES_128_FP8 + (BIG_128_FP8,)),
                          (256, SHAPES_256_FP8)):
        for s in shapes:
            assert dispatch256(*s) == (which == 256), s
            a, b = operands(*s)
            wq, wsc = ops.quantize_fp8_rowwise(b)
            print(f"fp8  {which} M={s[0]} N={s[1]} K={s[2]} "
                  f"{digest(ops.gemm_fp8(a, wq, wsc), s)}", flush=True)


if __name__ == "__main__":
    main()
