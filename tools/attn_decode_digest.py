"""One sha256 per decode-attention case over the bytes of `out`, on seeded
random operands that are NOT fp32-exact.

tests/test_attention_edges_gpu.py and tests/test_kv_fp8_gpu.py hold the two
split kernels to a float64 reference within a tolerance. This prints the
other half: run it on two builds and compare the lines; a digest that differs
means the arithmetic of that instantiation changed (order of the adds, a
fused or unfused multiply, a different scale fold).

Cases are the smallest that reach every template branch of
attn_decode_split_tiles (ops/hip/attn_decode_split.h): kh = 2, page = 16 (a
64-position tile crosses pages), both KV formats, hd 32/64/128, group 2, 3
(MG = 4, an idle fourth wave, a q image shorter than one piece) and 8 (two
heads per wave), a permuted table with identity=False and an identity table
with identity=True, and two geometries asserted through
decode_split_geometry: one split of four tiles at seq 193 (both buffers
restaged, a one-position last tile) and two splits of three and two tiles at
seq 300 (workspace + combine). One graph-mode case per format and hd: bound
1024, position 69, so the trailing splits walk zero tiles.
"""
import hashlib
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from adversarial_spec_amd import ops  # noqa: E402
from adversarial_spec_amd.ops import _advspec_hip as _hip  # noqa: E402
from adversarial_spec_amd.ops import torch_ref  # noqa: E402

DEV = "cuda:0"
KH, PAGE, DTILE, BOUND = 2, 16, 64, 1024
# (seq, split_blocks, tiles per split)
GEOMETRIES = [(193, 2, [4]), (300, 4, [3, 2])]
GRAPH_POS, GRAPH_TILES = 69, [1, 1] + [0] * 14


def check_geometry(seq, split_blocks, want, bound=None):
    assert os.environ.get("ADVSPEC_SPLIT_BLOCKS") is None
    ns, sl = _hip.decode_split_geometry(bound or seq, KH, split_blocks)
    got = [max(0, -(-(min(seq, (i + 1) * sl) - i * sl) // DTILE))
           for i in range(ns)]
    assert got == want, (seq, split_blocks, ns, sl, got, want)


def cache(hd, identity, fmt):
    """Device cache covering BOUND positions: (kc, vc, scales or (), table)."""
    g = torch.Generator().manual_seed(hd * 1009 + identity)
    npg = BOUND // PAGE + 2
    table = (torch.arange(npg) if identity else
             torch.randperm(npg, generator=g)).to(torch.int32)
    kc = torch.randn(npg, PAGE, KH, hd, generator=g).bfloat16()
    vc = torch.randn(npg, PAGE, KH, hd, generator=g).bfloat16()
    scales = ()
    if fmt == "fp8":
        kc, ks = torch_ref.quantize_kv_fp8(kc)
        vc, vs = torch_ref.quantize_kv_fp8(vc)
        # [n_pages, page, kh] -> [n_pages, kh, page]
        scales = (ks.permute(0, 2, 1).contiguous().to(DEV),
                  vs.permute(0, 2, 1).contiguous().to(DEV))
    return kc.to(DEV), vc.to(DEV), scales, table.to(DEV)


def run(fmt, hd, group, identity, seq, split_blocks, pos=None):
    kc, vc, scales, table = cache(hd, identity, fmt)
    g = torch.Generator().manual_seed(hd * 101 + group)
    q = torch.randn(KH * group, hd, generator=g).bfloat16().to(DEV)
    fn = ops.attn_decode_paged_fp8 if fmt == "fp8" else ops.attn_decode_paged
    pos_state = None if pos is None else torch.tensor(
        [pos], dtype=torch.int32, device=DEV)
    out = fn(q, kc, vc, *scales, table, seq, None, pos_state=pos_state,
             identity=identity, split_blocks=split_blocks)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    return hashlib.sha256(
        out.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    assert ops.hip_available(), "HIP extension not built"
    for fmt in ("bf16", "fp8"):
        for hd in (32, 64, 128):
            for group in (2, 3, 8):
                for identity in (False, True):
                    for seq, sb, tiles in GEOMETRIES:
                        check_geometry(seq, sb, tiles)
                        print(f"{fmt:4s} hd={hd:3d} g={group} "
                              f"ident={int(identity)} seq={seq} "
                              f"{run(fmt, hd, group, identity, seq, sb)}",
                              flush=True)
            check_geometry(GRAPH_POS + 1, 0, GRAPH_TILES, bound=BOUND)
            print(f"{fmt:4s} hd={hd:3d} g=2 ident=0 graph pos={GRAPH_POS} "
                  f"{run(fmt, hd, 2, False, BOUND, 0, pos=GRAPH_POS)}",
                  flush=True)


if __name__ == "__main__":
    main()
