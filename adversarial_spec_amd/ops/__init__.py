"""Op dispatch: CDNA4 HIP kernels on GPU, fp32 torch reference on CPU.

Single code path per device class — no multi-backend dispatch tables, no
Triton, no CUDA shims. On a CUDA(HIP) tensor the hand-written gfx950
extension `_advspec_hip` is REQUIRED: a missing extension raises instead of
silently falling back to eager PyTorch (the round-end harness records which
.so the GPU actually loaded).

CPU tensors use the fp32 reference in `torch_ref` (tests, BASELINE config 1).
"""

from __future__ import annotations

import math
import os
from typing import Optional, Tuple

import torch

from ..providers import validate_sampling_filter
from . import torch_ref

_hip = None
_hip_err: Optional[str] = None


def _load_hip():
    global _hip, _hip_err
    if _hip is not None or _hip_err is not None:
        return _hip
    try:
        from . import _advspec_hip  # built in-tree by setup.py build_ext --inplace

        _hip = _advspec_hip
    except ImportError as e:
        _hip_err = str(e)
    return _hip


def hip_available() -> bool:
    return _load_hip() is not None


def _require_hip():
    mod = _load_hip()
    if mod is None:
        raise RuntimeError(
            "adversarial_spec_amd HIP extension (_advspec_hip) is not built "
            f"but a GPU tensor was passed. Build it with `python setup.py "
            f"build_ext --inplace` (PYTORCH_ROCM_ARCH=gfx950) or via "
            f"__graft_entry__.build(). Import error: {_hip_err}"
        )
    return mod


def _on_gpu(x: torch.Tensor) -> bool:
    return x.is_cuda


def _attn_scale(q: torch.Tensor, scale: Optional[float]) -> float:
    """The softmax scale the kernels take: 1/sqrt(hd) unless given."""
    return scale if scale is not None else 1.0 / math.sqrt(q.shape[-1])


# --------------------------------------------------------------------------
# Public ops. Shapes documented in torch_ref (the contract is identical).
# --------------------------------------------------------------------------

def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    if _on_gpu(x):
        return _require_hip().rmsnorm(x, w, eps, out)
    return torch_ref.rmsnorm(x, w, eps)


def add_rmsnorm(
    resid: torch.Tensor, delta: torch.Tensor, w: torch.Tensor, eps: float,
    out_resid: Optional[torch.Tensor] = None,
    out_y: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    if _on_gpu(resid):
        return _require_hip().add_rmsnorm(resid, delta, w, eps, out_resid, out_y)
    return torch_ref.add_rmsnorm(resid, delta, w, eps)


def rope(
    q: torch.Tensor, k: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos0: int,
    pos_state: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    if _on_gpu(q):
        _require_hip().rope_inplace(q, k, cos, sin, pos0, pos_state)
        return q, k
    return torch_ref.rope(q, k, cos, sin, pos0)


def swiglu(gate: torch.Tensor, up: torch.Tensor,
           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    if _on_gpu(gate):
        return _require_hip().swiglu(gate, up, out)
    return torch_ref.swiglu(gate, up)


def attn_prefill(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    scale: Optional[float] = None,
    causal: bool = True,
    kv_offset: int = 0,
    window: int = 0,
) -> torch.Tensor:
    """window = W >= 1 (causal only) is a sliding window: the query at
    absolute position i sees keys max(0, i - W + 1) .. i; 0 = off."""
    if _on_gpu(q):
        return _require_hip().attn_prefill(q, k, v, _attn_scale(q, scale),
                                           causal, kv_offset, window)
    return torch_ref.attn_prefill(q, k, v, scale, causal, kv_offset, window)


def attn_decode_paged(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    page_table: torch.Tensor,
    seq_len: int,
    scale: Optional[float] = None,
    pos_state: Optional[torch.Tensor] = None,
    out: Optional[torch.Tensor] = None,
    identity: bool = False,
    split_blocks: int = 0,
    window: int = 0,
) -> torch.Tensor:
    """identity=True promises page_table[i] == i (the engine's single-pool
    cache): the split kernel then does pure address math — the per-lane
    table read otherwise forces a DMA-queue drain per staged tile.
    split_blocks>0 sets the split-grid block target (the engine passes its
    concurrency-aware pick; ADVSPEC_SPLIT_BLOCKS still overrides).
    With pos_state (graph mode) the true length is *pos_state + 1 in-kernel
    and seq_len is the static max bound sizing the split geometry.
    window = W >= 1 attends the last W positions only, [max(0, len - W), len);
    the split geometry is then sized for min(seq_len, W + 63), whatever the
    live length."""
    if _on_gpu(q):
        return _require_hip().attn_decode_paged(
            q, k_cache, v_cache, page_table, seq_len, _attn_scale(q, scale),
            pos_state, out, identity, split_blocks, window)
    return torch_ref.attn_decode_paged(q, k_cache, v_cache, page_table,
                                       seq_len, scale, window)


def kv_write(
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    page_table: torch.Tensor,
    pos0: int,
    k: torch.Tensor,
    v: torch.Tensor,
    pos_state: Optional[torch.Tensor] = None,
) -> None:
    if _on_gpu(k_cache):
        _require_hip().kv_write(k_cache, v_cache, page_table, pos0, k, v,
                                pos_state)
        return
    torch_ref.kv_write(k_cache, v_cache, page_table, pos0, k, v)


def rope_kv(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    cos: torch.Tensor,
    sin: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    page_table: torch.Tensor,
    pos0: int,
    pos_state: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Fused RoPE (q,k in place) + paged KV scatter of rotated k and v.
    One launch replaces rope + kv_write on the kernel-count-bound decode
    path. Returns (q, k) rotated."""
    if _on_gpu(q):
        _require_hip().rope_kv(q, k, v, cos, sin, k_cache, v_cache,
                               page_table, pos0, pos_state)
        return q, k
    q2, k2 = torch_ref.rope(q, k, cos, sin, pos0)
    torch_ref.kv_write(k_cache, v_cache, page_table, pos0, k2, v)
    return q2, k2


# ---- fp8 (e4m3fn) KV cache (storage contract in torch_ref) -----------------

def rope_kv_fp8(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    cos: torch.Tensor,
    sin: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    k_scale: torch.Tensor,
    v_scale: torch.Tensor,
    page_table: torch.Tensor,
    pos0: int,
    pos_state: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp8 twin of rope_kv: rotates q and k in place (bit-identical to
    rope_kv) and appends the rotated k and v rowwise-quantized to e4m3fn,
    one fp32 scale per (position, kv-head) row, in one launch. Returns
    (q, k) rotated."""
    if _on_gpu(q):
        _require_hip().rope_kv_fp8(q, k, v, cos, sin, k_cache, v_cache,
                                   k_scale, v_scale, page_table, pos0,
                                   pos_state)
        return q, k
    if pos_state is not None:
        pos0 = int(pos_state.reshape(-1)[0])
    q2, k2 = torch_ref.rope(q, k, cos, sin, pos0)
    torch_ref.kv_write_fp8(k_cache, v_cache, k_scale, v_scale, page_table,
                           pos0, k2, v)
    return q2, k2


def attn_decode_paged_fp8(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    k_scale: torch.Tensor,
    v_scale: torch.Tensor,
    page_table: torch.Tensor,
    seq_len: int,
    scale: Optional[float] = None,
    pos_state: Optional[torch.Tensor] = None,
    out: Optional[torch.Tensor] = None,
    identity: bool = False,
    split_blocks: int = 0,
    window: int = 0,
) -> torch.Tensor:
    """attn_decode_paged over an fp8 cache: same arguments plus the two
    scale tensors; the dequantization is folded into the split kernel (K
    scale on the score, V scale on p), the combine pass and the split
    geometry are the bf16 ones."""
    if _on_gpu(q):
        return _require_hip().attn_decode_paged_fp8(
            q, k_cache, v_cache, k_scale, v_scale, page_table, seq_len,
            _attn_scale(q, scale), pos_state, out, identity, split_blocks,
            window)
    if pos_state is not None:
        seq_len = int(pos_state.reshape(-1)[0]) + 1
    return torch_ref.attn_decode_paged_fp8(
        q, k_cache, v_cache, k_scale, v_scale, page_table, seq_len, scale,
        window)


def kv_dequant_fp8(
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    k_scale: torch.Tensor,
    v_scale: torch.Tensor,
    page_table: torch.Tensor,
    n: int,
    dtype: Optional[torch.dtype] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Positions [0, n) of one layer's fp8 cache as contiguous (k, v)
    [n, kh, hd], through the page table; bf16 on GPU (bit-exact: exact
    fp8 -> f32, one fp32 multiply, one rounding), where any other `dtype`
    is an error; the CPU reference honours `dtype` (default bf16).
    Chunked prefill only."""
    if _on_gpu(k_cache):
        if dtype not in (None, torch.bfloat16):
            raise ValueError(
                f"kv_dequant_fp8 returns bf16 on GPU, not {dtype}")
        return _require_hip().kv_dequant_fp8(k_cache, v_cache, k_scale,
                                             v_scale, page_table, n)
    return torch_ref.kv_dequant_fp8(k_cache, v_cache, k_scale, v_scale,
                                    page_table, n, dtype or torch.bfloat16)


def gemv(x: torch.Tensor, w: torch.Tensor,
         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Batch-1 matmul y = x @ w^T, weights ROW-MAJOR [out, in] (HF layout).
    On GPU, a hand-written weight-streaming kernel (decode's dominant cost
    is reading w once from HBM3E)."""
    if _on_gpu(x):
        return _require_hip().gemv(x, w, out)
    return x @ w.t()


def gemv_gateup(x: torch.Tensor, w_gate_up: torch.Tensor,
                out: torch.Tensor) -> torch.Tensor:
    """Fused decode MLP front half: act = silu(x @ Wg^T) * (x @ Wu^T) with
    w_gate_up = [gate rows | up rows] (the fused HF layout). One launch
    replaces gate_up GEMV + swiglu on the kernel-count-bound decode path."""
    if _on_gpu(x):
        _require_hip().gemv_gateup(x, w_gate_up, out)
        return out
    f = w_gate_up.shape[0] // 2
    gu = x @ w_gate_up.t()
    y = torch_ref.swiglu(gu[..., :f], gu[..., f:])
    out.copy_(y.reshape(out.shape))
    return out


def _rms_ref(x: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    return torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)


def gemv_norm(x: torch.Tensor, wln: torch.Tensor, w: torch.Tensor, eps: float,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Decode fusion: y = rmsnorm(x, wln, eps) @ w^T in ONE launch — the
    scalar rms factor commutes out of the dot, so the GEMV accumulates the
    wln-weighted dot and sum(x^2) from the x chunks it already streams.
    Replaces the separate (add_)rmsnorm launch before every consuming
    decode GEMV (0.30 ms/tok of launch-bound kernels, see profiles)."""
    if _on_gpu(x):
        return _require_hip().gemv_norm(x, wln, w, eps, out)
    y = ((x.float() * _rms_ref(x, eps) * wln.float()) @ w.float().t()).to(x.dtype)
    if out is not None:
        out.copy_(y.reshape(out.shape))
        return out
    return y


def qkv_rope_fusable(hq: int, kh: int, hd: int,
                     cos: Optional[torch.Tensor] = None,
                     sin: Optional[torch.Tensor] = None,
                     k_cache: Optional[torch.Tensor] = None,
                     v_cache: Optional[torch.Tensor] = None) -> bool:
    """Whether the fused qkv + RoPE + KV-append GEMVs accept this call: the
    w32 row geometry (one rotation pair per wave) and, for the tensors that
    are passed, everything their binding insists on (f32 contiguous
    [max_pos, hd/2] tables, contiguous [n_pages, page, kh, hd] caches).
    Anything else runs the GEMV followed by rope_kv."""
    if hd % 16 != 0 or (hq + 2 * kh) * hd > 8192:
        return False
    for t in (cos, sin):
        if t is not None and not (
            t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous()
            and t.shape[1] == hd // 2
        ):
            return False
    if cos is not None and sin is not None and cos.shape != sin.shape:
        return False
    for t in (k_cache, v_cache):
        if t is not None and not (
            t.dtype == torch.bfloat16 and t.dim() == 4 and t.is_contiguous()
            and t.shape[2] == kh and t.shape[3] == hd
        ):
            return False
    if (k_cache is not None and v_cache is not None
            and k_cache.shape != v_cache.shape):
        return False
    return True


def _rope_kv_on_qkv(y: torch.Tensor, hq: int, kh: int, cos, sin, k_cache,
                    v_cache, page_table, pos0: int, pos_state) -> torch.Tensor:
    """CPU composition shared by the fused qkv ops: rope_kv on the q/k/v
    views of the projected row y [1, (hq+2*kh)*hd], written back into y."""
    hd = y.numel() // (hq + 2 * kh)
    if pos_state is not None:
        pos0 = int(pos_state.reshape(-1)[0])
    row = y.view(1, -1)
    q = row[:, : hq * hd].view(1, hq, hd)
    k = row[:, hq * hd : (hq + kh) * hd].view(1, kh, hd)
    v = row[:, (hq + kh) * hd :].view(1, kh, hd)
    q2, k2 = rope_kv(q, k, v, cos, sin, k_cache, v_cache, page_table, pos0)
    q.copy_(q2)
    k.copy_(k2)
    return y


def gemv_norm_rope_kv(
    x: torch.Tensor, wln: torch.Tensor, w: torch.Tensor, eps: float,
    cos: torch.Tensor, sin: torch.Tensor, k_cache: torch.Tensor,
    v_cache: torch.Tensor, page_table: torch.Tensor, pos0: int,
    hq: int, kh: int, pos_state: Optional[torch.Tensor] = None,
    out: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Decode fusion: qkv = rmsnorm(x, wln) @ w^T with RoPE on the q/k
    heads and the rotated k plus v appended to the paged cache at `pos0`
    (`pos_state` in graph mode), in ONE launch. w is the fused [q|k|v]
    projection, (hq + 2*kh)*hd rows. Bit-identical to gemv_norm followed by
    rope_kv on the views of its output; returns that output [1, N]."""
    if _on_gpu(x):
        return _require_hip().gemv_norm_rope_kv(
            x, wln, w, eps, cos, sin, k_cache, v_cache, page_table, pos0,
            hq, kh, pos_state, out)
    y = gemv_norm(x, wln, w, eps).reshape(1, -1).contiguous()
    _rope_kv_on_qkv(y, hq, kh, cos, sin, k_cache, v_cache, page_table, pos0,
                    pos_state)
    if out is not None:
        out.copy_(y.reshape(out.shape))
        return out
    return y


def gemv_fp8_q_rope_kv(
    x8: torch.Tensor, xs: torch.Tensor, w_q: torch.Tensor,
    w_scale: torch.Tensor, out: torch.Tensor, cos: torch.Tensor,
    sin: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
    page_table: torch.Tensor, pos0: int, hq: int, kh: int,
    pos_state: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """fp8 twin of gemv_norm_rope_kv: pre-quantized x8/xs (quant_norm_fp8)
    against the rowwise-e4m3 fused qkv weight. Bit-identical to gemv_fp8_q
    followed by rope_kv."""
    if x8.is_cuda:
        _require_hip().gemv_fp8_q_rope_kv(
            x8, xs, w_q, w_scale, out, cos, sin, k_cache, v_cache,
            page_table, pos0, hq, kh, pos_state)
        return out
    y = torch.empty(1, w_q.shape[0], dtype=out.dtype)
    gemv_fp8_q(x8, xs, w_q, w_scale, y)
    _rope_kv_on_qkv(y, hq, kh, cos, sin, k_cache, v_cache, page_table, pos0,
                    pos_state)
    out.copy_(y.reshape(out.shape))
    return out


def gemv_res(x: torch.Tensor, w: torch.Tensor, resid: torch.Tensor) -> torch.Tensor:
    """Decode fusion: resid += x @ w^T in place (the producing GEMV's
    epilogue adds the residual, so the delta never materializes). NOT valid
    under TP — the all-reduce must see the raw partial projection."""
    if _on_gpu(x):
        _require_hip().gemv_res(x, w, resid)
        return resid
    resid.add_((x.float() @ w.float().t()).to(resid.dtype).reshape(resid.shape))
    return resid


def gemv_gateup_norm(x: torch.Tensor, wln: torch.Tensor, w_gate_up: torch.Tensor,
                     eps: float, out: torch.Tensor) -> torch.Tensor:
    """Decode fusion: act = swiglu(rmsnorm(x) @ [Wg|Wu]^T) in one launch."""
    if _on_gpu(x):
        _require_hip().gemv_gateup_norm(x, wln, w_gate_up, eps, out)
        return out
    normed = (x.float() * _rms_ref(x, eps) * wln.float()).to(x.dtype)
    return gemv_gateup(normed, w_gate_up, out)


def gemm(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """Prefill matmul C = x @ w^T, weights ROW-MAJOR [out, in] (HF layout).
    On GPU the in-tree tiled MFMA kernel — library GEMMs (hipBLASLt/rocBLAS
    Tensile kernels) intermittently return garbage on skinny-m bf16 shapes
    in recycled-memory states, and the in-tree kernel is deterministic and
    workspace-free. CPU uses torch."""
    if _on_gpu(x):
        return _require_hip().gemm(x, w)
    return x @ w.t()


def quantize_fp8_rowwise(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Rowwise OCP e4m3 quantization: returns (q uint8 [N,K], scale f32 [N]).
    Pure torch (runs once at engine init, CPU or GPU)."""
    wf = w.float()
    scale = wf.abs().amax(dim=1).clamp_min(1e-12) / 448.0
    q = (wf / scale[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    return q.contiguous(), scale.contiguous()


def dequantize_fp8(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    return q.view(torch.float8_e4m3fn).float() * scale[:, None]


def gemm_fp8(x: torch.Tensor, w_q: torch.Tensor, w_scale: torch.Tensor) -> torch.Tensor:
    """C = x @ W^T with W rowwise-e4m3-quantized; x is rowwise-quantized
    on the fly. GPU: mfma_f32_16x16x32_fp8_fp8 kernel. CPU: dequantized
    reference (tests)."""
    if _on_gpu(x):
        return _require_hip().gemm_fp8(x, w_q, w_scale)
    xf = x.float()
    xs = xf.abs().amax(dim=1).clamp_min(1e-12) / 448.0
    x8 = (xf / xs[:, None]).to(torch.float8_e4m3fn).float() * xs[:, None]
    return (x8 @ dequantize_fp8(w_q, w_scale).t()).to(x.dtype)


def gemv_fp8(x: torch.Tensor, w_q: torch.Tensor, w_scale: torch.Tensor,
             x8_buf: torch.Tensor, xs_buf: torch.Tensor,
             out: torch.Tensor) -> torch.Tensor:
    """Allocation-free fp8 decode GEMV (graph-capture safe): quantizes x
    into the provided scratch, writes bf16 into out."""
    _require_hip().gemv_fp8(x, w_q, w_scale, x8_buf, xs_buf, out)
    return out


# ---- fp8 decode fusion (mirror of the bf16 gemv_norm/gemv_res fusion) ----

def quant_norm_fp8(x: torch.Tensor, wln: torch.Tensor, x8: torch.Tensor,
                   xs: torch.Tensor, eps: float) -> None:
    """x8, xs[0] = rowwise-e4m3(rmsnorm(x, wln, eps)) in ONE launch: the
    rms scalar commutes, so one pass yields sum(x^2) AND amax(x*wln)."""
    if _on_gpu(x):
        _require_hip().quant_norm_fp8(x, wln, x8, xs, eps)
        return
    normed = (x.float() * _rms_ref(x, eps) * wln.float())
    s = normed.abs().amax().clamp_min(1e-12).item() / 448.0
    k = x.numel()
    q = (normed.flatten() / s).to(torch.float8_e4m3fn).view(torch.uint8)
    x8.flatten()[:k].copy_(q)
    xs[0] = s


def gemv_fp8_q(x8: torch.Tensor, xs: torch.Tensor, w_q: torch.Tensor,
               w_scale: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """Pre-quantized fp8 decode GEMV (x8/xs from quant_norm_fp8)."""
    if x8.is_cuda:
        _require_hip().gemv_fp8_q(x8, xs, w_q, w_scale, out)
        return out
    k = w_q.shape[1]
    xf = x8.flatten()[:k].view(torch.float8_e4m3fn).float() * xs[0]
    out.copy_((xf @ dequantize_fp8(w_q, w_scale).t()).to(out.dtype)
              .reshape(out.shape))
    return out


def gemv_fp8_res(x: torch.Tensor, w_q: torch.Tensor, w_scale: torch.Tensor,
                 x8: torch.Tensor, xs: torch.Tensor,
                 resid: torch.Tensor) -> torch.Tensor:
    """fp8 decode fusion: resid += x @ W^T in place (quantize + GEMV with
    residual epilogue). NOT valid under TP."""
    if _on_gpu(x):
        _require_hip().gemv_fp8_res(x, w_q, w_scale, x8, xs, resid)
        return resid
    y = gemm_fp8(x, w_q, w_scale)
    resid.add_(y.to(resid.dtype).reshape(resid.shape))
    return resid


def gemv_fp8_gateup(x8: torch.Tensor, xs: torch.Tensor, w_q: torch.Tensor,
                    w_scale: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """Pre-quantized fused fp8 gate_up GEMV + SwiGLU."""
    if x8.is_cuda:
        _require_hip().gemv_fp8_gateup(x8, xs, w_q, w_scale, out)
        return out
    f = w_q.shape[0] // 2
    k = w_q.shape[1]
    xf = x8.flatten()[:k].view(torch.float8_e4m3fn).float() * xs[0]
    gu = xf @ dequantize_fp8(w_q, w_scale).t()
    out.copy_(torch_ref.swiglu(gu[:f].unsqueeze(0), gu[f:].unsqueeze(0))
              .to(out.dtype).reshape(out.shape))
    return out


# LDS-staged single-launch fp8 fused GEMVs (each GEMV block quantizes its
# own activation copy into LDS; removes the serial 1-block quant kernels):

def gemv_fp8_norm(x: torch.Tensor, wln: torch.Tensor, w_q: torch.Tensor,
                  w_scale: torch.Tensor, eps: float,
                  out: torch.Tensor) -> torch.Tensor:
    """out = rmsnorm(x, wln, eps) @ W^T in ONE launch (fp8 weights)."""
    if _on_gpu(x):
        _require_hip().gemv_fp8_norm(x, wln, w_q, w_scale, eps, out)
        return out
    normed = (x.float() * _rms_ref(x, eps) * wln.float())
    s = float(normed.abs().amax().clamp_min(1e-12)) / 448.0
    n8 = (normed / s).to(torch.float8_e4m3fn).float() * s
    out.copy_((n8 @ dequantize_fp8(w_q, w_scale).t()).to(out.dtype)
              .reshape(out.shape))
    return out


def gemv_fp8_resl(x: torch.Tensor, w_q: torch.Tensor, w_scale: torch.Tensor,
                  resid: torch.Tensor) -> torch.Tensor:
    """resid += x @ W^T in place, one launch (fp8 weights, x quantized
    in-kernel). NOT valid under TP."""
    if _on_gpu(x):
        _require_hip().gemv_fp8_resl(x, w_q, w_scale, resid)
        return resid
    resid.add_(gemm_fp8(x, w_q, w_scale).to(resid.dtype).reshape(resid.shape))
    return resid


def gemv_fp8_gateup_norm(x: torch.Tensor, wln: torch.Tensor,
                         w_q: torch.Tensor, w_scale: torch.Tensor,
                         eps: float, out: torch.Tensor) -> torch.Tensor:
    """out = swiglu(rmsnorm(x, wln) @ [Wg|Wu]^T), one launch."""
    if _on_gpu(x):
        _require_hip().gemv_fp8_gateup_norm(x, wln, w_q, w_scale, eps, out)
        return out
    f = w_q.shape[0] // 2
    normed = (x.float() * _rms_ref(x, eps) * wln.float())
    s = float(normed.abs().amax().clamp_min(1e-12)) / 448.0
    n8 = (normed / s).to(torch.float8_e4m3fn).float() * s
    gu = n8 @ dequantize_fp8(w_q, w_scale).t()
    out.copy_(torch_ref.swiglu(gu[..., :f], gu[..., f:]).to(out.dtype)
              .reshape(out.shape))
    return out


def sample(
    logits: torch.Tensor,
    temperature: float = 0.7,
    top_p: float = 1.0,
    generator: Optional[torch.Generator] = None,
    seed: Optional[int] = None,
) -> int:
    if _on_gpu(logits):
        if top_p < 1.0:
            # exact nucleus needs a sorted vocab: cold path (default decode
            # samples at top_p == 1, reference models.py:626)
            return torch_ref.sample(logits.float().cpu(), temperature, top_p, generator)
        # Device-side fused temperature/softmax sampling kernel; the random
        # draw comes from a host-provided seed counter so HIP-graph replays
        # stay deterministic.
        if seed is None:
            seed = int(torch.randint(0, 2**31 - 1, (1,)).item())
        return int(_require_hip().sample(logits, temperature, top_p, seed))
    return torch_ref.sample(logits, temperature, top_p, generator)


def sample_filtered(
    logits: torch.Tensor,
    temperature: float = 0.7,
    top_p: float = 1.0,
    top_k: int = 0,
    generator: Optional[torch.Generator] = None,
    seed: Optional[int] = None,
) -> int:
    """Top-p / top-k filtered draw from a [vocab] logits row (the kept set
    is torch_ref.nucleus_keep's). On GPU one kernel finds the cut and draws,
    seeded by `seed`; on CPU the float64 reference draws with `generator`."""
    top_p, top_k = validate_sampling_filter(top_p, top_k)
    if _on_gpu(logits):
        if seed is None:
            seed = int(torch.randint(0, 2**31 - 1, (1,)).item())
        return int(_require_hip().sample_filtered(
            logits, temperature, top_p, top_k, seed))
    return torch_ref.sample_filtered(logits, temperature, top_p, top_k,
                                     generator)


def nucleus_mask(logits: torch.Tensor, temperature: float, top_p: float,
                 top_k: int = 0) -> torch.Tensor:
    """The kept set of sample_filtered as bool [vocab]; on GPU it comes from
    the sampling kernels' own cut."""
    top_p, top_k = validate_sampling_filter(top_p, top_k)
    if _on_gpu(logits):
        return _require_hip().nucleus_mask(
            logits, temperature, top_p, top_k).bool()
    return torch_ref.nucleus_keep(logits, temperature, top_p, top_k)
