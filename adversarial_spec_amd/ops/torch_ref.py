"""Plain-PyTorch fp32 reference implementations of every engine op.

These are the numerics oracle for the CDNA4 HIP kernels (tests compare the
HIP path against this fp32 reference, see tests/test_ops_gpu.py) and the
CPU execution path for plumbing tests and BASELINE config 1.

All functions accept/return torch tensors and compute in fp32 regardless of
input dtype (casting back at the end), matching the kernels' fp32
accumulation.
"""

from __future__ import annotations

import math
from typing import Optional, Tuple

import torch


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    """y = x / rms(x) * w, rowwise over the last dim."""
    xf = x.float()
    inv = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (xf * inv * w.float()).to(x.dtype)


def add_rmsnorm(
    resid: torch.Tensor, delta: torch.Tensor, w: torch.Tensor, eps: float
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Fused residual add + RMSNorm: resid' = resid + delta; y = rmsnorm(resid').

    On GPU this is one kernel (one read + one write of the residual stream
    instead of two passes over HBM).
    """
    r = (resid.float() + delta.float())
    inv = torch.rsqrt(r.pow(2).mean(-1, keepdim=True) + eps)
    y = r * inv * w.float()
    return r.to(resid.dtype), y.to(resid.dtype)


def rope_tables(
    head_dim: int, max_seq: int, theta: float, device, dtype=torch.float32
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Precomputed cos/sin tables [max_seq, head_dim/2] (host side, once).

    On-device trig per element would turn the memory-bound RoPE kernel into
    a VALU-bound one (cdna_hip_programming.md Appendix B), so tables are
    precomputed.
    """
    half = head_dim // 2
    freqs = 1.0 / (theta ** (torch.arange(half, device=device, dtype=torch.float64) / half))
    pos = torch.arange(max_seq, device=device, dtype=torch.float64)
    ang = torch.outer(pos, freqs)
    return ang.cos().to(dtype), ang.sin().to(dtype)


def rope(
    q: torch.Tensor, k: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos0: int
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Rotary embedding, interleaved-pair convention.

    q: [t, n_heads, hd], k: [t, n_kv_heads, hd]; rotates pairs
    (x[2i], x[2i+1]) by the angle for absolute position pos0+row.
    (HF-format weights are permuted at load time to this convention.)
    """
    t = q.shape[0]
    c = cos[pos0 : pos0 + t].unsqueeze(1)  # [t,1,hd/2]
    s = sin[pos0 : pos0 + t].unsqueeze(1)

    def rot(x: torch.Tensor) -> torch.Tensor:
        xf = x.float()
        ev = xf[..., 0::2]
        od = xf[..., 1::2]
        out = torch.empty_like(xf)
        out[..., 0::2] = ev * c - od * s
        out[..., 1::2] = ev * s + od * c
        return out.to(x.dtype)

    return rot(q), rot(k)


def swiglu(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    """silu(gate) * up, fused elementwise."""
    g = gate.float()
    return (g * torch.sigmoid(g) * up.float()).to(gate.dtype)


def attn_prefill(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    scale: Optional[float] = None,
    causal: bool = True,
    kv_offset: int = 0,
    window: int = 0,
) -> torch.Tensor:
    """Full prefill attention with GQA.

    q: [tq, n_heads, hd]; k, v: [tk, n_kv_heads, hd]. Causal mask aligns
    query row i with absolute position kv_offset + i (for chunked prefill
    tk >= tq and earlier keys are always visible).
    window = W >= 1 (causal only): the query at absolute position i sees
    keys max(0, i - W + 1) .. i, W keys including itself; 0 = no window.
    Returns [tq, n_heads, hd].
    """
    if window < 0 or (window and not causal):
        raise ValueError("attn_prefill: window >= 0, and 0 unless causal")
    tq, h, hd = q.shape
    tk, kh, _ = k.shape
    if scale is None:
        scale = 1.0 / math.sqrt(hd)
    group = h // kh
    qf = q.float().permute(1, 0, 2)  # [h, tq, hd]
    kf = k.float().permute(1, 0, 2)  # [kh, tk, hd]
    vf = v.float().permute(1, 0, 2)
    kf = kf.repeat_interleave(group, dim=0)  # [h, tk, hd]
    vf = vf.repeat_interleave(group, dim=0)
    scores = torch.bmm(qf, kf.transpose(1, 2)) * scale  # [h, tq, tk]
    if causal:
        qpos = torch.arange(tq, device=q.device).unsqueeze(1) + kv_offset
        kpos = torch.arange(tk, device=q.device).unsqueeze(0)
        mask = kpos > qpos  # future keys
        if window:
            mask = mask | (kpos < qpos - window + 1)  # below the window
        scores = scores.masked_fill(mask.unsqueeze(0), float("-inf"))
    p = torch.softmax(scores, dim=-1)
    out = torch.bmm(p, vf)  # [h, tq, hd]
    return out.permute(1, 0, 2).contiguous().to(q.dtype)


def attn_decode_paged(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    page_table: torch.Tensor,
    seq_len: int,
    scale: Optional[float] = None,
    window: int = 0,
) -> torch.Tensor:
    """Single-token decode attention over a paged KV cache.

    q: [n_heads, hd]; k_cache/v_cache: [n_pages, page_size, n_kv_heads, hd];
    page_table: int32 [n_used_pages] mapping logical page -> physical page.
    Attends to positions [0, seq_len), or with window = W >= 1 to
    [max(0, seq_len - W), seq_len). Returns [n_heads, hd].
    """
    if window < 0:
        raise ValueError("attn_decode_paged: window >= 0")
    h, hd = q.shape
    npg, ps, kh, _ = k_cache.shape
    if scale is None:
        scale = 1.0 / math.sqrt(hd)
    n_used = (seq_len + ps - 1) // ps
    phys = page_table[:n_used].long()
    k = k_cache[phys].reshape(n_used * ps, kh, hd)[:seq_len]  # [t, kh, hd]
    v = v_cache[phys].reshape(n_used * ps, kh, hd)[:seq_len]
    if window:
        k, v = k[max(0, seq_len - window):], v[max(0, seq_len - window):]
    group = h // kh
    qf = q.float()  # [h, hd]
    kf = k.float().repeat_interleave(group, dim=1).permute(1, 0, 2)  # [h, t, hd]
    vf = v.float().repeat_interleave(group, dim=1).permute(1, 0, 2)
    scores = torch.einsum("hd,htd->ht", qf, kf) * scale
    p = torch.softmax(scores, dim=-1)
    out = torch.einsum("ht,htd->hd", p, vf)
    return out.to(q.dtype)


def kv_write(
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    page_table: torch.Tensor,
    pos0: int,
    k: torch.Tensor,
    v: torch.Tensor,
) -> None:
    """Scatter t new K/V rows into the paged cache at positions pos0..pos0+t-1."""
    npg, ps, kh, hd = k_cache.shape
    t = k.shape[0]
    pos = torch.arange(pos0, pos0 + t, device=k.device)
    pages = page_table[(pos // ps).long()].long()
    flat = pages * ps + (pos % ps)
    k_cache.view(npg * ps, kh, hd)[flat] = k.to(k_cache.dtype)
    v_cache.view(npg * ps, kh, hd)[flat] = v.to(v_cache.dtype)


# ---- fp8 (e4m3fn) KV cache -------------------------------------------------
# Storage contract (shared with ops/hip/kv_fp8.hip):
#   k_cache, v_cache  uint8 [n_pages, page, kh, hd], OCP e4m3fn bytes
#   k_scale, v_scale  f32   [n_pages, kh, page] (head-major inside a page)
# One scale per (position, kv-head) row of hd elements:
#   scale = max(amax|x|, 1e-12) / 448 in fp32;  q = e4m3fn_rne(x / scale)
# — the rule of ops.quantize_fp8_rowwise, with a quantized zero always
# stored as byte 0x00. K is quantized after RoPE.

def quantize_kv_fp8(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [..., hd] -> (uint8 [..., hd], f32 scale [...]), one scale per row."""
    xf = x.float()
    scale = xf.abs().amax(dim=-1).clamp_min(1e-12) / 448.0
    q = (xf / scale.unsqueeze(-1)).to(torch.float8_e4m3fn).view(torch.uint8)
    # a quantized zero is always byte 0x00 (never -0 = 0x80): an all-zero
    # row is all zero bytes even where RoPE left -0.0 in it
    q = torch.where((q & 0x7F) == 0, torch.zeros_like(q), q)
    return q.contiguous(), scale.contiguous()


def dequantize_kv_fp8(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """Inverse of quantize_kv_fp8 in fp32: exact fp8 -> f32, one multiply."""
    return q.view(torch.float8_e4m3fn).float() * scale.unsqueeze(-1)


def kv_write_fp8(
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    k_scale: torch.Tensor,
    v_scale: torch.Tensor,
    page_table: torch.Tensor,
    pos0: int,
    k: torch.Tensor,
    v: torch.Tensor,
) -> None:
    """Quantize t new K/V rows [t, kh, hd] and scatter bytes and scales into
    the paged fp8 cache at positions pos0..pos0+t-1."""
    npg, ps, kh, hd = k_cache.shape
    t = k.shape[0]
    pos = torch.arange(pos0, pos0 + t, device=k.device)
    pages = page_table[(pos // ps).long()].long()
    inpage = pos % ps
    flat = pages * ps + inpage
    for cache, sc, x in ((k_cache, k_scale, k), (v_cache, v_scale, v)):
        q8, s = quantize_kv_fp8(x)
        cache.view(npg * ps, kh, hd)[flat] = q8
        sc[pages, :, inpage] = s


def dequant_cache_fp8(cache: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """Whole fp8 page pool -> fp32 [n_pages, page, kh, hd]."""
    return dequantize_kv_fp8(cache, scale.permute(0, 2, 1))


def kv_dequant_fp8(
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    k_scale: torch.Tensor,
    v_scale: torch.Tensor,
    page_table: torch.Tensor,
    n: int,
    dtype: torch.dtype = torch.bfloat16,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Positions [0, n) of an fp8 cache as contiguous [n, kh, hd] tensors of
    `dtype`, through the page table: one fp32 multiply, one rounding."""
    npg, ps, kh, hd = k_cache.shape
    n_used = (n + ps - 1) // ps
    phys = page_table[:n_used].long()
    outs = []
    for cache, sc in ((k_cache, k_scale), (v_cache, v_scale)):
        full = dequant_cache_fp8(cache[phys], sc[phys])
        outs.append(full.reshape(n_used * ps, kh, hd)[:n].to(dtype).contiguous())
    return outs[0], outs[1]


def attn_decode_paged_fp8(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    k_scale: torch.Tensor,
    v_scale: torch.Tensor,
    page_table: torch.Tensor,
    seq_len: int,
    scale: Optional[float] = None,
    window: int = 0,
) -> torch.Tensor:
    """attn_decode_paged over the dequantized (fp32) positions [0, seq_len)
    of an fp8 cache (the last `window` of them when window > 0); nothing at
    or past seq_len is read."""
    ps = k_cache.shape[1]
    n_used = (seq_len + ps - 1) // ps
    k, v = kv_dequant_fp8(k_cache, v_cache, k_scale, v_scale, page_table,
                          seq_len, torch.float32)
    pad = n_used * ps - seq_len
    if pad:
        k = torch.cat([k, k.new_zeros(pad, *k.shape[1:])])
        v = torch.cat([v, v.new_zeros(pad, *v.shape[1:])])
    ident = torch.arange(n_used, dtype=page_table.dtype, device=q.device)
    return attn_decode_paged(
        q, k.view(n_used, ps, *k.shape[1:]), v.view(n_used, ps, *v.shape[1:]),
        ident, seq_len, scale, window)


def sample(
    logits: torch.Tensor,
    temperature: float = 0.7,
    top_p: float = 1.0,
    generator: Optional[torch.Generator] = None,
) -> int:
    """Temperature + nucleus sampling over a [vocab] logits row."""
    lf = logits.float()
    if temperature <= 0.0:
        return int(lf.argmax().item())
    probs = torch.softmax(lf / temperature, dim=-1)
    if top_p < 1.0:
        sp, idx = probs.sort(descending=True)
        cum = sp.cumsum(-1)
        keep = cum - sp < top_p  # keep tokens whose prefix-before is < top_p
        sp = sp * keep
        sp = sp / sp.sum()
        choice = torch.multinomial(sp, 1, generator=generator)
        return int(idx[choice].item())
    choice = torch.multinomial(probs, 1, generator=generator)
    return int(choice.item())


def nucleus_mass_above(
    logits: torch.Tensor, temperature: float
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per token of a [vocab] row, in float64: G, the softmax(logits / T)
    probability of the tokens whose logit is strictly greater, and C, their
    number (int64). Equal logits form one group and share (G, C); +0.0 and
    -0.0 are equal (the row is taken `+ 0.0`, which turns -0.0 into +0.0
    before grouping)."""
    lf = logits.detach().reshape(-1).to(torch.float64) + 0.0
    vals, inv, counts = torch.unique(
        lf, sorted=True, return_inverse=True, return_counts=True)
    w = torch.exp((vals - vals.max()) / temperature) * counts
    gm = (w / w.sum()).flip(0)        # group masses, descending logit
    gc = counts.flip(0)
    zero = gm.new_zeros(1)
    g_above = torch.cat([zero, gm.cumsum(0)[:-1]]).flip(0)
    c_above = torch.cat([gc.new_zeros(1), gc.cumsum(0)[:-1]]).flip(0)
    return g_above[inv], c_above[inv]


def nucleus_keep(
    logits: torch.Tensor, temperature: float, top_p: float, top_k: int = 0
) -> torch.Tensor:
    """The kept set of top-p / top-k filtering as bool [vocab]: token i is
    kept iff G(i) < top_p and (top_k == 0 or C(i) < top_k), with G and C as
    in nucleus_mass_above. A group of equal logits is kept or dropped whole
    (the one difference from `sample`'s sorted-prefix rule, whose order
    among equal elements is arbitrary), the argmax group is always kept,
    and temperature <= 0 keeps the argmax group alone."""
    if temperature <= 0.0:
        lf = logits.detach().reshape(-1).to(torch.float64)
        return lf == lf.max()
    g_above, c_above = nucleus_mass_above(logits, temperature)
    # in real arithmetic G < 1 for every token; in float64 a tail of zero
    # weight rounds G up to 1.0, so top_p >= 1 is decided here, not compared
    keep = g_above < top_p if top_p < 1.0 else torch.ones_like(g_above,
                                                               dtype=torch.bool)
    if top_k > 0:
        keep &= c_above < top_k
    return keep


def sample_filtered(
    logits: torch.Tensor,
    temperature: float,
    top_p: float,
    top_k: int = 0,
    generator: Optional[torch.Generator] = None,
) -> int:
    """A draw from softmax(logits / T) restricted to nucleus_keep and
    renormalised; temperature <= 0 is the argmax (lowest index on ties)."""
    lf = logits.detach().reshape(-1).to(torch.float64)
    if temperature <= 0.0:
        return int((lf == lf.max()).nonzero()[0].item())
    keep = nucleus_keep(logits, temperature, top_p, top_k)
    probs = torch.softmax(lf / temperature, dim=-1) * keep
    probs = probs / probs.sum()
    choice = torch.multinomial(probs, 1, generator=generator)
    return int(choice.item())
