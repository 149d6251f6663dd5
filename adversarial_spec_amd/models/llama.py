"""Llama-family model for the MI355X engine.

Design (MI355X-first, not a port):
  - weights live as plain bf16 tensors in HBM3E (288 GB/GPU lets several
    opponent models co-reside) in ROW-MAJOR [out, in] — exactly the HF
    checkpoint layout, zero load-time transposes; the in-tree MFMA GEMM
    and row-dot GEMV compute x @ W^T natively (optionally e4m3-quantized
    rowwise for the fp8 path);
  - QKV and gate/up projections are fused into single GEMMs;
  - the residual stream is updated by a fused add+RMSNorm HIP kernel (one
    HBM round-trip instead of two — the ~8 TB/s HBM is the usual bound);
  - RoPE uses host-precomputed cos/sin tables (interleaved-pair
    convention; HF checkpoint weights are permuted at load);
  - KV cache is paged ([n_pages, page_size, n_kv_heads, head_dim]) with a
    per-sequence page table, read directly by the decode attention kernel;
  - prefill attention is a flash-style CDNA4 MFMA kernel over the freshly
    computed contiguous K/V of the prompt.

Replaces the reference's remote `completion()` call.
"""

from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import Optional

import torch

# hipBLASLt's skinny-m bf16 GEMMs intermittently return garbage (~1e33
# finite values) on first use in recycled-memory states (round-1 debugging:
# L0 qkv amax 4.6e33 from clean inputs, flaky by allocation layout, both
# prompt-sized m=36 and m=56). Route torch matmuls through rocBLAS until
# the in-tree MFMA GEMM replaces library GEMMs on the prefill path.
if torch.cuda.is_available():  # pragma: no cover - GPU only
    try:
        torch.backends.cuda.preferred_blas_library("cublas")
    except Exception:
        pass

from .. import ops
from ..ops import torch_ref
from .config import LlamaConfig


@dataclass
class QuantW:
    """Rowwise e4m3-quantized projection: q uint8 [out, in], scale f32 [out]."""
    q: torch.Tensor
    s: torch.Tensor


@dataclass
class LayerWeights:
    # all projection weights ROW-MAJOR [out, in] (HF layout; x @ W^T)
    attn_norm: torch.Tensor  # [d]
    wqkv: torch.Tensor  # [(h + 2*kh) * hd, d]
    wo: torch.Tensor  # [d, h*hd]
    mlp_norm: torch.Tensor  # [d]
    w_gate_up: torch.Tensor  # [2*ffn, d]
    w_down: torch.Tensor  # [d, ffn]


KV_DTYPES = ("bf16", "fp8")


class PagedKVCache:
    """Block-table KV cache: physical pages of `page_size` tokens.

    With 288 GB of HBM3E a debate sequence never needs eviction; the page
    indirection exists so several co-resident opponents can draw from one
    pool and so decode attention is cache-layout independent.
    """

    def __init__(self, config: LlamaConfig, max_seq: int, device, dtype,
                 page_size: int = 256, kv_dtype: str = "bf16") -> None:
        if kv_dtype not in KV_DTYPES:
            raise ValueError(
                f"kv_dtype must be one of {KV_DTYPES}, got {kv_dtype!r}")
        self.kv_dtype = kv_dtype
        self.page_size = page_size
        n_pages = (max_seq + page_size - 1) // page_size
        kh, hd = config.n_kv_heads, config.head_dim
        nl = config.n_layers
        # per-layer page pools: [n_layers, n_pages, page_size, kh, hd]
        if kv_dtype == "fp8":
            # opt-in e4m3fn storage (contract in ops/torch_ref.py): 1-byte
            # elements plus one f32 scale per (position, kv-head) row,
            # [n_layers, n_pages, kh, page_size] — head-major inside a page
            # so a decode tile's scales are contiguous.
            self.k = torch.zeros(nl, n_pages, page_size, kh, hd, device=device,
                                 dtype=torch.uint8)
            self.v = torch.zeros_like(self.k)
            self.k_scale = torch.zeros(nl, n_pages, kh, page_size,
                                       device=device, dtype=torch.float32)
            self.v_scale = torch.zeros_like(self.k_scale)
        else:
            self.k = torch.zeros(nl, n_pages, page_size, kh, hd, device=device, dtype=dtype)
            self.v = torch.zeros(nl, n_pages, page_size, kh, hd, device=device, dtype=dtype)
            self.k_scale = self.v_scale = None
        # identity mapping by default; kept as a real table for paged reads.
        # `identity` certifies page_table[i] == i to the kernels (pure
        # address math, no table read) and to chunked prefill (which views
        # the pool as contiguous [seq, kh, hd]); any future eviction logic
        # must clear it.
        self.page_table = torch.arange(n_pages, device=device, dtype=torch.int32)
        self.identity = True
        self.seq_len = 0
        self.max_seq = n_pages * page_size

    def reset(self) -> None:
        self.seq_len = 0


class DecodeWorkspace:
    """Preallocated buffers for the single-token decode step.

    The captured HIP-graph step must perform ZERO torch allocations:
    allocator traffic during stream capture corrupts the caching
    allocator's bookkeeping on this torch/ROCm combo (later engines'
    freshly-allocated prefill buffers alias, producing flaky NaN logits —
    round-1 debugging). A static workspace also removes per-step allocator
    overhead from eager decode.
    """

    def __init__(self, model: "LlamaModel") -> None:
        c = model.config
        dev, dt = model.device, model.dtype
        h, kh, hd = c.n_heads, c.n_kv_heads, c.head_dim

        def mk(*shape):
            return torch.empty(*shape, device=dev, dtype=dt)

        self.resid = mk(1, c.dim)
        self.resid2 = mk(1, c.dim)
        self.normed = mk(1, c.dim)
        self.qkv = mk(1, (h + 2 * kh) * hd)
        self.attn = mk(h, hd)
        self.attn_out = mk(1, c.dim)
        self.gu = mk(1, 2 * c.ffn_dim)
        self.act = mk(1, c.ffn_dim)
        self.mlp_out = mk(1, c.dim)
        self.logits = mk(1, c.vocab_size)
        self.tok_long = torch.empty(1, dtype=torch.long, device=dev)
        # fp8 decode scratch: rowwise-quantized activation + scale
        kmax = max(c.dim, h * hd, c.ffn_dim)
        self.x8 = torch.empty(1, kmax, dtype=torch.uint8, device=dev)
        self.xs = torch.empty(1, dtype=torch.float32, device=dev)


# fp8 fused-decode variant (A/B-measured, profiles/r02_measurements.md):
# default = quant_norm trio (one 1-block quant_norm + plain fp8 GEMVs) —
# best under the production 3-opponent concurrency (0.816 critiques/s vs
# 0.744 for the LDS trio). ADVSPEC_FP8_LDS=1 switches to the LDS-staged
# single-launch trio, which wins SOLO decode (3.51 vs 3.70 ms/tok): the
# per-block redundant staging work is free on an idle chip but costs
# shared VALU/L2 when co-resident opponents saturate the device.
_FP8_LDS = os.environ.get("ADVSPEC_FP8_LDS") == "1"


class LlamaModel:
    """Decoder-only transformer (RMSNorm / RoPE / GQA / SwiGLU)."""

    def __init__(self, config: LlamaConfig, device="cpu",
                 dtype: Optional[torch.dtype] = None, seed: int = 0,
                 tp=None) -> None:
        # tp: Optional[parallel.tp.TPContext] — head-sharded tensor
        # parallelism; self.config becomes the per-rank LOCAL config while
        # full_config keeps the replicated dims (embed/norm/lm_head).
        self.full_config = config
        self.tp = tp
        if tp is not None and tp.size > 1:
            from ..parallel.tp import shard_config

            config = shard_config(config, tp.size)
        self.config = config
        self.device = torch.device(device)
        if dtype is None:
            dtype = torch.bfloat16 if self.device.type == "cuda" else torch.float32
        self.dtype = dtype
        self.seed = seed
        c = config
        self.scale = 1.0 / math.sqrt(c.head_dim)
        # +8 slack: the multi-step decode graph may overshoot max_new by
        # up to _SPG-1 harmless steps whose RoPE reads land past the
        # nominal window (tokens discarded, but the table read must stay
        # in bounds)
        self.cos, self.sin = torch_ref.rope_tables(
            c.head_dim, c.max_seq_len + 8, c.rope_theta, self.device
        )
        self.embed: Optional[torch.Tensor] = None  # [vocab, d]
        self.final_norm: Optional[torch.Tensor] = None  # [d]
        self.lm_head: Optional[torch.Tensor] = None  # [vocab, d]
        self.layers: list[LayerWeights] = []
        self.fp8 = False  # set by quantize_fp8()
        # storage format of the caches new_cache() hands out; independent
        # of the weight dtype (the engine sets it from its spec)
        self.kv_dtype = "bf16"
        # decode-attention split-grid block target; 0 = kernel default
        # (256). The engine sets this from its live-opponent count before
        # capturing decode graphs: solo decode wants ~512 blocks of
        # self-occupancy, co-resident opponents share the chip and want
        # 256 (bf16) / 512 (fp8) — all A/B-measured (profiles).
        self.split_blocks = 0
        self.layers_q: list = []  # per-layer QuantW mirrors when fp8
        self.lm_head_q = None

    # -- weight initialisation ---------------------------------------------

    def init_random(self) -> "LlamaModel":
        """Deterministic random-init weights (synthetic/bench opponents).

        BASELINE.json mandates random-init opponent weights for the
        benchmark (no network for checkpoints); std is scaled so logits
        stay finite through deep stacks.

        Under TP every rank generates the FULL weights from the shared seed
        and keeps its shard, so TP=N is numerically identical to TP=1.
        """
        c = self.full_config
        g = torch.Generator(device="cpu").manual_seed(self.seed)

        def t(*shape, std=0.02):
            # generate in fp32 on CPU for cross-device determinism of tests;
            # large GPU models generate directly on device for speed.
            if self.device.type == "cuda":
                gd = torch.Generator(device=self.device)
                gd.manual_seed(self.seed + sum(shape) + len(self.layers) * 7919)
                x = torch.randn(*shape, generator=gd, device=self.device,
                                dtype=torch.float32)
            else:
                x = torch.randn(*shape, generator=g, dtype=torch.float32)
            return (x * std).to(self.dtype).to(self.device)

        d, hd = c.dim, c.head_dim
        proj_std = 0.02 / math.sqrt(2 * c.n_layers)
        self.embed = t(c.vocab_size, d)
        self.final_norm = torch.ones(d, device=self.device, dtype=self.dtype)
        self.lm_head = t(c.vocab_size, d)
        tp = self.tp
        self.layers = []
        for _ in range(c.n_layers):
            wqkv = t((c.n_heads + 2 * c.n_kv_heads) * hd, d)
            wo = t(d, c.n_heads * hd, std=proj_std)
            w_gate_up = t(2 * c.ffn_dim, d)
            w_down = t(d, c.ffn_dim, std=proj_std)
            if tp is not None and tp.size > 1:
                from ..parallel.tp import (
                    shard_down,
                    shard_gate_up,
                    shard_o,
                    shard_qkv,
                )

                wqkv = shard_qkv(wqkv, c, tp.size, tp.rank)
                wo = shard_o(wo, c, tp.size, tp.rank)
                w_gate_up = shard_gate_up(w_gate_up, c, tp.size, tp.rank)
                w_down = shard_down(w_down, c, tp.size, tp.rank)
            self.layers.append(
                LayerWeights(
                    attn_norm=torch.ones(d, device=self.device, dtype=self.dtype),
                    wqkv=wqkv,
                    wo=wo,
                    mlp_norm=torch.ones(d, device=self.device, dtype=self.dtype),
                    w_gate_up=w_gate_up,
                    w_down=w_down,
                )
            )
        return self

    def load_safetensors(self, path: str) -> "LlamaModel":
        """Load HF-format Llama weights from a local safetensors dir.

        Fuses q/k/v and gate/up (keeping HF's [out, in] row-major layout)
        and permutes q/k rows from HF's half-split RoPE layout to the
        interleaved-pair convention the RoPE kernel uses.
        """
        import glob as _glob
        import json as _json
        import os as _os

        from safetensors import safe_open

        c = self.config
        files = sorted(_glob.glob(_os.path.join(path, "*.safetensors")))
        if not files:
            raise FileNotFoundError(f"No safetensors files under {path}")
        tensors: dict[str, torch.Tensor] = {}
        want_prefixes = ("model.", "lm_head.")
        for f in files:
            with safe_open(f, framework="pt", device="cpu") as sf:
                for key in sf.keys():
                    if key.startswith(want_prefixes):
                        tensors[key] = sf.get_tensor(key)

        def perm_rope_rows(w: torch.Tensor, n_heads: int) -> torch.Tensor:
            # HF stores [rot_half] order; convert rows to interleaved pairs.
            hd = c.head_dim
            w = w.reshape(n_heads, hd, -1)
            half = hd // 2
            idx = torch.empty(hd, dtype=torch.long)
            idx[0::2] = torch.arange(0, half)
            idx[1::2] = torch.arange(half, hd)
            return w[:, idx, :].reshape(n_heads * hd, -1)

        def g(key: str) -> torch.Tensor:
            return tensors[key].to(torch.float32)

        # HF checkpoints store projections [out, in] — exactly our wire
        # layout, so no transposes: only q/k row permutation for the
        # interleaved-pair RoPE convention and the qkv / gate-up fusions.
        self.embed = g("model.embed_tokens.weight").to(self.dtype).to(self.device)
        self.final_norm = g("model.norm.weight").to(self.dtype).to(self.device)
        lm = tensors.get("lm_head.weight")
        if lm is None:  # tied embeddings
            lm = tensors["model.embed_tokens.weight"]
        self.lm_head = lm.to(torch.float32).contiguous().to(self.dtype).to(self.device)
        self.layers = []
        for i in range(c.n_layers):
            p = f"model.layers.{i}."
            wq = perm_rope_rows(g(p + "self_attn.q_proj.weight"), c.n_heads)
            wk = perm_rope_rows(g(p + "self_attn.k_proj.weight"), c.n_kv_heads)
            wv = g(p + "self_attn.v_proj.weight")
            wqkv = torch.cat([wq, wk, wv], dim=0).contiguous()
            w_gate_up = torch.cat(
                [g(p + "mlp.gate_proj.weight"), g(p + "mlp.up_proj.weight")], dim=0
            ).contiguous()
            self.layers.append(
                LayerWeights(
                    attn_norm=g(p + "input_layernorm.weight").to(self.dtype).to(self.device),
                    wqkv=wqkv.to(self.dtype).to(self.device),
                    wo=g(p + "self_attn.o_proj.weight").contiguous().to(self.dtype).to(self.device),
                    mlp_norm=g(p + "post_attention_layernorm.weight").to(self.dtype).to(self.device),
                    w_gate_up=w_gate_up.to(self.dtype).to(self.device),
                    w_down=g(p + "mlp.down_proj.weight").contiguous().to(self.dtype).to(self.device),
                )
            )
        return self

    # fp8 default = UNIFORM: under multi-opponent concurrency decode is
    # HBM-bound, so total BYTES win — uniform fp8 (8 GB/8B model) measured
    # 0.714 critiques/s vs 0.670 for a mixed scheme that kept the small
    # latency-bound projections bf16 (solo-kernel ALU numbers do not
    # transfer to the bandwidth-shared regime).
    FP8_PROJECTIONS = ("wqkv", "wo", "w_gate_up", "w_down")

    def quantize_fp8(self, projections=None, lm_head: bool = True) -> "LlamaModel":
        """Switch projection weights to rowwise OCP e4m3 (BASELINE config
        5: fp8 MFMA prefill + halved decode weight streaming). Norms,
        embeddings and the attention path stay bf16; scales factor out of
        every dot product, so dequantization is exact in the kernel
        epilogue. `projections=("wqkv","wo","w_gate_up","w_down")` forces
        uniform fp8."""
        if projections is None:
            projections = self.FP8_PROJECTIONS
        self.layers_q = []
        for L in self.layers:
            q = {}
            for f in projections:
                qt, sc = ops.quantize_fp8_rowwise(getattr(L, f))
                q[f] = QuantW(qt.to(self.device), sc.to(self.device))
                setattr(L, f, None)  # free the bf16 copy
            self.layers_q.append(q)
        if lm_head:
            qt, sc = ops.quantize_fp8_rowwise(self.lm_head)
            self.lm_head_q = QuantW(qt.to(self.device), sc.to(self.device))
            self.lm_head = None
        self.fp8 = True
        return self

    # -- inference ----------------------------------------------------------

    def new_cache(self, max_seq: Optional[int] = None,
                  kv_dtype: Optional[str] = None) -> PagedKVCache:
        """kv_dtype "bf16" (default: elements in the model dtype) or "fp8"
        (rowwise e4m3fn, opt-in); None takes the model's `kv_dtype`."""
        return PagedKVCache(
            self.config, max_seq or self.config.max_seq_len, self.device,
            self.dtype, kv_dtype=kv_dtype or self.kv_dtype,
        )

    def _forward(self, tokens: torch.Tensor, cache: PagedKVCache, pos0: int,
                 pos_state: Optional[torch.Tensor] = None,
                 max_seq_bound: int = 0) -> torch.Tensor:
        """Run t tokens at positions pos0..pos0+t-1; return last-token logits.

        Graph mode (t==1, GPU): pos_state is a device int32[1] holding the
        position — rope/kv_write/attention read it in-kernel so one captured
        HIP graph replays for every decode token; max_seq_bound sizes the
        attention split geometry once for the whole generation.
        """
        c = self.config
        t = tokens.shape[0]
        h, kh, hd = c.n_heads, c.n_kv_heads, c.head_dim
        resid = self.embed[tokens]  # [t, d]

        # batch-1 decode projections stream weights through the hand-written
        # GEMV kernel; prefill (t>1) uses the in-tree tiled MFMA GEMM; fp8
        # mode routes every projection through the e4m3 MFMA kernel.
        mm = ops.gemv if t == 1 else ops.gemm
        fp8 = self.fp8

        def proj(x, L_, Qd, name):
            qw = Qd.get(name) if Qd is not None else None
            if qw is not None:
                if t == 1 and x.is_cuda:
                    # batch-1 decode: the weight-streaming fp8 GEMV, not
                    # the tiled GEMM (eager 70B decode measured 10x slow
                    # through the M=1 GEMM path)
                    out = torch.empty(1, qw.q.shape[0], device=x.device,
                                      dtype=x.dtype)
                    x8 = torch.empty(1, x.shape[-1], dtype=torch.uint8,
                                     device=x.device)
                    xs = torch.empty(1, dtype=torch.float32, device=x.device)
                    return ops.gemv_fp8(x, qw.q, qw.s, x8, xs, out)
                return ops.gemm_fp8(x, qw.q, qw.s)
            return mm(x, getattr(L_, name))

        normed = ops.rmsnorm(resid, self.layers[0].attn_norm, c.norm_eps)
        for i, L in enumerate(self.layers):
            Qd = self.layers_q[i] if fp8 else None
            qkv = proj(normed, L, Qd, "wqkv")  # [t, (h+2kh)*hd]
            q = qkv[:, : h * hd].view(t, h, hd)
            k = qkv[:, h * hd : (h + kh) * hd].view(t, kh, hd)
            v = qkv[:, (h + kh) * hd :].view(t, kh, hd)
            kv8 = cache.kv_dtype == "fp8"
            if kv8:
                q, k = ops.rope_kv_fp8(
                    q, k, v, self.cos, self.sin, cache.k[i], cache.v[i],
                    cache.k_scale[i], cache.v_scale[i], cache.page_table,
                    pos0, pos_state=pos_state)
            else:
                q, k = ops.rope_kv(q, k, v, self.cos, self.sin, cache.k[i],
                                   cache.v[i], cache.page_table, pos0,
                                   pos_state=pos_state)
            if t > 1:
                if pos0 == 0:
                    # (fp8 cache too: single-shot prefill attends over the
                    # fresh unquantized K/V; only the cache copy is fp8)
                    attn = ops.attn_prefill(q, k, v, self.scale, causal=True,
                                            window=c.sliding_window)
                elif kv8:
                    # chunked prefill over an fp8 cache: the prefix (this
                    # chunk's own rows included) is read back dequantized,
                    # so the result is NOT bit-equal to single-shot
                    # prefill, which never sees quantized K/V.
                    k_all, v_all = ops.kv_dequant_fp8(
                        cache.k[i], cache.v[i], cache.k_scale[i],
                        cache.v_scale[i], cache.page_table, pos0 + t,
                        dtype=q.dtype)
                    attn = ops.attn_prefill(q, k_all, v_all, self.scale,
                                            causal=True, kv_offset=pos0,
                                            window=c.sliding_window)
                else:
                    # chunked prefill: this chunk's queries attend to ALL
                    # cached positions plus themselves. The page table is
                    # identity (PagedKVCache allocates one pool), so the
                    # cache view [0 : pos0+t] IS contiguous [seq, kh, hd] —
                    # the same flash prefill kernel runs with kv_offset.
                    kh_ = k.shape[1]
                    k_all = cache.k[i].view(-1, kh_, hd)[: pos0 + t]
                    v_all = cache.v[i].view(-1, kh_, hd)[: pos0 + t]
                    attn = ops.attn_prefill(q, k_all, v_all, self.scale,
                                            causal=True, kv_offset=pos0,
                                            window=c.sliding_window)
            else:
                seq = max_seq_bound if pos_state is not None else pos0 + 1
                if kv8:
                    attn = ops.attn_decode_paged_fp8(
                        q[0], cache.k[i], cache.v[i], cache.k_scale[i],
                        cache.v_scale[i], cache.page_table, seq, self.scale,
                        pos_state=pos_state, identity=cache.identity,
                        split_blocks=self.split_blocks,
                        window=c.sliding_window,
                    ).unsqueeze(0)
                else:
                    attn = ops.attn_decode_paged(
                        q[0], cache.k[i], cache.v[i], cache.page_table, seq,
                        self.scale, pos_state=pos_state,
                        identity=cache.identity,
                        split_blocks=self.split_blocks,
                        window=c.sliding_window,
                    ).unsqueeze(0)
            attn_out = proj(attn.reshape(t, h * hd), L, Qd, "wo")
            if self.tp is not None and self.tp.size > 1:
                self.tp.all_reduce_(attn_out)  # row-parallel wo partial sums
            resid, normed = ops.add_rmsnorm(resid, attn_out, L.mlp_norm, c.norm_eps)
            if t == 1 and Qd is None:
                # decode: fused gate_up GEMV + SwiGLU (one launch)
                act = torch.empty(1, c.ffn_dim, device=normed.device,
                                  dtype=normed.dtype)
                ops.gemv_gateup(normed, L.w_gate_up, act)
            else:
                gu = proj(normed, L, Qd, "w_gate_up")
                act = ops.swiglu(gu[:, : c.ffn_dim], gu[:, c.ffn_dim :])
            mlp_out = proj(act, L, Qd, "w_down")
            if self.tp is not None and self.tp.size > 1:
                self.tp.all_reduce_(mlp_out)  # row-parallel down partial sums
            next_norm = (
                self.layers[i + 1].attn_norm if i + 1 < c.n_layers else self.final_norm
            )
            resid, normed = ops.add_rmsnorm(resid, mlp_out, next_norm, c.norm_eps)
        if self.lm_head_q is not None:
            logits = ops.gemm_fp8(normed[-1:].contiguous(), self.lm_head_q.q,
                                  self.lm_head_q.s)
        else:
            logits = ops.gemv(normed[-1:].contiguous(), self.lm_head)  # [1, vocab]
        return logits[0]

    def prefill(self, tokens: torch.Tensor, cache: PagedKVCache,
                chunk: Optional[int] = None) -> torch.Tensor:
        """Prefill the prompt; returns last-position logits [vocab].

        `chunk` caps the tokens processed per forward pass: 32k single-shot
        prefill fits comfortably in 288 GB HBM3E, so chunking is an
        ACTIVATION-memory valve for longer documents, not
        the default. Chunk boundaries re-run attention against the cached
        prefix (kv_offset), numerically identical to single-shot — with a
        bf16 cache. An fp8 cache hands later chunks the DEQUANTIZED prefix,
        so chunked prefill then agrees with single-shot only to
        quantization noise, not bitwise."""
        n = tokens.shape[0]
        if n > cache.max_seq:
            raise ValueError(f"prompt {n} exceeds cache {cache.max_seq}")
        if chunk is None or n <= chunk:
            logits = self._forward(tokens, cache, 0)
            cache.seq_len = n
            return logits
        pos = 0
        logits = None
        while pos < n:
            step = min(chunk, n - pos)
            logits = self._forward(tokens[pos : pos + step], cache, pos)
            pos += step
            cache.seq_len = pos
        return logits

    def decode_one(self, token, cache: PagedKVCache) -> torch.Tensor:
        """Append one token; returns next-token logits [vocab].

        `token` may be a Python int or a device scalar tensor (the async
        decode loop feeds the sampled id back without a host round-trip).
        """
        if isinstance(token, torch.Tensor):
            tok = token.reshape(1).to(torch.long)
        else:
            tok = torch.tensor([token], device=self.device, dtype=torch.long)
        logits = self._forward(tok, cache, cache.seq_len)
        cache.seq_len += 1
        return logits

    def new_decode_ws(self) -> DecodeWorkspace:
        return DecodeWorkspace(self)

    def decode_step_ws(self, cache: PagedKVCache, pos_state: torch.Tensor,
                       max_seq_bound: int, W: DecodeWorkspace) -> torch.Tensor:
        """Allocation-free single-token decode: token id in W.tok_long,
        logits written into W.logits. Safe to capture in a HIP graph (all
        dynamic state in device words, zero allocator traffic)."""
        # GPU-only: the CPU op wrappers ignore out= (they return fresh
        # tensors), which would silently drop every write into W.
        assert self.device.type == "cuda", "decode_step_ws is GPU-only"
        c = self.config
        h, kh, hd = c.n_heads, c.n_kv_heads, c.head_dim
        fp8 = self.fp8

        def proj(x, L_, Qd, name, out):
            qw = Qd.get(name) if Qd is not None else None
            if qw is not None:
                ops.gemv_fp8(x, qw.q, qw.s, W.x8, W.xs, out.view(1, -1))
                return out
            return ops.gemv(x, getattr(L_, name), out=out)

        # norm/residual GEMV fusion (non-TP): the rmsnorm folds into the
        # consuming GEMV's prologue (bf16: LDS-staged x*wln; fp8: fused
        # quant_norm producing x8/xs) and the residual add into the
        # producing GEMV's epilogue — 65 (bf16) / ~128 (fp8, incl. the
        # separate quantize launches) fewer launches per step (the decode
        # anatomy's add_rmsnorm x2 row was pure launch-bound small
        # kernels). TP keeps the unfused sequence: the all-reduce must see
        # the raw partial projection before the add.
        fused = self.tp is None or self.tp.size == 1
        # the fp8 fused path needs every projection + lm_head quantized
        # (mixed schemes from quantize_fp8(projections=...) fall back)
        fused_f8 = (
            fused and fp8 and self.lm_head_q is not None
            and all(
                q.get(f) is not None for q in self.layers_q
                for f in self.FP8_PROJECTIONS
            )
        )

        fused_bf = fused and not fp8

        torch.index_select(self.embed, 0, W.tok_long, out=W.resid)
        if not (fused_bf or fused_f8):
            ops.rmsnorm(W.resid, self.layers[0].attn_norm, c.norm_eps,
                        out=W.normed)
        # RoPE + KV append ride in the qkv GEMV's epilogue (one launch, no
        # qkv round trip) wherever the w32 row geometry holds; the
        # ADVSPEC_FP8_LDS path, TP and odd shapes keep the rope_kv launch
        # (every layer's cache is a slice of one tensor: layer 0 speaks for all)
        fuse_rope = ops.qkv_rope_fusable(h, kh, hd, self.cos, self.sin,
                                         cache.k[0], cache.v[0])
        # an fp8 cache never fuses (qkv_rope_fusable refuses a non-bf16
        # cache: the per-row amax spans 16 blocks of the w32 GEMV and cannot
        # ride its epilogue): unfused qkv GEMV, then rope_kv_fp8.
        kv8 = cache.kv_dtype == "fp8"
        for i, L in enumerate(self.layers):
            Qd = self.layers_q[i] if fp8 else None
            roped = False
            if fused_f8:
                qw = Qd.get("wqkv")
                if _FP8_LDS:
                    ops.gemv_fp8_norm(W.resid, L.attn_norm, qw.q, qw.s,
                                      c.norm_eps, W.qkv)
                else:
                    ops.quant_norm_fp8(W.resid, L.attn_norm, W.x8, W.xs,
                                       c.norm_eps)
                    if fuse_rope:
                        ops.gemv_fp8_q_rope_kv(
                            W.x8, W.xs, qw.q, qw.s, W.qkv, self.cos, self.sin,
                            cache.k[i], cache.v[i], cache.page_table, 0, h,
                            kh, pos_state=pos_state)
                        roped = True
                    else:
                        ops.gemv_fp8_q(W.x8, W.xs, qw.q, qw.s, W.qkv)
            elif fused_bf:
                if fuse_rope:
                    ops.gemv_norm_rope_kv(
                        W.resid, L.attn_norm, L.wqkv, c.norm_eps, self.cos,
                        self.sin, cache.k[i], cache.v[i], cache.page_table, 0,
                        h, kh, pos_state=pos_state, out=W.qkv)
                    roped = True
                else:
                    ops.gemv_norm(W.resid, L.attn_norm, L.wqkv, c.norm_eps,
                                  out=W.qkv)
            else:
                proj(W.normed, L, Qd, "wqkv", W.qkv)
            q = W.qkv[:, : h * hd].view(1, h, hd)
            if not roped:
                k = W.qkv[:, h * hd : (h + kh) * hd].view(1, kh, hd)
                v = W.qkv[:, (h + kh) * hd :].view(1, kh, hd)
                if kv8:
                    ops.rope_kv_fp8(q, k, v, self.cos, self.sin, cache.k[i],
                                    cache.v[i], cache.k_scale[i],
                                    cache.v_scale[i], cache.page_table, 0,
                                    pos_state=pos_state)
                else:
                    ops.rope_kv(q, k, v, self.cos, self.sin, cache.k[i],
                                cache.v[i], cache.page_table, 0,
                                pos_state=pos_state)
            if kv8:
                ops.attn_decode_paged_fp8(
                    q[0], cache.k[i], cache.v[i], cache.k_scale[i],
                    cache.v_scale[i], cache.page_table, max_seq_bound,
                    self.scale, pos_state=pos_state, out=W.attn,
                    identity=cache.identity, split_blocks=self.split_blocks,
                    window=c.sliding_window,
                )
            else:
                ops.attn_decode_paged(
                    q[0], cache.k[i], cache.v[i], cache.page_table,
                    max_seq_bound, self.scale, pos_state=pos_state,
                    out=W.attn, identity=cache.identity,
                    split_blocks=self.split_blocks,
                    window=c.sliding_window,
                )
            if fused_f8:
                gw = Qd.get("w_gate_up")
                if _FP8_LDS:
                    ops.gemv_fp8_resl(W.attn.view(1, h * hd),
                                      Qd.get("wo").q, Qd.get("wo").s,
                                      W.resid)
                    ops.gemv_fp8_gateup_norm(W.resid, L.mlp_norm, gw.q,
                                             gw.s, c.norm_eps, W.act)
                    ops.gemv_fp8_resl(W.act, Qd.get("w_down").q,
                                      Qd.get("w_down").s, W.resid)
                else:
                    ops.gemv_fp8_res(W.attn.view(1, h * hd),
                                     Qd.get("wo").q, Qd.get("wo").s,
                                     W.x8, W.xs, W.resid)
                    ops.quant_norm_fp8(W.resid, L.mlp_norm, W.x8, W.xs,
                                       c.norm_eps)
                    ops.gemv_fp8_gateup(W.x8, W.xs, gw.q, gw.s, W.act)
                    ops.gemv_fp8_res(W.act, Qd.get("w_down").q,
                                     Qd.get("w_down").s, W.x8, W.xs,
                                     W.resid)
                continue
            if fused_bf:
                ops.gemv_res(W.attn.view(1, h * hd), L.wo, W.resid)
                ops.gemv_gateup_norm(W.resid, L.mlp_norm, L.w_gate_up,
                                     c.norm_eps, W.act)
                ops.gemv_res(W.act, L.w_down, W.resid)
                continue
            proj(W.attn.view(1, h * hd), L, Qd, "wo", W.attn_out)
            if self.tp is not None and self.tp.size > 1:
                self.tp.all_reduce_(W.attn_out)
            ops.add_rmsnorm(W.resid, W.attn_out, L.mlp_norm, c.norm_eps,
                            out_resid=W.resid2, out_y=W.normed)
            if Qd is None:
                # fused gate_up GEMV + SwiGLU: one launch, no gu round-trip
                ops.gemv_gateup(W.normed, L.w_gate_up, W.act)
            else:
                proj(W.normed, L, Qd, "w_gate_up", W.gu)
                ops.swiglu(W.gu[:, : c.ffn_dim], W.gu[:, c.ffn_dim :],
                           out=W.act)
            proj(W.act, L, Qd, "w_down", W.mlp_out)
            if self.tp is not None and self.tp.size > 1:
                self.tp.all_reduce_(W.mlp_out)
            nxt = (self.layers[i + 1].attn_norm if i + 1 < c.n_layers
                   else self.final_norm)
            ops.add_rmsnorm(W.resid2, W.mlp_out, nxt, c.norm_eps,
                            out_resid=W.resid, out_y=W.normed)
        if fused_f8:
            if _FP8_LDS:
                ops.gemv_fp8_norm(W.resid, self.final_norm,
                                  self.lm_head_q.q, self.lm_head_q.s,
                                  c.norm_eps, W.logits)
            else:
                ops.quant_norm_fp8(W.resid, self.final_norm, W.x8, W.xs,
                                   c.norm_eps)
                ops.gemv_fp8_q(W.x8, W.xs, self.lm_head_q.q,
                               self.lm_head_q.s, W.logits)
        elif fused_bf:
            ops.gemv_norm(W.resid, self.final_norm, self.lm_head, c.norm_eps,
                          out=W.logits)
        elif self.lm_head_q is not None:
            ops.gemv_fp8(W.normed, self.lm_head_q.q, self.lm_head_q.s,
                         W.x8, W.xs, W.logits)
        else:
            ops.gemv(W.normed, self.lm_head, out=W.logits)
        return W.logits

    def decode_one_graph(self, tok_slot: torch.Tensor, cache: PagedKVCache,
                         pos_state: torch.Tensor, max_seq_bound: int) -> torch.Tensor:
        """One graph-capturable decode step: position from pos_state, token
        from tok_slot (int32[1] on device). Does NOT advance cache.seq_len —
        the engine reconciles it after the replay loop."""
        tok = tok_slot.to(torch.long)
        return self._forward(tok, cache, 0, pos_state=pos_state,
                             max_seq_bound=max_seq_bound)
