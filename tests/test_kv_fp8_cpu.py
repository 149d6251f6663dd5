"""fp8 (e4m3fn) KV cache on the CPU reference path: the quantizer contract,
the cache object, a tiny model running on it, and the switches that select
it (engine spec, ADVSPEC_KV_DTYPE, `debate.py local alias --kv-dtype`).

Quantizer contract (ops/torch_ref.py): one scale per (position, kv-head)
row, scale = max(amax|x|, 1e-12) / 448 in fp32, q = e4m3fn round-to-nearest
of x / scale. The test bound is the half-step of the e4m3 grid at the
quantized magnitude, which any round-to-nearest meets whatever its tie rule
and which truncation, a wrong exponent bias or the fnuz encoding miss.
"""

import json

import pytest
import torch
from kv_fp8_common import assert_half_step

from adversarial_spec_amd import ops, providers
from adversarial_spec_amd.cli import debate
from adversarial_spec_amd.engine.local import (
    LocalEngine, clear_engines, get_engine, resolve_kv_dtype)
from adversarial_spec_amd.models import LlamaModel, get_config
from adversarial_spec_amd.models.llama import PagedKVCache
from adversarial_spec_amd.ops import torch_ref


class TestQuantizerContract:
    @pytest.mark.parametrize("hd", [32, 64, 128])
    def test_half_step_bound(self, hd):
        g = torch.Generator().manual_seed(hd)
        x = torch.randn(97, 2, hd, generator=g)
        # spread the rows over many binades, and put exact ties and values
        # near every edge of the grid into one row
        x = x * torch.logspace(-6, 4, 97).view(-1, 1, 1)
        x[0, 0, :8] = torch.tensor([448., 416., 432., 0.001, 2. ** -9,
                                    1.5 * 2. ** -9, -448., 17.])
        x = x.to(torch.bfloat16)
        q8, s = torch_ref.quantize_kv_fp8(x)
        assert q8.dtype == torch.uint8 and q8.shape == x.shape
        assert s.dtype == torch.float32 and s.shape == x.shape[:-1]
        want = x.float().abs().amax(-1).clamp_min(1e-12) / 448.0
        assert torch.equal(s, want)
        assert_half_step(x.float(), q8, s, f"quantize hd={hd}")
        assert torch.equal(torch_ref.dequantize_kv_fp8(q8, s),
                           q8.view(torch.float8_e4m3fn).float()
                           * s.unsqueeze(-1))

    def test_bound_rejects_wrong_quantizers(self):
        """The bound is not vacuous: truncation and the fnuz encoding (bias
        8: every byte decodes to half its e4m3fn value) both miss it."""
        x = torch.randn(64, 2, 64, generator=torch.Generator().manual_seed(1))
        q8, s = torch_ref.quantize_kv_fp8(x)
        y = (x / s.unsqueeze(-1))
        trunc = torch.where(
            y.abs() < q8.view(torch.float8_e4m3fn).float().abs(),
            (q8.to(torch.int16) - 1).clamp_min(0).to(torch.uint8), q8)
        with pytest.raises(AssertionError):
            assert_half_step(x, trunc, s, "truncation")
        with pytest.raises(AssertionError):
            assert_half_step(x, q8, s / 2, "fnuz bias")

    def test_zero_row(self):
        x = torch.zeros(3, 2, 32)
        q8, s = torch_ref.quantize_kv_fp8(x)
        assert int(q8.to(torch.int32).abs().sum()) == 0
        assert torch.isfinite(s).all() and (s > 0).all()
        assert torch.equal(torch_ref.dequantize_kv_fp8(q8, s), x)

    def test_write_gather_roundtrip_through_page_table(self):
        """kv_write_fp8 + kv_dequant_fp8 across a permuted table equal the
        quantizer applied to the rows, and decode attention over the cache
        equals fp32 attention over the dequantized rows."""
        page, kh, hd, npg, n = 16, 2, 32, 6, 70
        g = torch.Generator().manual_seed(3)
        table = torch.randperm(npg, generator=g).to(torch.int32)
        k = torch.randn(n, kh, hd, generator=g)
        v = torch.randn(n, kh, hd, generator=g)
        kc = torch.full((npg, page, kh, hd), 0x7F, dtype=torch.uint8)
        vc = kc.clone()
        ks = torch.full((npg, kh, page), float("nan"))
        vs = ks.clone()
        torch_ref.kv_write_fp8(kc, vc, ks, vs, table, 0, k[:5], v[:5])
        torch_ref.kv_write_fp8(kc, vc, ks, vs, table, 5, k[5:], v[5:])
        kd, vd = ops.kv_dequant_fp8(kc, vc, ks, vs, table, n,
                                    dtype=torch.float32)
        assert torch.equal(kd, torch_ref.dequantize_kv_fp8(
            *torch_ref.quantize_kv_fp8(k)))
        assert torch.equal(vd, torch_ref.dequantize_kv_fp8(
            *torch_ref.quantize_kv_fp8(v)))
        q = torch.randn(4, hd, generator=g)
        got = ops.attn_decode_paged_fp8(q, kc, vc, ks, vs, table, n)
        want = torch_ref.attn_prefill(q.unsqueeze(0), kd, vd, causal=False)[0]
        assert torch.isfinite(got).all()
        assert torch.allclose(got, want, atol=1e-5)


class TestCacheObject:
    def test_fp8_cache_layout(self):
        cfg = get_config("tiny")
        c = PagedKVCache(cfg, 100, "cpu", torch.float32, page_size=32,
                         kv_dtype="fp8")
        npg = 4
        kh, hd, nl = cfg.n_kv_heads, cfg.head_dim, cfg.n_layers
        assert c.kv_dtype == "fp8"
        for t in (c.k, c.v):
            assert t.dtype == torch.uint8 and t.element_size() == 1
            assert t.shape == (nl, npg, 32, kh, hd)
        for t in (c.k_scale, c.v_scale):
            assert t.dtype == torch.float32
            assert t.shape == (nl, npg, kh, 32)
        assert c.identity and c.max_seq == 128

    def test_default_cache_unchanged(self):
        cfg = get_config("tiny")
        m = LlamaModel(cfg, device="cpu", seed=1)
        c = m.new_cache(300)
        kh, hd, nl = cfg.n_kv_heads, cfg.head_dim, cfg.n_layers
        assert c.kv_dtype == "bf16"
        assert c.k.dtype == m.dtype and c.v.dtype == m.dtype
        assert c.k.shape == c.v.shape == (nl, 2, 256, kh, hd)
        assert c.identity is True and c.max_seq == 512 and c.seq_len == 0
        assert torch.equal(c.page_table, torch.arange(2, dtype=torch.int32))
        assert c.k_scale is None and c.v_scale is None
        assert m.new_cache(64, kv_dtype="fp8").k.dtype == torch.uint8

    def test_bad_kv_dtype_raises(self):
        with pytest.raises(ValueError):
            PagedKVCache(get_config("tiny"), 64, "cpu", torch.float32,
                         kv_dtype="int4")


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(
        a.float().unsqueeze(0), b.float().unsqueeze(0)).item()


class TestTinyModelFp8KV:
    def setup_method(self):
        self.cfg = get_config("tiny")
        self.model = LlamaModel(self.cfg, device="cpu", seed=5).init_random()

    def test_prefill_then_decode_finite(self):
        cache = self.model.new_cache(256, kv_dtype="fp8")
        logits = self.model.prefill(torch.arange(2, 40), cache)
        assert logits.shape == (self.cfg.vocab_size,)
        assert torch.isfinite(logits).all()
        assert int(cache.k[:, 0, :38].to(torch.int32).sum()) > 0
        assert (cache.k_scale[:, 0, :, :38] > 0).all()
        for tok in (7, 8, 9):
            logits = self.model.decode_one(tok, cache)
            assert torch.isfinite(logits).all()
        assert cache.seq_len == 41
        # the fp8 cache changes the logits only by quantization noise
        ref_cache = self.model.new_cache(256)
        self.model.prefill(torch.arange(2, 40), ref_cache)
        for tok in (7, 8, 9):
            ref = self.model.decode_one(tok, ref_cache)
        assert _cos(ref, logits) > 0.995

    def test_chunked_prefill_agrees_with_single_shot(self):
        """The bf16 chunked test of test_engine_cpu.py is bitwise-level
        (allclose atol=1e-4); with an fp8 cache later chunks read the
        DEQUANTIZED prefix while single-shot prefill never sees quantized
        K/V, so the two are no longer bit-equal. The agreement level is the
        cosine bound of test_decode_matches_prefill_gpu (> 0.995)."""
        toks = torch.arange(2, 120)  # 118 tokens
        c1 = self.model.new_cache(256, kv_dtype="fp8")
        ref = self.model.prefill(toks, c1)
        c2 = self.model.new_cache(256, kv_dtype="fp8")
        got = self.model.prefill(toks, c2, chunk=48)  # 48 + 48 + 22
        assert c2.seq_len == 118
        assert torch.isfinite(got).all()
        cos = _cos(ref, got)
        print(f"fp8-KV chunked vs single-shot cosine {cos:.6f}")
        assert cos > 0.995, f"chunked/single cosine {cos}"
        assert ref.argmax() == got.argmax()


class TestSwitches:
    def setup_method(self):
        clear_engines()

    def teardown_method(self):
        clear_engines()

    def test_spec_key_reaches_cache(self, monkeypatch):
        monkeypatch.delenv("ADVSPEC_KV_DTYPE", raising=False)
        eng = LocalEngine({"name": "k8", "arch": "tiny", "kv_dtype": "fp8"},
                          device="cpu")
        assert eng.kv_dtype == "fp8" and not eng.model.fp8
        cache = eng._get_cache(100)
        assert cache.kv_dtype == "fp8" and cache.k.dtype == torch.uint8
        text, in_tok, out_tok, _ = eng.generate(
            "s", "u", max_tokens=6, temperature=0.0, timeout=30)
        assert in_tok > 0 and 0 <= out_tok <= 6
        assert eng._cache.kv_dtype == "fp8"

    def test_kv_dtype_independent_of_weight_dtype(self, monkeypatch):
        monkeypatch.delenv("ADVSPEC_KV_DTYPE", raising=False)
        eng = LocalEngine({"name": "w8", "arch": "tiny", "dtype": "fp8"},
                          device="cpu")
        assert eng.model.fp8 and eng._get_cache(10).kv_dtype == "bf16"
        eng = LocalEngine({"name": "w8k8", "arch": "tiny", "dtype": "fp8",
                           "kv_dtype": "fp8"}, device="cpu")
        assert eng.model.fp8 and eng._get_cache(10).kv_dtype == "fp8"

    def test_env_fallback(self, monkeypatch):
        monkeypatch.delenv("ADVSPEC_KV_DTYPE", raising=False)
        assert resolve_kv_dtype({"arch": "tiny"}) == "bf16"
        assert LocalEngine({"name": "d", "arch": "tiny"},
                           device="cpu")._get_cache(10).kv_dtype == "bf16"
        monkeypatch.setenv("ADVSPEC_KV_DTYPE", "fp8")
        assert resolve_kv_dtype({"arch": "tiny"}) == "fp8"
        eng = LocalEngine({"name": "e", "arch": "tiny"}, device="cpu")
        assert eng._get_cache(10).kv_dtype == "fp8"
        # the spec key wins over the environment
        eng = LocalEngine({"name": "f", "arch": "tiny", "kv_dtype": "bf16"},
                          device="cpu")
        assert eng._get_cache(10).kv_dtype == "bf16"
        # and the engine cache keeps the two apart
        a = get_engine({"name": "c", "arch": "tiny"}, device="cpu")
        monkeypatch.delenv("ADVSPEC_KV_DTYPE")
        b = get_engine({"name": "c", "arch": "tiny"}, device="cpu")
        assert a is not b and (a.kv_dtype, b.kv_dtype) == ("fp8", "bf16")

    def test_bad_values_raise(self, monkeypatch):
        monkeypatch.delenv("ADVSPEC_KV_DTYPE", raising=False)
        with pytest.raises(ValueError):
            LocalEngine({"name": "x", "arch": "tiny", "kv_dtype": "fp4"},
                        device="cpu")
        monkeypatch.setenv("ADVSPEC_KV_DTYPE", "e5m2")
        with pytest.raises(ValueError):
            LocalEngine({"name": "y", "arch": "tiny"}, device="cpu")

    def test_cli_flag_stored_in_registry(self, tmp_path, monkeypatch):
        monkeypatch.setattr(providers, "GLOBAL_CONFIG_PATH",
                            tmp_path / "config.json")
        monkeypatch.delenv("ADVSPEC_KV_DTYPE", raising=False)
        args = debate.create_parser().parse_args(
            ["local", "alias", "mine", "tiny", "--kv-dtype", "fp8",
             "--model-dtype", "bf16"])
        assert args.kv_dtype == "fp8"
        assert debate.handle_utility_command(args) == 0
        stored = json.loads((tmp_path / "config.json").read_text())
        alias = stored["local"]["custom_aliases"]["mine"]
        assert alias["kv_dtype"] == "fp8" and alias["dtype"] == "bf16"
        spec = providers.resolve_local_model("mine", stored["local"])
        assert spec["kv_dtype"] == "fp8"
        assert LocalEngine(spec, device="cpu")._get_cache(10).kv_dtype == "fp8"
        with pytest.raises(SystemExit):
            debate.create_parser().parse_args(
                ["local", "alias", "m2", "tiny", "--kv-dtype", "int8"])
        # without the flag the registry entry carries no kv_dtype key
        args = debate.create_parser().parse_args(["local", "alias", "m3",
                                                  "tiny"])
        assert debate.handle_utility_command(args) == 0
        stored = json.loads((tmp_path / "config.json").read_text())
        assert "kv_dtype" not in stored["local"]["custom_aliases"]["m3"]
