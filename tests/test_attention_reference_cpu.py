"""CPU self-check of the float64 attention reference that judges the HIP
kernels in tests/test_attention_edges_gpu.py.

The reference is validated on its own before it judges a kernel: against
closed-form values, and against the project's fp32 oracle
(`torch_ref.attn_prefill`, `torch_ref.attn_decode_paged`) including
`kv_offset > 0` and `causal=False`.
"""

import importlib.util
import math
import os

import pytest
import torch

from adversarial_spec_amd.ops import torch_ref

_spec = importlib.util.spec_from_file_location(
    "_attention_edges",
    os.path.join(os.path.dirname(__file__), "test_attention_edges_gpu.py"))
edges = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(edges)

# fp32 oracle vs float64 reference on O(1) values averaged over <= a few
# hundred keys: fp32 eps 6e-8 times the sum lengths, with a wide margin.
F32_ATOL = 2e-5


def _bf_as_f32(*shape, gen):
    """bf16-rounded values held in fp32, so torch_ref returns fp32."""
    return torch.randn(*shape, generator=gen).to(torch.bfloat16).float()


class TestClosedForm:
    def test_single_key_returns_v(self):
        g = torch.Generator().manual_seed(1)
        q = torch.randn(1, 4, 32, generator=g)
        k = torch.randn(1, 2, 32, generator=g)
        v = torch.randn(1, 2, 32, generator=g)
        out = edges.ref_attention(q, k, v)
        assert out.dtype == torch.float64
        want = v.double().repeat_interleave(2, dim=1)
        assert torch.equal(out, want)

    @pytest.mark.parametrize("kv_offset", [0, 3])
    def test_equal_scores_average_the_visible_prefix(self, kv_offset):
        """k = 0 makes every score equal: row i is the mean of the values
        it may see, keys 0..kv_offset+i when causal, all keys otherwise."""
        g = torch.Generator().manual_seed(2)
        tq, hq, kh, hd = 5, 4, 2, 32
        tk = kv_offset + tq
        q = torch.randn(tq, hq, hd, generator=g)
        k = torch.zeros(tk, kh, hd)
        v = torch.randn(tk, kh, hd, generator=g)
        vd = v.double().repeat_interleave(hq // kh, dim=1)
        out = edges.ref_attention(q, k, v, kv_offset=kv_offset)
        for i in range(tq):
            want = vd[: kv_offset + i + 1].mean(dim=0)
            assert torch.allclose(out[i], want, atol=1e-14)
        out = edges.ref_attention(q, k, v, causal=False)
        assert torch.allclose(out, vd.mean(dim=0).expand(tq, -1, -1),
                              atol=1e-14)

    def test_two_keys_hand_softmax(self):
        hd = 32
        q = torch.zeros(1, 1, hd)
        q[0, 0, 0] = 2.0
        k = torch.zeros(2, 1, hd)
        k[1, 0, 0] = 3.0
        v = torch.zeros(2, 1, hd)
        v[0, 0, 0], v[1, 0, 1] = 1.0, 1.0
        out = edges.ref_attention(q, k, v, scale=0.5, causal=False)
        w1 = 1.0 / (1.0 + math.exp(-3.0))  # scores 0 and 2*3*0.5
        assert out[0, 0, 0].item() == pytest.approx(1.0 - w1, abs=1e-15)
        assert out[0, 0, 1].item() == pytest.approx(w1, abs=1e-15)

    def test_gqa_maps_consecutive_heads_to_one_kv_head(self):
        g = torch.Generator().manual_seed(3)
        q = torch.randn(2, 6, 32, generator=g)
        k = torch.randn(9, 2, 32, generator=g)
        v = torch.randn(9, 2, 32, generator=g)
        out = edges.ref_attention(q, k, v, kv_offset=7)
        for h in range(6):
            one = edges.ref_attention(q[:, h:h + 1], k[:, h // 3:h // 3 + 1],
                                      v[:, h // 3:h // 3 + 1], kv_offset=7)
            assert torch.allclose(out[:, h:h + 1], one, atol=1e-14)


class TestAgainstTorchRef:
    @pytest.mark.parametrize("tq,tk,kv_offset,causal", [
        (33, 33, 0, True),
        (7, 12, 5, True),
        (33, 97, 64, True),
        (1, 2, 1, True),
        (5, 77, 0, False),
        (70, 70, 0, False),
    ])
    @pytest.mark.parametrize("hd", [32, 128])
    def test_prefill(self, tq, tk, kv_offset, causal, hd):
        g = torch.Generator().manual_seed(tq * 1000 + tk + hd)
        q = _bf_as_f32(tq, 4, hd, gen=g)
        k = _bf_as_f32(tk, 2, hd, gen=g)
        v = _bf_as_f32(tk, 2, hd, gen=g)
        want = torch_ref.attn_prefill(q, k, v, None, causal, kv_offset)
        got = edges.ref_attention(q, k, v, None, causal, kv_offset)
        assert got.dtype == torch.float64 and got.shape == want.shape
        assert (got - want.double()).abs().max().item() <= F32_ATOL

    @pytest.mark.parametrize("seq_len", [1, 7, 65, 300])
    @pytest.mark.parametrize("page,group,hd", [(64, 4, 128), (16, 3, 32),
                                               (256, 1, 64)])
    def test_decode_paged(self, seq_len, page, group, hd):
        g = torch.Generator().manual_seed(seq_len * 1000 + page + hd)
        kh = 2
        npg = (seq_len + page - 1) // page + 2
        q = _bf_as_f32(kh * group, hd, gen=g)
        kc = _bf_as_f32(npg, page, kh, hd, gen=g)
        vc = _bf_as_f32(npg, page, kh, hd, gen=g)
        table = torch.randperm(npg, generator=g).to(torch.int32)
        want = torch_ref.attn_decode_paged(q, kc, vc, table, seq_len)
        got = edges.ref_decode(q, kc, vc, table, seq_len)
        assert got.dtype == torch.float64 and got.shape == want.shape
        assert (got - want.double()).abs().max().item() <= F32_ATOL


class TestCaseBuilders:
    """The GPU module's input builders, checked where no GPU is needed."""

    def test_nan_fill_covers_everything_past_seq_len(self):
        seq, page = 65, 64
        q, kc, vc, table = edges._decode_inputs(seq, 32, 2, nan_fill=True,
                                                cover=1024)
        n_used = 1024 // page
        for c in (kc, vc):
            logical = c[table[:n_used].long()].reshape(n_used * page, -1)
            assert torch.isfinite(logical[:seq]).all()
            assert torch.isnan(logical[seq:]).all()
            reached = set(table[:n_used].tolist())
            for p in set(range(c.shape[0])) - reached:
                assert torch.isnan(c[p]).all()
        assert torch.isfinite(edges.ref_decode(q, kc, vc, table, seq)).all()

    def test_tiles_per_split(self):
        assert edges._tiles(300, 2, 192) == [3, 2]
        assert edges._tiles(700, 2, 384) == [6, 5]
        assert edges._tiles(101, 2, 512) == [2, 0]
        assert edges._tiles(65, 16, 64) == [1, 1] + [0] * 14

    @pytest.mark.parametrize("c,want", [
        (3.0, ["defer", "defer", "rescale", "defer"]),
        (7.5, ["defer", "rescale", "defer", "rescale"]),
        (9.0, ["rescale"] * 4),
    ])
    def test_ramp_takes_the_intended_softmax_branches(self, c, want):
        q, k, _ = edges._ramp_inputs(c)
        trace = [t for t in edges._defer_trace(q, k) if t[1] > 0]
        assert not [t for t in trace if t[3] == "edge"]
        assert [t[3] for t in trace if t[0] == 304] == want
