"""CPU branch of the fused qkv + RoPE + KV-append wrappers: it composes the
`torch_ref` pieces the two-kernel sequence is made of, so it must equal
them exactly, for a host position and for a `pos_state` word."""

import pytest
import torch

from adversarial_spec_amd import ops
from adversarial_spec_amd.ops import torch_ref

EPS = 1e-5
PAGE, N_PAGES = 16, 4
K, HQ, KH, HD = 256, 4, 2, 32
N = (HQ + 2 * KH) * HD


def _bf(x):
    return x.to(torch.bfloat16)


@pytest.fixture(scope="module")
def data():
    gen = torch.Generator().manual_seed(11)
    cos, sin = torch_ref.rope_tables(HD, PAGE * N_PAGES, 10000.0, "cpu")
    return dict(
        x=_bf(torch.randn(1, K, generator=gen)),
        wln=_bf(1.0 + 0.1 * torch.randn(K, generator=gen)),
        w=_bf(torch.randn(N, K, generator=gen) * K ** -0.5),
        kc=_bf(torch.randn(N_PAGES, PAGE, KH, HD, generator=gen)),
        vc=_bf(torch.randn(N_PAGES, PAGE, KH, HD, generator=gen)),
        table=torch.tensor([2, 0, 3, 1], dtype=torch.int32),
        cos=cos, sin=sin,
    )


def _composed(y, d, pos):
    """torch_ref rope + kv_write on the q/k/v slices of the projected row."""
    kc, vc = d["kc"].clone(), d["vc"].clone()
    q = y[:, : HQ * HD].view(1, HQ, HD)
    k = y[:, HQ * HD : (HQ + KH) * HD].view(1, KH, HD)
    v = y[:, (HQ + KH) * HD :].view(1, KH, HD)
    q2, k2 = torch_ref.rope(q, k, d["cos"], d["sin"], pos)
    torch_ref.kv_write(kc, vc, d["table"], pos, k2, v)
    return torch.cat([q2.reshape(1, -1), k2.reshape(1, -1),
                      v.reshape(1, -1)], dim=1), kc, vc


def _pos_args(pos, source):
    if source == "scalar":
        return pos, None
    return 0, torch.tensor([pos], dtype=torch.int32)


def test_fusable_shapes():
    assert ops.qkv_rope_fusable(32, 8, 128)
    assert ops.qkv_rope_fusable(2, 1, 32)
    assert not ops.qkv_rope_fusable(2, 1, 24)     # hd % 16
    assert not ops.qkv_rope_fusable(64, 8, 128)   # N = 10240 > 8192


def test_fusable_looks_at_the_tensors_it_is_given(data):
    """What the binding would refuse keeps the call on the two-kernel path
    instead of raising inside the decode step."""
    d = data
    ok = (d["cos"], d["sin"], d["kc"], d["vc"])
    assert ops.qkv_rope_fusable(HQ, KH, HD, *ok)
    assert not ops.qkv_rope_fusable(HQ, KH, HD, d["cos"].double(), d["sin"],
                                    d["kc"], d["vc"])
    assert not ops.qkv_rope_fusable(HQ, KH, HD, d["cos"].t().contiguous().t(),
                                    d["sin"], d["kc"], d["vc"])
    assert not ops.qkv_rope_fusable(HQ, KH, HD, d["cos"][:, :8].contiguous(),
                                    d["sin"], d["kc"], d["vc"])
    assert not ops.qkv_rope_fusable(HQ, KH, HD, d["cos"], d["sin"],
                                    d["kc"].transpose(0, 1), d["vc"])
    assert not ops.qkv_rope_fusable(HQ, KH, HD, d["cos"], d["sin"],
                                    d["kc"].float(), d["vc"])
    assert not ops.qkv_rope_fusable(HQ, KH, HD, d["cos"], d["sin"], d["kc"],
                                    d["vc"][:2])


@pytest.mark.parametrize("source", ["scalar", "pos_state"])
@pytest.mark.parametrize("pos", [0, 15, 16, PAGE * N_PAGES - 1])
def test_bf16_wrapper_equals_composed_reference(data, pos, source):
    d = data
    want = _composed(ops.gemv_norm(d["x"], d["wln"], d["w"], EPS), d, pos)
    pos0, pos_state = _pos_args(pos, source)
    kc, vc = d["kc"].clone(), d["vc"].clone()
    out = torch.full((1, N), 7.0, dtype=torch.bfloat16)
    ret = ops.gemv_norm_rope_kv(d["x"], d["wln"], d["w"], EPS, d["cos"],
                                d["sin"], kc, vc, d["table"], pos0, HQ, KH,
                                pos_state=pos_state, out=out)
    assert ret is out
    for g, w in zip((out, kc, vc), want):
        assert torch.equal(g, w)
    assert not torch.equal(kc, d["kc"]) and not torch.equal(vc, d["vc"])
    fresh = ops.gemv_norm_rope_kv(d["x"], d["wln"], d["w"], EPS, d["cos"],
                                  d["sin"], d["kc"].clone(), d["vc"].clone(),
                                  d["table"], pos0, HQ, KH,
                                  pos_state=pos_state)
    assert fresh.shape == (1, N) and torch.equal(fresh, want[0])


@pytest.mark.parametrize("source", ["scalar", "pos_state"])
@pytest.mark.parametrize("pos", [0, 16, PAGE * N_PAGES - 1])
def test_fp8_wrapper_equals_composed_reference(data, pos, source):
    d = data
    wq, wsc = ops.quantize_fp8_rowwise(d["w"])
    x8 = torch.empty(K, dtype=torch.uint8)
    xs = torch.empty(1, dtype=torch.float32)
    ops.quant_norm_fp8(d["x"], d["wln"], x8, xs, EPS)
    y = torch.empty(1, N, dtype=torch.bfloat16)
    ops.gemv_fp8_q(x8, xs, wq, wsc, y)
    want = _composed(y, d, pos)
    pos0, pos_state = _pos_args(pos, source)
    kc, vc = d["kc"].clone(), d["vc"].clone()
    out = torch.empty(1, N, dtype=torch.bfloat16)
    ops.gemv_fp8_q_rope_kv(x8, xs, wq, wsc, out, d["cos"], d["sin"], kc, vc,
                           d["table"], pos0, HQ, KH, pos_state=pos_state)
    for g, w in zip((out, kc, vc), want):
        assert torch.equal(g, w)
