"""qkv GEMV with the RoPE + KV-append epilogue vs the two-kernel sequence.

`ops.gemv_norm_rope_kv` (bf16) and `ops.gemv_fp8_q_rope_kv` (fp8) promise
the bits of `ops.gemv_norm` / `ops.gemv_fp8_q` followed by `ops.rope_kv`:
the projection is rounded to bf16 before the rotation, the rotation uses the
same fp32 expressions and table rows. So every comparison here is
`torch.equal`, on the projected row AND on the whole K and V caches, which
start from random contents: the right cache row was written and nothing
else moved.

Shapes (K, hq, kh, hd): (2560, 4, 2, 128) runs one pass of the 8-deep
weight loop plus a tail, (1536, 4, 4, 64) the tail only, (512, 2, 1, 32) a
single tail step. Positions, page = 16 with 4 pages: 0, 15 (last slot of a
page), 16 (first slot of the next), 63 (last slot of the last page).
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from adversarial_spec_amd import ops
    from adversarial_spec_amd.ops import torch_ref
else:  # collected but deselected on CPU
    ops = torch_ref = None

DEV = "cuda:0"
EPS = 1e-5
PAGE = 16
N_PAGES = 4
SHAPES = [(2560, 4, 2, 128), (1536, 4, 4, 64), (512, 2, 1, 32)]
POSITIONS = [0, 15, 16, PAGE * N_PAGES - 1]


def _bf(x):
    return x.to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _inputs(K, hq, kh, hd):
    """Device inputs for one shape, built once, never written: the tests
    clone the caches they hand to an op."""
    gen = torch.Generator().manual_seed(K * 1009 + hq * 101 + kh * 11 + hd)
    N = (hq + 2 * kh) * hd
    d = dict(
        x=_bf(torch.randn(1, K, generator=gen)),
        wln=_bf(1.0 + 0.1 * torch.randn(K, generator=gen)),
        w=_bf(torch.randn(N, K, generator=gen) * K ** -0.5),
        kc=_bf(torch.randn(N_PAGES, PAGE, kh, hd, generator=gen)),
        vc=_bf(torch.randn(N_PAGES, PAGE, kh, hd, generator=gen)),
        ident=torch.arange(N_PAGES, dtype=torch.int32),
        perm=torch.tensor([2, 0, 3, 1], dtype=torch.int32),
    )
    d = {k: v.to(DEV) for k, v in d.items()}
    d["cos"], d["sin"] = torch_ref.rope_tables(hd, PAGE * N_PAGES, 10000.0,
                                               DEV)
    return d


def _views(y, hq, kh, hd):
    q = y[:, : hq * hd].view(1, hq, hd)
    k = y[:, hq * hd : (hq + kh) * hd].view(1, kh, hd)
    v = y[:, (hq + kh) * hd :].view(1, kh, hd)
    return q, k, v


def _pos_args(pos, source):
    """(pos0, pos_state) for the op: a host scalar, or a device word with a
    wrong scalar beside it (graph mode must ignore the scalar)."""
    if source == "scalar":
        return pos, None
    return 0, torch.tensor([pos], dtype=torch.int32, device=DEV)


def _two_kernel_bf16(d, table, hq, kh, hd, pos0, pos_state):
    kc, vc = d["kc"].clone(), d["vc"].clone()
    y = ops.gemv_norm(d["x"], d["wln"], d["w"], EPS)
    q, k, v = _views(y, hq, kh, hd)
    ops.rope_kv(q, k, v, d["cos"], d["sin"], kc, vc, table, pos0,
                pos_state=pos_state)
    return y, kc, vc


def _assert_same(got, want, what):
    for name, g, w in zip(("y", "k_cache", "v_cache"), got, want):
        assert g.shape == w.shape, f"{what}: {name} shape"
        n_diff = int((g.view(torch.int16) != w.view(torch.int16)).sum())
        print(f"{what}: {name} differing elements {n_diff}/{g.numel()}")
        assert torch.equal(g, w), f"{what}: {name} differs in {n_diff} elements"


@pytest.mark.parametrize("source", ["scalar", "pos_state"])
@pytest.mark.parametrize("table", ["ident", "perm"])
@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("K,hq,kh,hd", SHAPES)
def test_bf16_equals_gemv_norm_then_rope_kv(K, hq, kh, hd, pos, table, source):
    d = _inputs(K, hq, kh, hd)
    pos0, pos_state = _pos_args(pos, source)
    want = _two_kernel_bf16(d, d[table], hq, kh, hd, pos0, pos_state)
    # the cache row of `pos` really changes in the reference
    assert not torch.equal(want[1], d["kc"]) and not torch.equal(want[2], d["vc"])

    kc, vc = d["kc"].clone(), d["vc"].clone()
    y = ops.gemv_norm_rope_kv(d["x"], d["wln"], d["w"], EPS, d["cos"],
                              d["sin"], kc, vc, d[table], pos0, hq, kh,
                              pos_state=pos_state)
    assert y.shape == (1, (hq + 2 * kh) * hd)
    _assert_same((y, kc, vc), want,
                 f"bf16 K={K} hd={hd} pos={pos} {table} {source}")


def test_rotation_roundings_over_two_million_pairs():
    """The rotation rounds to bf16 from fp32, so fusing the other product
    into the fma (`fma(od, c, ev*s)` for `fma(ev, s, od*c)`) moves about one
    result in 2^15. The cases above rotate some 10^4 values and would let
    that through; this one rotates 2 * 10^6 (N = 8192, the widest row the
    kernel takes, 300 activation rows) and still demands equality."""
    K, hq, kh, hd = 512, 48, 8, 128
    N = (hq + 2 * kh) * hd
    assert N == 8192 and ops.qkv_rope_fusable(hq, kh, hd)
    gen = torch.Generator().manual_seed(99)
    xs = _bf(torch.randn(300, 1, K, generator=gen)).to(DEV)
    wln = _bf(1.0 + 0.1 * torch.randn(K, generator=gen)).to(DEV)
    w = _bf(torch.randn(N, K, generator=gen) * K ** -0.5).to(DEV)
    kc = _bf(torch.randn(N_PAGES, PAGE, kh, hd, generator=gen)).to(DEV)
    vc = kc.clone()
    wkc, wvc = kc.clone(), vc.clone()
    cos, sin = torch_ref.rope_tables(hd, PAGE * N_PAGES, 10000.0, DEV)
    table = torch.tensor([2, 0, 3, 1], dtype=torch.int32, device=DEV)
    got = torch.empty(300, 1, N, dtype=torch.bfloat16, device=DEV)
    want = torch.empty_like(got)
    for i in range(300):
        pos = 1 + i % (PAGE * N_PAGES - 1)  # never 0: cos = 1, sin = 0
        ops.gemv_norm_rope_kv(xs[i], wln, w, EPS, cos, sin, kc, vc, table,
                              pos, hq, kh, out=got[i])
        ops.gemv_norm(xs[i], wln, w, EPS, out=want[i])
        q, k, v = _views(want[i], hq, kh, hd)
        ops.rope_kv(q, k, v, cos, sin, wkc, wvc, table, pos)
    _assert_same((got, kc, vc), (want, wkc, wvc), "2e6 rotated values")


def test_bf16_out_written_in_place():
    K, hq, kh, hd = SHAPES[0]
    d = _inputs(K, hq, kh, hd)
    want = _two_kernel_bf16(d, d["perm"], hq, kh, hd, 16, None)
    kc, vc = d["kc"].clone(), d["vc"].clone()
    out = torch.full((1, (hq + 2 * kh) * hd), 7.0, dtype=torch.bfloat16,
                     device=DEV)
    ret = ops.gemv_norm_rope_kv(d["x"], d["wln"], d["w"], EPS, d["cos"],
                                d["sin"], kc, vc, d["perm"], 16, hq, kh,
                                out=out)
    assert ret.data_ptr() == out.data_ptr()
    _assert_same((out, kc, vc), want, "bf16 out=")


def test_graph_replay_at_two_positions():
    """Captured once with pos_state, replayed at two successive positions
    that straddle a page boundary (15 -> 16): each replay equals eager."""
    K, hq, kh, hd = SHAPES[0]
    d = _inputs(K, hq, kh, hd)
    table = d["perm"]
    pos_state = torch.tensor([3], dtype=torch.int32, device=DEV)
    kc, vc = d["kc"].clone(), d["vc"].clone()
    y = torch.empty(1, (hq + 2 * kh) * hd, dtype=torch.bfloat16, device=DEV)

    def step():
        ops.gemv_norm_rope_kv(d["x"], d["wln"], d["w"], EPS, d["cos"],
                              d["sin"], kc, vc, table, 0, hq, kh,
                              pos_state=pos_state, out=y)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()

    # eager reference over the same sequence of appends: 3 (warm-up and
    # capture do not run the kernel twice: capture records only), 15, 16
    ekc, evc = d["kc"].clone(), d["vc"].clone()
    ey = torch.empty_like(y)
    for pos, replay in ((3, False), (15, True), (16, True)):
        ps = torch.tensor([pos], dtype=torch.int32, device=DEV)
        ops.gemv_norm_rope_kv(d["x"], d["wln"], d["w"], EPS, d["cos"],
                              d["sin"], ekc, evc, table, 0, hq, kh,
                              pos_state=ps, out=ey)
        if replay:
            pos_state.fill_(pos)
            graph.replay()
            torch.cuda.synchronize()
            _assert_same((y, kc, vc), (ey, ekc, evc), f"graph replay pos={pos}")
    # and the eager sequence itself is the two-kernel one at the last step
    want_y = _two_kernel_bf16(d, table, hq, kh, hd, 16, None)[0]
    assert torch.equal(ey, want_y)


@pytest.mark.parametrize("source", ["scalar", "pos_state"])
@pytest.mark.parametrize("table", ["ident", "perm"])
@pytest.mark.parametrize("pos", POSITIONS)
def test_fp8_equals_gemv_fp8_q_then_rope_kv(pos, table, source):
    K, hq, kh, hd = SHAPES[0]
    N = (hq + 2 * kh) * hd
    d = _inputs(K, hq, kh, hd)
    wq, wsc = ops.quantize_fp8_rowwise(d["w"])
    x8 = torch.empty(K, dtype=torch.uint8, device=DEV)
    xs = torch.empty(1, dtype=torch.float32, device=DEV)
    ops.quant_norm_fp8(d["x"], d["wln"], x8, xs, EPS)
    pos0, pos_state = _pos_args(pos, source)

    wkc, wvc = d["kc"].clone(), d["vc"].clone()
    wy = torch.empty(1, N, dtype=torch.bfloat16, device=DEV)
    ops.gemv_fp8_q(x8, xs, wq, wsc, wy)
    q, k, v = _views(wy, hq, kh, hd)
    ops.rope_kv(q, k, v, d["cos"], d["sin"], wkc, wvc, d[table], pos0,
                pos_state=pos_state)

    kc, vc = d["kc"].clone(), d["vc"].clone()
    y = torch.empty(1, N, dtype=torch.bfloat16, device=DEV)
    ops.gemv_fp8_q_rope_kv(x8, xs, wq, wsc, y, d["cos"], d["sin"], kc, vc,
                           d[table], pos0, hq, kh, pos_state=pos_state)
    _assert_same((y, kc, vc), (wy, wkc, wvc),
                 f"fp8 pos={pos} {table} {source}")


def test_rejects_shapes_outside_the_row_geometry():
    """hd % 16 != 0 has no whole rotation pair per wave and N > 8192 is not
    the w32 kernel's: both are errors, never a silent other path."""
    assert ops.qkv_rope_fusable(32, 8, 128)        # Llama-3-8B: N = 6144
    assert not ops.qkv_rope_fusable(2, 1, 24)
    assert not ops.qkv_rope_fusable(64, 8, 128)    # N = 10240
    K, hq, kh, hd = 256, 2, 1, 24
    N = (hq + 2 * kh) * hd
    x = torch.zeros(1, K, dtype=torch.bfloat16, device=DEV)
    wln = torch.ones(K, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(N, K, dtype=torch.bfloat16, device=DEV)
    kc = torch.zeros(N_PAGES, PAGE, kh, hd, dtype=torch.bfloat16, device=DEV)
    vc = torch.zeros_like(kc)
    cos, sin = torch_ref.rope_tables(hd, PAGE * N_PAGES, 10000.0, DEV)
    table = torch.arange(N_PAGES, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="hd % 16"):
        ops.gemv_norm_rope_kv(x, wln, w, EPS, cos, sin, kc, vc, table, 0,
                              hq, kh)
    # a scalar position past the tables is refused on the host
    K, hq, kh, hd = SHAPES[2]
    d = _inputs(K, hq, kh, hd)
    with pytest.raises(RuntimeError, match="pos inside"):
        ops.gemv_norm_rope_kv(d["x"], d["wln"], d["w"], EPS, d["cos"],
                              d["sin"], d["kc"].clone(), d["vc"].clone(),
                              d["ident"], PAGE * N_PAGES, hq, kh)


def _decode_logits(fp8, seed):
    """decode_step_ws on the 3-layer config of test_ops_gpu's fused decode
    tests, from a freshly prefilled cache; returns (logits, k caches)."""
    from adversarial_spec_amd.models import LlamaModel
    from adversarial_spec_amd.models.config import LlamaConfig

    cfg = LlamaConfig(
        name="fuse-rope", dim=512, n_layers=3, n_heads=4, n_kv_heads=2,
        ffn_dim=1024, vocab_size=1024, max_seq_len=512, rope_theta=10000.0,
    )
    m = LlamaModel(cfg, device=DEV, dtype=torch.bfloat16, seed=seed)
    m.init_random()
    if fp8:
        m.quantize_fp8()
    toks = torch.arange(1, 33, device=DEV)
    cache = m.new_cache(256)
    m.prefill(toks[:-1], cache)
    W = m.new_decode_ws()
    W.tok_long.fill_(int(toks[-1]))
    pos_state = torch.tensor([cache.seq_len], dtype=torch.int32, device=DEV)
    logits = m.decode_step_ws(cache, pos_state, 256, W).clone()
    return logits, [k.clone() for k in cache.k], [v.clone() for v in cache.v]


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_decode_step_equals_two_kernel_sequence(fp8, monkeypatch):
    calls = {"fused": 0, "composed": 0}
    real_bf, real_f8 = ops.gemv_norm_rope_kv, ops.gemv_fp8_q_rope_kv

    def count_bf(*a, **kw):
        calls["fused"] += 1
        return real_bf(*a, **kw)

    def count_f8(*a, **kw):
        calls["fused"] += 1
        return real_f8(*a, **kw)

    monkeypatch.setattr(ops, "gemv_norm_rope_kv", count_bf)
    monkeypatch.setattr(ops, "gemv_fp8_q_rope_kv", count_f8)
    fused = _decode_logits(fp8, seed=3)
    assert calls["fused"] == 3, "decode_step_ws did not take the fused op"

    def composed_bf(x, wln, w, eps, cos, sin, kc, vc, table, pos0, hq, kh,
                    pos_state=None, out=None):
        calls["composed"] += 1
        y = ops.gemv_norm(x, wln, w, eps, out=out)
        q, k, v = _views(y, hq, kh, y.numel() // (hq + 2 * kh))
        ops.rope_kv(q, k, v, cos, sin, kc, vc, table, pos0,
                    pos_state=pos_state)
        return y

    def composed_f8(x8, xs, wq, wsc, out, cos, sin, kc, vc, table, pos0, hq,
                    kh, pos_state=None):
        calls["composed"] += 1
        ops.gemv_fp8_q(x8, xs, wq, wsc, out)
        q, k, v = _views(out, hq, kh, out.numel() // (hq + 2 * kh))
        ops.rope_kv(q, k, v, cos, sin, kc, vc, table, pos0,
                    pos_state=pos_state)
        return out

    monkeypatch.setattr(ops, "gemv_norm_rope_kv", composed_bf)
    monkeypatch.setattr(ops, "gemv_fp8_q_rope_kv", composed_f8)
    two = _decode_logits(fp8, seed=3)
    assert calls["composed"] == 3

    assert torch.isfinite(fused[0].float()).all()
    assert torch.equal(fused[0], two[0]), (
        f"logits differ: max diff "
        f"{(fused[0].float() - two[0].float()).abs().max():.4g}")
    for a, b in zip(fused[1] + fused[2], two[1] + two[2]):
        assert torch.equal(a, b), "KV caches differ after the decode step"
