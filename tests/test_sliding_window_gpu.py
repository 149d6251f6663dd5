"""Sliding-window attention on the GPU: prefill (MFMA and simple kernels),
the bf16 and fp8 decode split kernels, the graph-mode entry and the tiny
model end to end, against a float64 reference.

`window = W >= 1`: the query at absolute position i sees keys
max(0, i - W + 1) .. i; 0 = off.

The reference (`ref_attention_w`, `ref_decode_w`) is a brute-force float64
mask over the same rounded inputs. It, the input builders (what they poison
and why) and the end-to-end constants live in tests/sliding_window_common.py
and are checked on the CPU by tests/test_sliding_window_cpu.py. Tolerances
and `_assert_within` are those of tests/test_attention_edges_gpu.py (decode
atol=rtol=2e-2, prefill atol=2.5e-2 / rtol=2e-2, zero elements out of bound).
"""

import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sliding_window_common import (  # noqa: E402
    DECODE_TOL, DEV, DTILE, E2E_CHECK_STEPS, E2E_PROMPT, E2E_STEPS,
    E2E_WINDOW, KH, PREFILL_TOL, _assert_within, _dev, _pos_state,
    decode_case, decode_ref, e2e_cpu_logits, e2e_cpu_model, e2e_logits,
    e2e_within, prefill_inputs, prefill_ref, walked_tiles)

from adversarial_spec_amd.models import LlamaModel  # noqa: E402
from adversarial_spec_amd.models.llama import LayerWeights  # noqa: E402

if torch.cuda.is_available():
    from adversarial_spec_amd import ops
    from adversarial_spec_amd.engine.local import LocalEngine
    from adversarial_spec_amd.ops import _advspec_hip as _hip
else:  # collected but deselected on CPU
    ops = _hip = LocalEngine = None


def run_decode(case, seq, window, **kw):
    q, kc, vc, table = _dev(case["q"], case["kc"], case["vc"], case["table"])
    if "ks" in case:
        ks, vs = _dev(case["ks"], case["vs"])
        return ops.attn_decode_paged_fp8(q, kc, vc, ks, vs, table, seq,
                                         window=window, **kw)
    return ops.attn_decode_paged(q, kc, vc, table, seq, window=window, **kw)


def _gpu_twin(mc):
    """The CPU model's weights on the GPU in bf16 (as test_engine_gpu.py)."""
    mg = LlamaModel(mc.config, device=DEV, dtype=torch.bfloat16, seed=mc.seed)
    mg.embed = mc.embed.to(torch.bfloat16).to(DEV)
    mg.final_norm = mc.final_norm.to(torch.bfloat16).to(DEV)
    mg.lm_head = mc.lm_head.to(torch.bfloat16).to(DEV)
    mg.layers = [
        LayerWeights(**{
            f: getattr(L, f).to(torch.bfloat16).to(DEV)
            for f in ("attn_norm", "wqkv", "wo", "mlp_norm", "w_gate_up",
                      "w_down")})
        for L in mc.layers]
    return mg


# ---------------------------------------------------------------------------
# prefill, MFMA kernel (hd=128)
# ---------------------------------------------------------------------------

MFMA = dict(hq=4, kh=2, hd=128)
KINDS = ["ramp", "plain"]


def _prefill(kind, n, shape, window, rows=None, kv_offset=0):
    q, k, v = _dev(*prefill_inputs(kind, n, **shape))
    if rows is not None:
        q = q[rows].contiguous()
    return ops.attn_prefill(q, k, v, kv_offset=kv_offset, window=window)


class TestPrefillMfma:
    # a window inside one tile, on a tile edge, one past it, spanning blocks
    @pytest.mark.parametrize("window", [1, 17, 64, 65, 200])
    @pytest.mark.parametrize("kind", KINDS)
    def test_vs_ref(self, kind, window):
        got = _prefill(kind, 320, MFMA, window)
        _assert_within(got, prefill_ref(kind, 320, 4, 2, 128, window),
                       **PREFILL_TOL, name=f"prefill mfma {kind} W={window}")

    def test_ramp_shows_a_missing_window(self):
        """The ramp does what the module docstring says: without the window
        the kernel is far outside tolerance of the windowed reference."""
        got = _prefill("ramp", 320, MFMA, 0).double().cpu()
        err = (got - prefill_ref("ramp", 320, 4, 2, 128, 64)).abs().max()
        assert err > 1.0, err

    @pytest.mark.parametrize("window", [320, 4096])
    @pytest.mark.parametrize("kind", KINDS)
    def test_window_covering_everything_is_bitwise_windowless(self, kind,
                                                              window):
        assert torch.equal(_prefill(kind, 320, MFMA, window),
                           _prefill(kind, 320, MFMA, 0))

    @pytest.mark.parametrize("kv_offset,tq", [(128, 192), (256, 64)])
    @pytest.mark.parametrize("kind", KINDS)
    def test_chunk_is_bitwise_single_shot(self, kind, kv_offset, tq):
        """A chunk that starts on a multiple of 128 walks the tiles the
        single-shot prefill walks for those rows."""
        window = 100
        single = _prefill(kind, 320, MFMA, window)
        _assert_within(single, prefill_ref(kind, 320, 4, 2, 128, window),
                       **PREFILL_TOL, name=f"prefill mfma {kind} single")
        assert kv_offset + tq == 320
        chunk = _prefill(kind, 320, MFMA, window,
                         rows=slice(kv_offset, 320), kv_offset=kv_offset)
        assert torch.equal(chunk, single[kv_offset:]), (
            f"max diff "
            f"{(chunk.float() - single[kv_offset:].float()).abs().max():.4g}")

    @pytest.mark.parametrize("kv_offset,tq", [(65, 130), (200, 33)])
    def test_unaligned_chunk_vs_ref(self, kv_offset, tq):
        window, n = 70, kv_offset + tq
        got = _prefill("ramp", n, MFMA, window, rows=slice(kv_offset, n),
                       kv_offset=kv_offset)
        want = prefill_ref("ramp", n, 4, 2, 128, window)[kv_offset:]
        _assert_within(got, want, **PREFILL_TOL,
                       name=f"prefill mfma off={kv_offset} tq={tq}")

    # 130 rows: the second block holds two rows
    @pytest.mark.parametrize("window", [2, 65, 129])
    @pytest.mark.parametrize("kind", KINDS)
    def test_ragged_last_block(self, kind, window):
        got = _prefill(kind, 130, MFMA, window)
        _assert_within(got, prefill_ref(kind, 130, 4, 2, 128, window),
                       **PREFILL_TOL,
                       name=f"prefill mfma ragged {kind} W={window}")


class TestPrefillSimple:
    @pytest.mark.parametrize("window", [1, 40, 150])
    @pytest.mark.parametrize("hd", [64, 32])
    @pytest.mark.parametrize("kind", KINDS)
    def test_vs_ref(self, kind, hd, window):
        shape = dict(hq=4, kh=2, hd=hd)
        got = _prefill(kind, 150, shape, window)
        _assert_within(got, prefill_ref(kind, 150, 4, 2, hd, window),
                       **PREFILL_TOL,
                       name=f"prefill simple {kind} hd={hd} W={window}")
        if window == 150:
            assert torch.equal(got, _prefill(kind, 150, shape, 0))

    def test_chunk_vs_ref(self):
        shape, window, off = dict(hq=4, kh=2, hd=64), 40, 77
        got = _prefill("ramp", 150, shape, window, rows=slice(off, 150),
                       kv_offset=off)
        _assert_within(got, prefill_ref("ramp", 150, 4, 2, 64, window)[off:],
                       **PREFILL_TOL, name="prefill simple chunk")


class TestPrefillRefused:
    @pytest.mark.parametrize("hd", [64, 128])
    def test_non_causal_window(self, hd):
        q, k, v = _dev(*prefill_inputs("plain", 150, 4, 2, hd))
        with pytest.raises(RuntimeError):
            ops.attn_prefill(q, k, v, causal=False, window=8)

    def test_negative_window(self):
        q, k, v = _dev(*prefill_inputs("plain", 150, 4, 2, 64))
        with pytest.raises(RuntimeError):
            ops.attn_prefill(q, k, v, window=-1)


# ---------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------

# lo = seq - W mid-tile, on a tile edge, and in another split than seq - 1
SEQ_WINDOW = [(300, 1), (300, 63), (300, 64), (300, 65), (300, 236),
              (1000, 130)]
SPLIT_BLOCKS = 4   # 2 splits over KH = 2 kv heads


def _check_geometry(seq, window, split_blocks, bound=None):
    """Geometry of a windowed decode launch through the launcher's own rule;
    returns the tiles each split walks at true length `seq`."""
    assert os.environ.get("ADVSPEC_SPLIT_BLOCKS") is None, (
        "ADVSPEC_SPLIT_BLOCKS overrides the block target of these tests")
    ns, sl = _hip.decode_split_geometry(bound or seq, KH, split_blocks, window)
    tiles = walked_tiles(seq, window, ns, sl)
    lo = max(0, seq - window) if window else 0
    assert sum(tiles) * DTILE >= seq - lo // DTILE * DTILE, (ns, sl, tiles)
    return ns, sl, tiles


class TestDecodeWindow:
    @pytest.mark.parametrize("seq,window", SEQ_WINDOW)
    @pytest.mark.parametrize("identity", [True, False], ids=["ident", "table"])
    @pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
    def test_group4(self, fp8, identity, seq, window):
        ns, sl, tiles = _check_geometry(seq, window, SPLIT_BLOCKS)
        if window in (130, 236):
            # two splits of two or more tiles each in the grid; the window's
            # first row and the newest row lie in different splits
            assert ns == 2 and sl // DTILE >= 2 and tiles[1] >= 1
            lo = seq - window
            assert (lo - lo // DTILE * DTILE) // sl != (
                seq - 1 - lo // DTILE * DTILE) // sl
        case = decode_case(seq, window, 128, 4, fp8=fp8, identity=identity)
        got = run_decode(case, seq, window, identity=identity,
                         split_blocks=SPLIT_BLOCKS)
        _assert_within(got, decode_ref(case, seq, window), **DECODE_TOL,
                       name=f"decode W={window} s={seq} fp8={fp8} "
                            f"ident={identity} tiles={tiles}")

    @pytest.mark.parametrize("hd,group", [(32, 1), (64, 8)])
    @pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
    def test_other_groups(self, fp8, hd, group):
        seq, window = 300, 236
        _check_geometry(seq, window, SPLIT_BLOCKS)
        case = decode_case(seq, window, hd, group, fp8=fp8)
        got = run_decode(case, seq, window, split_blocks=SPLIT_BLOCKS)
        _assert_within(got, decode_ref(case, seq, window), **DECODE_TOL,
                       name=f"decode W={window} hd={hd} g={group} fp8={fp8}")

    @pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
    def test_one_tile_per_split(self, fp8):
        """The default block target: every split walks one tile."""
        seq, window = 1000, 130
        ns, sl, tiles = _check_geometry(seq, window, 0)
        assert sl == DTILE and ns == 4 and tiles == [1, 1, 1, 0], (ns, sl,
                                                                   tiles)
        case = decode_case(seq, window, 128, 4, fp8=fp8)
        got = run_decode(case, seq, window)
        _assert_within(got, decode_ref(case, seq, window), **DECODE_TOL,
                       name=f"decode W={window} s={seq} fp8={fp8} default")

    @pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
    def test_poison_shows_a_missing_window(self, fp8):
        case = decode_case(300, 65, 128, 4, fp8=fp8)
        got = run_decode(case, 300, 0, split_blocks=SPLIT_BLOCKS)
        err = (got.double().cpu() - decode_ref(case, 300, 65)).abs().max()
        assert err > 100, err

    @pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
    def test_sequence_shorter_than_window(self, fp8):
        seq, window = 50, 130
        case = decode_case(seq, window, 128, 4, fp8=fp8)
        assert case["lo"] == 0
        got = run_decode(case, seq, window, split_blocks=SPLIT_BLOCKS)
        _assert_within(got, decode_ref(case, seq, window), **DECODE_TOL,
                       name=f"decode s={seq} < W={window} fp8={fp8}")

    @pytest.mark.parametrize("window", [300, 5000])
    @pytest.mark.parametrize("graph", [False, True], ids=["host", "pos_state"])
    @pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
    def test_window_of_the_bound_is_bitwise_windowless(self, fp8, graph,
                                                       window):
        bound = 300
        assert (_hip.decode_split_geometry(bound, KH, SPLIT_BLOCKS, window)
                == _hip.decode_split_geometry(bound, KH, SPLIT_BLOCKS))
        seq = 211 if graph else bound
        case = decode_case(seq, 0, 128, 4, fp8=fp8, cover=bound)
        kw = dict(split_blocks=SPLIT_BLOCKS)
        if graph:
            kw["pos_state"] = _pos_state(seq - 1)
        a = run_decode(case, bound, window, **kw)
        b = run_decode(case, bound, 0, **kw)
        assert torch.equal(a, b)
        _assert_within(a, decode_ref(case, seq, 0), **DECODE_TOL,
                       name=f"decode W={window} >= bound fp8={fp8}")

    def test_negative_window_refused(self):
        case = decode_case(300, 0, 128, 4)
        with pytest.raises(RuntimeError):
            run_decode(case, 300, -1)


class TestDecodeWindowGraphMode:
    BOUND, WINDOW = 2048, 130

    @pytest.mark.parametrize("identity", [True, False], ids=["ident", "table"])
    @pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
    def test_window_slides_under_one_geometry(self, fp8, identity):
        """The device position moves; the geometry is asked for once and is
        the one of min(bound, W + 63) positions, whatever the position."""
        bound, window = self.BOUND, self.WINDOW
        geo = _hip.decode_split_geometry(bound, KH, SPLIT_BLOCKS, window)
        assert geo == _hip.decode_split_geometry(
            min(bound, window + DTILE - 1), KH, SPLIT_BLOCKS)
        assert geo == (2, 128)
        for pos in (63, 64, 200, 1500):
            seq = pos + 1
            case = decode_case(seq, window, 128, 4, fp8=fp8,
                               identity=identity, cover=bound)
            tiles = walked_tiles(seq, window, *geo)
            assert sum(tiles) * DTILE >= seq - case["lo"] // DTILE * DTILE
            got = run_decode(case, bound, window, identity=identity,
                             split_blocks=SPLIT_BLOCKS,
                             pos_state=_pos_state(pos))
            _assert_within(got, decode_ref(case, seq, window), **DECODE_TOL,
                           name=f"decode graph W={window} pos={pos} "
                                f"fp8={fp8} ident={identity} tiles={tiles}")


# ---------------------------------------------------------------------------
# end to end: the tiny model behind a 96-token window
# ---------------------------------------------------------------------------

def _greedy_ids(eng, monkeypatch, user, n):
    captured = []
    orig = eng.tokenizer.decode

    def capture(ids):
        captured.append(list(ids))
        return orig(ids)

    monkeypatch.setattr(eng.tokenizer, "decode", capture)
    out = eng.generate("sys", user, max_tokens=n, temperature=0.0,
                       timeout=300)
    monkeypatch.setattr(eng.tokenizer, "decode", orig)
    return captured[-1], out[1]


def e2e_user_message(tokenizer):
    """A user message whose rendered chat prompt is E2E_PROMPT tokens."""
    base = len(tokenizer.render_chat("sys", ""))
    user = "w" * (E2E_PROMPT - base)
    assert len(tokenizer.render_chat("sys", user)) == E2E_PROMPT
    return user


class TestEndToEnd:
    @pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
    def test_graph_and_eager_token_ids(self, monkeypatch, kv_dtype):
        monkeypatch.delenv("ADVSPEC_KV_DTYPE", raising=False)
        eng = LocalEngine({"name": f"sw-{kv_dtype}", "arch": "tiny",
                           "kv_dtype": kv_dtype,
                           "sliding_window": E2E_WINDOW}, device=DEV)
        assert eng.model.config.sliding_window == E2E_WINDOW
        user = e2e_user_message(eng.tokenizer)
        monkeypatch.setenv("ADVSPEC_NO_GRAPH", "1")
        a, in_tok = _greedy_ids(eng, monkeypatch, user, E2E_STEPS)
        monkeypatch.delenv("ADVSPEC_NO_GRAPH")
        b, _ = _greedy_ids(eng, monkeypatch, user, E2E_STEPS)
        assert in_tok == E2E_PROMPT
        assert eng._graph_state is not None
        assert eng._cache.kv_dtype == kv_dtype
        # past the window and past the first 64-position tile boundary
        # behind it
        assert in_tok + len(a) > 128 > E2E_WINDOW, len(a)
        div = next((i for i, (p, q) in enumerate(zip(a, b)) if p != q), None)
        assert a == b, f"diverge at {div}: eager={a} graph={b}"

    def test_logits_vs_cpu_model(self):
        kv_dtype = "bf16"
        mc = e2e_cpu_model(E2E_WINDOW)
        want = e2e_cpu_logits(E2E_WINDOW, kv_dtype)
        full = e2e_cpu_logits(0, kv_dtype)
        got = e2e_logits(_gpu_twin(mc), kv_dtype)
        assert torch.isfinite(got).all()
        for step in (0,) + E2E_CHECK_STEPS:
            ok, cos = e2e_within(got[step], want[step])
            ok0, cos0 = e2e_within(got[step], full[step])
            print(f"{kv_dtype} step {step}: cosine with the windowed CPU "
                  f"model {cos:.6f}, with the windowless one {cos0:.6f}")
            assert ok, f"step {step}: cosine {cos}"
            if step:
                assert not ok0, f"step {step}: window=0 cosine {cos0}"
