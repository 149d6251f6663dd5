"""Sliding-window attention on the CPU: the torch_ref oracle, the option's
way from the CLI through the alias to the engine's config, the tiny model,
and a self-check of everything tests/test_sliding_window_gpu.py judges the
kernels with (tests/sliding_window_common.py: the float64 reference, the
poisoned inputs, the end-to-end constants).

`window = W >= 1`: the query at absolute position i sees keys
max(0, i - W + 1) .. i, W keys including itself; 0 = off.
"""

import dataclasses
import json
import os
import sys

import pytest
import torch

from adversarial_spec_amd import ops, providers
from adversarial_spec_amd.cli import debate
from adversarial_spec_amd.engine.local import (LocalEngine,
                                               resolve_sliding_window)
from adversarial_spec_amd.models import LlamaModel, get_config
from adversarial_spec_amd.ops import torch_ref

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sliding_window_common as common  # noqa: E402

# fp32 oracle vs float64 reference on O(1) values averaged over <= a few
# hundred keys (tests/test_attention_reference_cpu.py)
F32_ATOL = 2e-5


def _f32(*ts):
    """bf16-rounded inputs held in fp32, so torch_ref returns fp32."""
    return tuple(t.float() for t in ts)


def _paged(rows, page=16):
    """Logical rows [n, kh, hd] -> (cache [n_pages, page, kh, hd], table)
    through a reversed page table."""
    n, kh, hd = rows.shape
    n_pages = (n + page - 1) // page
    table = torch.arange(n_pages - 1, -1, -1, dtype=torch.int32)
    cache = torch.zeros(n_pages, page, kh, hd)
    padded = torch.zeros(n_pages * page, kh, hd)
    padded[:n] = rows
    cache[table.long()] = padded.view(n_pages, page, kh, hd)
    return cache, table


class TestReferenceItself:
    """The shared float64 reference against the edge tests' one."""

    @pytest.mark.parametrize("kv_offset,tq", [(0, 40), (23, 17)])
    def test_windowless_equals_edges_reference(self, kv_offset, tq):
        q, k, v = common.prefill_inputs("plain", kv_offset + tq, 4, 2, 32)
        q = q[kv_offset:]
        a = common.ref_attention_w(q, k, v, kv_offset=kv_offset)
        b = common.edges.ref_attention(q, k, v, kv_offset=kv_offset)
        assert (a - b).abs().max() < 1e-12

    def test_window_one_returns_own_v(self):
        q, k, v = common.prefill_inputs("plain", 20, 4, 2, 32)
        out = common.ref_attention_w(q, k, v, window=1)
        assert torch.equal(out, v.double().repeat_interleave(2, dim=1))

    def test_window_counts_w_keys(self):
        """Equal scores: the output is the mean of exactly the W last V rows
        (fewer near the start)."""
        n, w = 12, 5
        q = torch.zeros(n, 2, 32)
        k = torch.zeros(n, 1, 32)
        v = torch.arange(n).float().view(n, 1, 1).expand(n, 1, 32)
        out = common.ref_attention_w(q, k, v, window=w)
        for i in range(n):
            want = sum(range(max(0, i - w + 1), i + 1)) / min(w, i + 1)
            assert abs(out[i, 0, 0].item() - want) < 1e-12, i


class TestTorchRefPrefill:
    @pytest.mark.parametrize("window", [1, 7, 16, 40])
    @pytest.mark.parametrize("kv_offset,tq", [(0, 40), (23, 17)])
    @pytest.mark.parametrize("kind", ["plain", "ramp"])
    def test_vs_brute_force(self, kind, kv_offset, tq, window):
        q, k, v = common.prefill_inputs(kind, kv_offset + tq, 4, 2, 32)
        q = q[kv_offset:]
        got = torch_ref.attn_prefill(*_f32(q, k, v), kv_offset=kv_offset,
                                     window=window)
        want = common.ref_attention_w(q, k, v, kv_offset=kv_offset,
                                   window=window)
        assert got.dtype == torch.float32
        err = (got.double() - want).abs().max().item()
        assert err < F32_ATOL * (1 if kind == "plain" else 4), err

    @pytest.mark.parametrize("window", [40, 41, 4096])
    def test_window_of_all_keys_is_exactly_windowless(self, window):
        q, k, v = _f32(*common.prefill_inputs("plain", 40, 4, 2, 32))
        assert torch.equal(torch_ref.attn_prefill(q, k, v, window=window),
                           torch_ref.attn_prefill(q, k, v))
        assert torch.equal(ops.attn_prefill(q, k, v, window=window),
                           ops.attn_prefill(q, k, v))

    def test_ramp_shows_a_missing_window(self):
        q, k, v = common.prefill_inputs("ramp", 320, 4, 2, 128)
        got = torch_ref.attn_prefill(*_f32(q, k, v))
        err = (got.double() - common.prefill_ref("ramp", 320, 4, 2, 128, 64))
        assert err.abs().max() > 1.0
        # one key too many, or one too few, is as visible
        for wrong in (63, 65):
            got = torch_ref.attn_prefill(*_f32(q, k, v), window=wrong)
            err = got.double() - common.prefill_ref("ramp", 320, 4, 2, 128, 64)
            assert err[64:].abs().max() > 0.25, wrong

    def test_non_causal_window_raises(self):
        q, k, v = _f32(*common.prefill_inputs("plain", 40, 4, 2, 32))
        with pytest.raises(ValueError):
            torch_ref.attn_prefill(q, k, v, causal=False, window=4)
        with pytest.raises(ValueError):
            ops.attn_prefill(q, k, v, causal=False, window=4)
        with pytest.raises(ValueError):
            torch_ref.attn_prefill(q, k, v, window=-1)
        # window=0 stays legal without a causal mask
        torch_ref.attn_prefill(q, k, v, causal=False, window=0)


class TestTorchRefDecode:
    @pytest.mark.parametrize("seq,window", [(50, 1), (50, 16), (50, 17),
                                            (50, 49), (50, 50), (50, 80)])
    def test_vs_brute_force(self, seq, window):
        q, k, v = common.prefill_inputs("plain", 64, 4, 2, 32)
        q1 = q[seq - 1]
        kc, table = _paged(k.float())
        vc, _ = _paged(v.float())
        got = ops.attn_decode_paged(q1.float(), kc, vc, table, seq,
                                    window=window)
        want = common.ref_decode_w(q1, k, v, seq, window)
        assert (got.double() - want).abs().max() < F32_ATOL
        if window >= seq:
            assert torch.equal(
                got, ops.attn_decode_paged(q1.float(), kc, vc, table, seq))

    @pytest.mark.parametrize("seq,window", [(50, 16), (37, 5)])
    def test_equals_full_decode_over_last_w_rows(self, seq, window):
        q, k, v = _f32(*common.prefill_inputs("plain", 64, 4, 2, 32))
        q1 = q[seq - 1]
        kc, table = _paged(k)
        vc, _ = _paged(v)
        windowed = torch_ref.attn_decode_paged(q1, kc, vc, table, seq,
                                               window=window)
        kc2, table2 = _paged(k[seq - window:seq])
        vc2, _ = _paged(v[seq - window:seq])
        full = torch_ref.attn_decode_paged(q1, kc2, vc2, table2, window)
        assert torch.equal(windowed, full)

    @pytest.mark.parametrize("seq,window", [(50, 1), (50, 16), (50, 80)])
    def test_fp8_vs_brute_force(self, seq, window):
        q, k, v = common.prefill_inputs("plain", 64, 4, 2, 32)
        q1 = q[seq - 1]
        parts = {}
        for name, rows in (("k", k), ("v", v)):
            cache, table = _paged(rows.float())
            c8, cs = torch_ref.quantize_kv_fp8(cache)
            parts[name] = (c8, cs.permute(0, 2, 1).contiguous())
            deq = torch_ref.dequantize_kv_fp8(c8, cs).double()
            parts[name + "_rows"] = deq[table.long()].reshape(-1, 2, 32)
        got = ops.attn_decode_paged_fp8(
            q1.float(), parts["k"][0], parts["v"][0], parts["k"][1],
            parts["v"][1], table, seq, window=window)
        want = common.ref_decode_w(q1, parts["k_rows"], parts["v_rows"], seq,
                                window)
        assert (got.double() - want).abs().max() < F32_ATOL

    @pytest.mark.parametrize("fp8", [False, True])
    def test_poisoned_case_builder(self, fp8):
        """The shared decode inputs: the oracle agrees with the
        reference through the page table, and dropping the window is off by
        the poison's size."""
        seq, window = 300, 65
        case = common.decode_case(seq, window, 128, 4, fp8=fp8)
        assert case["lo"] == seq - window
        assert torch.isfinite(case["k_rows"]).all()
        # (1e3 comes back from e4m3 within a rounding of the row scale)
        assert (case["v_rows"][:case["lo"]] > 0.9 * common.POISON_V).all()
        assert (case["v_rows"][seq:] > 0.9 * common.POISON_V).all()
        want = common.decode_ref(case, seq, window)
        assert want.abs().max() < 10
        q = case["q"].float()
        if fp8:
            run = lambda w: torch_ref.attn_decode_paged_fp8(
                q, case["kc"], case["vc"], case["ks"], case["vs"],
                case["table"], seq, window=w)
        else:
            run = lambda w: torch_ref.attn_decode_paged(
                q, case["kc"].float(), case["vc"].float(), case["table"],
                seq, window=w)
        assert (run(window).double() - want).abs().max() < 1e-4
        for wrong in (0, window + 1):
            assert (run(wrong).double() - want).abs().max() > 100, wrong

    def test_walked_tiles(self):
        # seq 300, W 236: lo = 64, two splits of 192 from position 64
        assert common.walked_tiles(300, 236, 2, 192) == [3, 1]
        # seq 1000, W 130: lo = 870, base 832, splits [832,960) [960,1000)
        assert common.walked_tiles(1000, 130, 2, 128) == [2, 1]
        assert common.walked_tiles(64, 130, 2, 128) == [1, 0]
        assert common.walked_tiles(300, 0, 2, 192) == [3, 2]


class TestResolveSlidingWindow:
    TINY = get_config("tiny")
    V01 = get_config("mistral-7b-v0.1")

    def _weights(self, tmp_path, config):
        d = tmp_path / "ckpt"
        d.mkdir()
        (d / "config.json").write_text(json.dumps(config))
        return str(d)

    def test_presets(self):
        base = get_config("mistral-7b")
        assert base.sliding_window == 0 and self.TINY.sliding_window == 0
        assert self.V01.sliding_window == 4096
        assert dataclasses.replace(
            self.V01, name="mistral-7b", sliding_window=0) == base
        assert providers.LOCAL_MODEL_MAP["mistral-7b-v0.1"] == "mistral-7b-v0.1"

    def test_precedence(self, tmp_path):
        w = self._weights(tmp_path, {"sliding_window": 1024, "x": 1})
        # preset alone
        assert resolve_sliding_window({}, self.TINY, None) == 0
        assert resolve_sliding_window({}, self.V01, None) == 4096
        # checkpoint config over the preset
        assert resolve_sliding_window({}, self.V01, w) == 1024
        # spec key over both, 0 included
        assert resolve_sliding_window({"sliding_window": 8}, self.V01, w) == 8
        assert resolve_sliding_window({"sliding_window": 0}, self.V01, w) == 0
        assert resolve_sliding_window({"sliding_window": 0}, self.V01,
                                      None) == 0

    def test_checkpoint_null_and_missing(self, tmp_path):
        null = self._weights(tmp_path, {"sliding_window": None})
        assert resolve_sliding_window({}, self.V01, null) == 0
        (tmp_path / "other").mkdir()
        nokey = tmp_path / "other"
        (nokey / "config.json").write_text(json.dumps({"hidden_size": 4096}))
        assert resolve_sliding_window({}, self.V01, str(nokey)) == 4096
        # a weights directory without config.json falls through to the preset
        (tmp_path / "bare").mkdir()
        assert resolve_sliding_window({}, self.V01,
                                      str(tmp_path / "bare")) == 4096

    @pytest.mark.parametrize("bad", [True, False, -1, 1.5, "64", 2**31])
    def test_rejections(self, tmp_path, bad):
        with pytest.raises(ValueError):
            resolve_sliding_window({"sliding_window": bad}, self.TINY, None)
        w = self._weights(tmp_path, {"sliding_window": bad})
        with pytest.raises(ValueError):
            resolve_sliding_window({}, self.TINY, w)
        with pytest.raises(ValueError):
            resolve_sliding_window(
                {}, dataclasses.replace(self.TINY, sliding_window=bad), None)

    def test_engine_applies_it(self):
        eng = LocalEngine({"name": "sw", "arch": "tiny",
                           "sliding_window": 96}, device="cpu")
        assert eng.config.sliding_window == 96
        assert eng.model.config.sliding_window == 96
        assert get_config("tiny").sliding_window == 0
        plain = LocalEngine({"name": "sw", "arch": "tiny"}, device="cpu")
        assert plain.model.config is get_config("tiny")
        with pytest.raises(ValueError):
            LocalEngine({"name": "sw", "arch": "tiny",
                         "sliding_window": True}, device="cpu")


class TestCli:
    def test_alias_round_trip(self, isolated_paths):
        args = debate.create_parser().parse_args(
            ["local", "alias", "m", "mistral-7b", "--sliding-window", "4096",
             "--kv-dtype", "fp8"])
        assert args.sliding_window == 4096
        assert debate.handle_utility_command(args) == 0
        stored = json.loads((isolated_paths / "config.json").read_text())
        alias = stored["local"]["custom_aliases"]["m"]
        assert alias["sliding_window"] == 4096 and alias["kv_dtype"] == "fp8"
        spec = providers.resolve_local_model("m", stored["local"])
        assert spec["sliding_window"] == 4096
        assert resolve_sliding_window(spec, get_config(spec["arch"]),
                                      None) == 4096
        # 0 is stored (it overrides a checkpoint's window); no flag, no key
        for name, extra in (("z", ["--sliding-window", "0"]), ("n", [])):
            args = debate.create_parser().parse_args(
                ["local", "alias", name, "tiny"] + extra)
            assert debate.handle_utility_command(args) == 0
        stored = json.loads((isolated_paths / "config.json").read_text())
        assert stored["local"]["custom_aliases"]["z"]["sliding_window"] == 0
        assert "sliding_window" not in stored["local"]["custom_aliases"]["n"]

    def test_alias_engine(self, isolated_paths):
        args = debate.create_parser().parse_args(
            ["local", "alias", "t", "tiny", "--sliding-window", "96"])
        assert debate.handle_utility_command(args) == 0
        stored = json.loads((isolated_paths / "config.json").read_text())
        spec = providers.resolve_local_model("t", stored["local"])
        assert LocalEngine(spec, device="cpu").model.config.sliding_window == 96

    @pytest.mark.parametrize("value", ["-1", "2.5", "abc", str(2**31)])
    def test_rejected_at_parse_time(self, value):
        with pytest.raises(SystemExit):
            debate.create_parser().parse_args(
                ["local", "alias", "x", "tiny", "--sliding-window", value])

    def test_handle_local_command_rejects(self, isolated_paths, capsys):
        for bad in (-1, True, 2**31):
            assert providers.handle_local_command(
                "alias", "x", "tiny", None, None, sliding_window=bad) == 1
        assert "sliding_window" in capsys.readouterr().err
        assert not (isolated_paths / "config.json").exists()


class TestTinyModel:
    """Fixes the seed, the lengths and the compared steps that the GPU
    end-to-end test reuses."""

    def test_prefill_plus_decode_equals_one_windowed_prefill(self):
        steps = common.e2e_cpu_logits(common.E2E_WINDOW)
        m = common.e2e_cpu_model(common.E2E_WINDOW)
        toks = common.e2e_tokens()
        for step in common.E2E_CHECK_STEPS + (common.E2E_STEPS,):
            n = common.E2E_PROMPT + step
            one = m.prefill(toks[:n], m.new_cache(256))
            assert torch.allclose(one, steps[step], atol=1e-4), step
        # chunked prefill: a chunk boundary inside and past the window
        n = common.E2E_PROMPT + common.E2E_STEPS
        chunked = m.prefill(toks[:n], m.new_cache(256), chunk=64)
        assert torch.allclose(chunked, steps[common.E2E_STEPS], atol=1e-4)

    def test_fp8_cache_decode_takes_the_window(self):
        a = common.e2e_cpu_logits(common.E2E_WINDOW, "fp8")
        b = common.e2e_cpu_logits(common.E2E_WINDOW)
        c = common.e2e_cpu_logits(0)
        step = common.E2E_STEPS
        assert (a[step] - b[step]).abs().max() < (a[step] - c[step]).abs().max() / 4

    def test_window_changes_the_logits_beyond_the_engine_tolerance(self):
        assert common.E2E_PROMPT < common.E2E_WINDOW < 128
        assert common.E2E_PROMPT + max(common.E2E_CHECK_STEPS) > 128
        win = common.e2e_cpu_logits(common.E2E_WINDOW)
        full = common.e2e_cpu_logits(0)
        # while every key is inside the window nothing changes
        inside = common.E2E_WINDOW - common.E2E_PROMPT
        assert torch.equal(win[:inside + 1], full[:inside + 1])
        for step in common.E2E_CHECK_STEPS:
            ok, cos = common.e2e_within(win[step], full[step])
            assert not ok and cos < 0.98, (step, cos)
        # and the compared rows are not near-ties, so that bf16 kernels can
        # be held to top-1 agreement with this model
        for step in (0,) + common.E2E_CHECK_STEPS:
            top = win[step].topk(2).values
            assert top[0] - top[1] > 0.1, (step, top)
