"""Top-p / top-k filtered sampling without a GPU: the float64 contract
(torch_ref.nucleus_keep), argument validation at the engine and CLI layers,
alias storage, and a CPU engine whose tokens stay inside the kept set."""

from __future__ import annotations

import json

import pytest
import torch

from nucleus_common import (descending_row, geometric_row, head_index,
                            mixed_sign_row, tie_row)

from adversarial_spec_amd import ops, providers
from adversarial_spec_amd.cli import debate
from adversarial_spec_amd.engine.backend import LocalBackend
from adversarial_spec_amd.engine.local import (LocalEngine, clear_engines,
                                               get_engine,
                                               resolve_sampling_filter)
from adversarial_spec_amd.ops import torch_ref

V = 1024


def _kept(row, t, top_p, top_k=0):
    return set(torch_ref.nucleus_keep(row, t, top_p, top_k).nonzero()
               .flatten().tolist())


def _heads(n, vocab=V):
    return {head_index(vocab, k) for k in range(n)}


class TestNucleusKeepContract:
    def test_geometric_row(self):
        row = geometric_row(V)
        p = torch.softmax(row.double(), -1)
        top = [float(p[head_index(V, k)]) for k in range(4)]
        assert [round(x, 2) for x in top] == [0.50, 0.25, 0.13, 0.06]
        assert _kept(row, 1.0, 0.9) == _heads(4)
        # G of the third token is p0 + p1 = 0.747, not < 0.5
        assert _kept(row, 1.0, 0.5) == _heads(2)
        assert _kept(row, 1.0, 1e-6) == _heads(1)
        assert _kept(row, 1.0, 1.0) == set(range(V))

    def test_boundary_is_strict(self):
        """G == top_p exactly is NOT kept: two equal-mass groups, p = 0.5
        each (exact in binary), top_p = 0.5."""
        row = torch.tensor([0.0, -1e4, -1e4, -1e4, 0.0, -1e4, -1e4, -1e4])
        row[4] = -0.0  # same group as +0.0
        assert _kept(row.bfloat16(), 1.0, 0.5) == {0, 4}
        row2 = torch.tensor([1.0, 1.0, 0.0] + [-1e4] * 5).bfloat16()
        g, c = torch_ref.nucleus_mass_above(row2, 1.0)
        assert float(g[0]) == 0.0 and int(c[2]) == 2
        assert _kept(row2, 1.0, float(g[2])) == {0, 1}
        assert _kept(row2, 1.0, float(g[2]) + 1e-9) == {0, 1, 2}

    def test_tie_group_kept_whole(self):
        row = tie_row(V)
        p = torch.softmax(row.double(), -1)
        assert abs(float(p[head_index(V, 0)]) - 0.1) < 1e-3
        assert _kept(row, 1.0, 0.45) == _heads(8)
        # C == 0 for every member of the top group: top_k cannot split it
        assert _kept(row, 1.0, 0.45, top_k=3) == _heads(8)
        assert _kept(row, 1.0, 1.0, top_k=3) == _heads(8)
        # the sorted-prefix rule of torch_ref.sample would stop inside it
        assert _kept(row, 1.0, 0.85) == _heads(12)

    def test_top_k_on_distinct_logits(self):
        row = descending_row(V)
        assert _kept(row, 1.0, 1.0, top_k=3) == _heads(3)
        assert _kept(row, 1.0, 1.0, top_k=1) == _heads(1)
        assert _kept(row, 1.0, 1.0, top_k=0) == set(range(V))

    def test_combination_is_intersection(self):
        row = geometric_row(V)
        for top_p, top_k in ((0.9, 2), (0.5, 3), (0.9, 40), (0.99, 5)):
            both = _kept(row, 1.0, top_p, top_k)
            assert both == _kept(row, 1.0, top_p) & _kept(row, 1.0, 1.0, top_k)
        assert _kept(row, 1.0, 0.9, 2) == _heads(2)
        assert _kept(row, 1.0, 0.5, 3) == _heads(2)

    def test_signed_zeros_are_one_group(self):
        row, t = mixed_sign_row(V)
        kept = _kept(row, t, 0.5)
        assert kept == _heads(2 + 4 + 16)
        zeros = (row.float() == 0.0).nonzero().flatten().tolist()
        assert len(zeros) == 16 and set(zeros) <= kept

    def test_temperature_sharpens(self):
        row = geometric_row(V)
        assert len(_kept(row, 0.25, 0.9)) < len(_kept(row, 1.0, 0.9))
        assert len(_kept(row, 4.0, 0.9)) > len(_kept(row, 1.0, 0.9))

    def test_greedy(self):
        row = geometric_row(V)
        g = torch.Generator().manual_seed(0)
        for t in (0.0, -1.0):
            assert torch_ref.sample_filtered(row, t, 0.3, 5, g) == head_index(V, 0)
            assert _kept(row, t, 0.3, 5) == _heads(1)
        ties = tie_row(V)
        assert torch_ref.sample_filtered(ties, 0.0, 0.9, 0, g) == min(_heads(8))


class TestReferenceSampler:
    def test_draws_stay_in_kept_set_and_cover_it(self):
        row = geometric_row(V)
        g = torch.Generator().manual_seed(3)
        seen = {torch_ref.sample_filtered(row, 1.0, 0.9, 0, g)
                for _ in range(400)}
        assert seen == _heads(4)
        seen = {ops.sample_filtered(row, 1.0, 1.0, top_k=2, generator=g)
                for _ in range(100)}
        assert seen == _heads(2)

    def test_ops_mask_on_cpu_is_the_reference(self):
        row = tie_row(V)
        assert torch.equal(ops.nucleus_mask(row, 1.0, 0.45, 3),
                           torch_ref.nucleus_keep(row, 1.0, 0.45, 3))

    def test_existing_sample_unchanged(self):
        """torch_ref.sample keeps its sorted-prefix rule."""
        logits = torch.tensor([10.0, 9.5, -5.0, -5.0])
        g = torch.Generator().manual_seed(0)
        for _ in range(20):
            assert torch_ref.sample(logits, 1.0, 0.9, g) in (0, 1)


BAD_TOP_P = (0, -0.1, 1.5)


class TestValidation:
    @pytest.mark.parametrize("top_p", BAD_TOP_P)
    def test_engine_spec_rejects_top_p(self, top_p):
        with pytest.raises(ValueError):
            LocalEngine({"name": "v", "arch": "tiny", "top_p": top_p},
                        device="cpu")

    def test_engine_spec_rejects_top_k(self):
        with pytest.raises(ValueError):
            LocalEngine({"name": "v", "arch": "tiny", "top_k": -1},
                        device="cpu")
        with pytest.raises(ValueError):
            resolve_sampling_filter({"arch": "tiny", "top_k": 2.5})
        with pytest.raises(ValueError):
            resolve_sampling_filter({"arch": "tiny", "top_p": float("nan")})
        assert resolve_sampling_filter({"arch": "tiny"}) == (1.0, 0)
        assert resolve_sampling_filter(
            {"arch": "tiny", "top_p": 0.9, "top_k": 40}) == (0.9, 40)

    def test_generate_rejects(self):
        eng = LocalEngine({"name": "v", "arch": "tiny"}, device="cpu")
        for top_p in BAD_TOP_P:
            with pytest.raises(ValueError):
                eng.generate("s", "u", max_tokens=2, top_p=top_p)
        with pytest.raises(ValueError):
            eng.generate("s", "u", max_tokens=2, top_k=-1)

    def test_ops_reject(self):
        row = geometric_row(V)
        for top_p in BAD_TOP_P:
            with pytest.raises(ValueError):
                ops.sample_filtered(row, 1.0, top_p, 0)
            with pytest.raises(ValueError):
                ops.nucleus_mask(row, 1.0, top_p, 0)
        with pytest.raises(ValueError):
            ops.sample_filtered(row, 1.0, 0.9, -1)

    @pytest.mark.parametrize("flag,value", [("--top-p", "0"),
                                            ("--top-p", "-0.1"),
                                            ("--top-p", "1.5"),
                                            ("--top-p", "abc"),
                                            ("--top-k", "-1"),
                                            ("--top-k", "2.5")])
    def test_cli_rejects_at_parse_time(self, flag, value):
        with pytest.raises(SystemExit):
            debate.create_parser().parse_args(
                ["local", "alias", "x", "tiny", flag, value])

    def test_handle_local_command_rejects(self, isolated_paths, capsys):
        for top_p in BAD_TOP_P:
            assert providers.handle_local_command(
                "alias", "x", "tiny", None, None, top_p=top_p) == 1
        assert providers.handle_local_command(
            "alias", "x", "tiny", None, None, top_k=-1) == 1
        assert "top_p" in capsys.readouterr().err
        assert not (isolated_paths / "config.json").exists()


class TestAliasAndEngine:
    def test_alias_round_trip(self, isolated_paths):
        args = debate.create_parser().parse_args(
            ["local", "alias", "x", "tiny", "--top-p", "0.9", "--top-k", "40"])
        assert (args.top_p, args.top_k) == (0.9, 40)
        assert debate.handle_utility_command(args) == 0
        stored = json.loads((isolated_paths / "config.json").read_text())
        alias = stored["local"]["custom_aliases"]["x"]
        assert alias["top_p"] == 0.9 and alias["top_k"] == 40
        spec = providers.resolve_local_model("x", stored["local"])
        eng = LocalEngine(spec, device="cpu")
        assert (eng.top_p, eng.top_k) == (0.9, 40)
        # without the flags the alias carries neither key
        args = debate.create_parser().parse_args(["local", "alias", "y", "tiny"])
        assert debate.handle_utility_command(args) == 0
        stored = json.loads((isolated_paths / "config.json").read_text())
        assert not {"top_p", "top_k"} & set(
            stored["local"]["custom_aliases"]["y"])

    def test_engine_cache_key_includes_defaults(self):
        clear_engines()
        try:
            a = get_engine({"name": "ck", "arch": "tiny"}, device="cpu")
            b = get_engine({"name": "ck", "arch": "tiny", "top_p": 0.9},
                           device="cpu")
            c = get_engine({"name": "ck", "arch": "tiny", "top_p": 0.9,
                            "top_k": 5}, device="cpu")
            assert a is not b and b is not c
            assert get_engine({"name": "ck", "arch": "tiny", "top_p": 0.9},
                              device="cpu") is b
        finally:
            clear_engines()

    def _record(self, monkeypatch):
        calls = []
        orig = ops.sample_filtered

        def wrapped(logits, temperature=0.7, top_p=1.0, top_k=0, **kw):
            tok = orig(logits, temperature=temperature, top_p=top_p,
                       top_k=top_k, **kw)
            keep = torch_ref.nucleus_keep(logits, temperature, top_p, top_k)
            calls.append((tok, bool(keep[tok]), int(keep.sum()), top_p, top_k))
            return tok

        monkeypatch.setattr(ops, "sample_filtered", wrapped)
        return calls

    def test_spec_default_top_p_is_used(self, monkeypatch):
        calls = self._record(monkeypatch)
        eng = LocalEngine({"name": "np", "arch": "tiny", "top_p": 0.9},
                          device="cpu")
        _, _, out_tok, _ = eng.generate("s", "u", max_tokens=12,
                                        temperature=0.7, timeout=300)
        assert out_tok > 0 and len(calls) >= out_tok
        assert all(in_set for _, in_set, _, _, _ in calls)
        assert all(p == 0.9 and k == 0 for *_, p, k in calls)
        # the filter does truncate this model's rows
        assert all(n < eng.config.vocab_size for _, _, n, _, _ in calls)

    def test_top_k_on_cpu_and_caller_overrides_default(self, monkeypatch):
        calls = self._record(monkeypatch)
        eng = LocalEngine({"name": "nk", "arch": "tiny", "top_p": 0.9},
                          device="cpu")
        eng.generate("s", "u", max_tokens=6, temperature=0.7, timeout=300,
                     top_p=1.0, top_k=3)
        assert calls and all(p == 1.0 and k == 3 for *_, p, k in calls)
        assert all(in_set and n <= 3 for _, in_set, n, _, _ in calls)
        # an unfiltered request never reaches the filtered sampler
        calls.clear()
        eng.generate("s", "u", max_tokens=4, temperature=0.7, timeout=300,
                     top_p=1.0, top_k=0)
        assert calls == []

    def test_backend_forwards_only_what_the_caller_gave(self, monkeypatch,
                                                        isolated_paths):
        seen = []

        class FakeEngine:
            def generate(self, *a, **kw):
                seen.append(kw)
                return "t", 1, 1, {}

        from adversarial_spec_amd.engine import local as local_mod

        monkeypatch.setattr(local_mod, "get_engine",
                            lambda spec, device=None: FakeEngine())
        be = LocalBackend("local/tiny", device="cpu")
        be.generate("s", "u", max_tokens=4, temperature=0.7, timeout=10)
        assert "top_p" not in seen[-1] and "top_k" not in seen[-1]
        be.generate("s", "u", max_tokens=4, temperature=0.7, timeout=10,
                    top_p=0.8)
        assert seen[-1]["top_p"] == 0.8 and "top_k" not in seen[-1]
        be.generate("s", "u", max_tokens=4, temperature=0.7, timeout=10,
                    top_k=7)
        assert seen[-1]["top_k"] == 7 and "top_p" not in seen[-1]
