"""Top-p / top-k filtered sampling on the GPU: the kernels' kept set against
the float64 contract bit for bit, the draw's support, distribution and
determinism, and the engine decoding filtered requests through the captured
graph.

Exact mask comparisons are decided by the contract only when no value group
has its strictly-greater mass G within 1e-4 (the kernel's cut accuracy) of
top_p; every such test asserts that first."""

from __future__ import annotations

import functools
import math
from pathlib import Path

import numpy as np
import pytest
import torch

from nucleus_common import (band_count, descending_row, geometric_row,
                            head_index, mixed_sign_row, tie_row)

from adversarial_spec_amd import ops
from adversarial_spec_amd.engine.local import LocalEngine
from adversarial_spec_amd.ops import torch_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WIDE = 128256
GOLDEN = Path(__file__).parent / "golden" / "sample_unfiltered_ids.npy"


def _hip():
    return ops._require_hip()


@functools.lru_cache(maxsize=None)
def _wide_row(seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(WIDE, generator=g) * 2).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _wide_row_dev(seed: int) -> torch.Tensor:
    return _wide_row(seed).to(DEV)


def _assert_mask_exact(row, t, top_p, top_k=0):
    """row on the CPU; compares the kernel's mask with the reference."""
    if t > 0 and top_p < 1.0:
        assert band_count(row, t, top_p) == 0, "input no longer decides the cut"
    ref = torch_ref.nucleus_keep(row, t, top_p, top_k)
    got = _hip().nucleus_mask(row.to(DEV), t, top_p, top_k)
    assert got.dtype == torch.uint8 and got.shape == (row.numel(),)
    got = got.cpu().bool()
    diff = (got != ref).nonzero().flatten().tolist()
    assert not diff, (f"kept {int(got.sum())} vs reference {int(ref.sum())}, "
                      f"first differing ids {diff[:8]}")
    # a threshold set: every kept logit >= every dropped logit
    lf = row.float()
    if (~got).any():
        assert lf[got].min() > lf[~got].max()
    return int(ref.sum())


class TestMaskSmall:
    @pytest.mark.parametrize("vocab", [8, 1024])
    @pytest.mark.parametrize("top_p,top_k", [(0.9, 0), (0.5, 0), (1e-6, 0),
                                             (0.9, 2), (0.5, 3), (1.0, 3),
                                             (1.0, 0)])
    def test_geometric(self, vocab, top_p, top_k):
        n = _assert_mask_exact(geometric_row(vocab), 1.0, top_p, top_k)
        if vocab == 1024 and top_k == 0 and top_p < 1.0:
            assert n == {0.9: 4, 0.5: 2, 1e-6: 1}[top_p]

    @pytest.mark.parametrize("top_p,top_k", [(0.45, 0), (0.45, 3), (1.0, 3),
                                             (0.85, 0)])
    def test_tie_group(self, top_p, top_k):
        n = _assert_mask_exact(tie_row(1024), 1.0, top_p, top_k)
        assert n == (12 if top_p == 0.85 else 8)
        # vocab 8: one bf16x8 vector, 1023 idle lanes; 5 tied + 3 below
        n = _assert_mask_exact(tie_row(8, n_top=5, n_low=3), 1.0, 0.45, top_k)
        assert n == 5

    @pytest.mark.parametrize("vocab", [8, 1024])
    def test_top_k_distinct(self, vocab):
        for top_k in (1, 3, 7):
            assert _assert_mask_exact(descending_row(vocab), 1.0, 1.0,
                                      top_k) == top_k

    @pytest.mark.parametrize("t", [0.25, 1.0, 4.0])
    def test_temperature(self, t):
        _assert_mask_exact(geometric_row(1024), t, 0.9)

    @pytest.mark.parametrize("vocab", [8, 1024, WIDE])
    def test_all_equal_row_keeps_everything(self, vocab):
        """One group of `vocab` tokens: kept whole for any top_p / top_k, and
        its count (128 256 at real width) must not overflow."""
        row = torch.full((vocab,), 1.5).to(torch.bfloat16)
        for top_p, top_k in ((1e-3, 0), (0.5, 0), (1.0, 5), (0.3, 1)):
            assert _assert_mask_exact(row, 0.7, top_p, top_k) == vocab

    def test_mixed_sign_extreme_and_signed_zeros(self):
        row, t = mixed_sign_row(1024)
        assert int((row.view(torch.int16) == -32768).sum()) == 8  # -0.0 bits
        # G down the groups: 0, 0.176, 0.305 (both zeros), 0.823, 0.952
        for top_p, n in ((0.1, 2), (0.25, 6), (0.5, 22), (0.9, 26),
                         (0.99, 30)):
            assert _assert_mask_exact(row, t, top_p) == n
        assert _assert_mask_exact(row, t, 1.0, top_k=7) == 22

    def test_cut_below_the_first_histogram_window(self):
        """Logits in [-5, -1] under a maximum of 8 at T = 8: the histogram
        window below the maximum's key ends near -0.5, so the cut is found
        in the second pass over the key space."""
        g = torch.Generator().manual_seed(5)
        row = (-torch.rand(1024, generator=g) * 4 - 1).to(torch.bfloat16)
        row[head_index(1024, 0)] = 8.0
        for top_p in (0.3, 0.7, 0.97):
            n = _assert_mask_exact(row, 8.0, top_p)
            assert 100 < n < 1024
        _assert_mask_exact(row, 8.0, 1.0, top_k=500)

    def test_greedy_mask_is_the_argmax_group(self):
        assert _assert_mask_exact(tie_row(1024), 0.0, 0.45, 3) == 8


class TestMaskRealWidth:
    @pytest.mark.parametrize("seed", [0, 1, 2])
    @pytest.mark.parametrize("t,top_p", [(0.7, 0.9), (1.0, 0.5), (0.3, 0.95)])
    def test_randn_rows(self, seed, t, top_p):
        n = _assert_mask_exact(_wide_row(seed), t, top_p)
        assert 6 <= n <= 7954

    @pytest.mark.parametrize("top_k", [1, 40])
    def test_top_k(self, top_k):
        n = _assert_mask_exact(_wide_row(0), 0.7, 0.9, top_k)
        assert top_k <= n <= top_k + 8  # whole groups: a tie may add a few

    def test_binding_rejects_bad_arguments(self):
        row = _wide_row_dev(0)
        hip = _hip()
        with pytest.raises(RuntimeError):
            hip.nucleus_mask(row[:12], 0.7, 0.9, 0)        # vocab % 8
        with pytest.raises(RuntimeError):
            hip.nucleus_mask(row, 0.7, 0.0, 0)
        with pytest.raises(RuntimeError):
            hip.sample_filtered(row, 0.7, 1.5, 0, 1)
        with pytest.raises(RuntimeError):
            hip.sample_filtered(row, 0.7, 0.9, -1, 1)
        with pytest.raises(RuntimeError):
            hip.sample_filtered(row.float(), 0.7, 0.9, 0, 1)
        with pytest.raises(ValueError):
            ops.sample_filtered(row, 0.7, 0.0, 0, seed=1)


class _State:
    """The device words of one graph-state sampling loop."""

    def __init__(self, n, temp, top_p, top_k, seed):
        i32 = dict(dtype=torch.int32, device=DEV)
        self.temp = torch.tensor([temp], dtype=torch.float32, device=DEV)
        self.top_p = torch.tensor([top_p], dtype=torch.float32, device=DEV)
        self.top_k = torch.tensor([top_k], **i32)
        self.rng = torch.tensor([seed], **i32)
        self.step = torch.zeros(1, **i32)
        self.pos = torch.zeros(1, **i32)
        self.hist = torch.full((n,), -1, **i32)
        self.tok_long = torch.zeros(1, dtype=torch.int64, device=DEV)

    def sample(self, row):
        _hip().sample_state_filtered(row, self.temp, self.top_p, self.top_k,
                                     self.rng, self.hist, self.step,
                                     self.tok_long)

    def bump(self):
        _hip().bump(self.pos, self.step)


class TestDraw:
    def test_support_and_distribution(self):
        n = 4096
        row = geometric_row(1024)
        keep = torch_ref.nucleus_keep(row, 1.0, 0.9)
        assert int(keep.sum()) == 4
        st = _State(n, 1.0, 0.9, 0, seed=12345)
        rng_hist = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
        drow = row.to(DEV)
        rng_hist[0:1].copy_(st.rng)
        for i in range(n):          # no host sync inside the loop
            st.sample(drow)
            st.bump()
            rng_hist[i + 1:i + 2].copy_(st.rng)
        toks = st.hist.cpu()
        assert int(st.step.item()) == n and int(st.tok_long.item()) == int(toks[-1])
        assert bool(keep[toks.long()].all()), "token outside the kept set"
        # Pearson chi-square against the renormalised reference
        p = torch.softmax(row.double(), -1) * keep
        p = p / p.sum()
        ids = keep.nonzero().flatten()
        obs = torch.bincount(toks.long(), minlength=1024)[ids].double()
        exp = p[ids] * n
        chi2 = float(((obs - exp) ** 2 / exp).sum())
        d = len(ids) - 1
        print(f"chi2 {chi2:.3f} over {d} dof, bound {d + 6 * math.sqrt(2 * d):.3f}")
        assert chi2 < d + 6 * math.sqrt(2 * d)
        rng = rng_hist.cpu()
        assert bool((rng != 0).all())
        assert bool((rng[1:] != rng[:-1]).all())

    def test_deterministic_and_entries_agree(self):
        row = _wide_row_dev(0)
        keep = torch_ref.nucleus_keep(_wide_row(0), 0.7, 0.9)
        hip = _hip()
        seeds = [1 + 7919 * i for i in range(64)]
        first = [hip.sample_filtered(row, 0.7, 0.9, 0, s) for s in seeds]
        again = [hip.sample_filtered(row, 0.7, 0.9, 0, s) for s in seeds]
        assert first == again
        assert all(bool(keep[t]) for t in first)
        assert len(set(first)) > 8  # the seed matters
        st = _State(64, 0.7, 0.9, 0, seed=1)
        for s in seeds:
            st.rng.fill_(s)
            st.sample(row)
            st.bump()
        assert st.hist.cpu().tolist() == first

    def test_top_k_draw_support(self):
        row = _wide_row_dev(1)
        keep = torch_ref.nucleus_keep(_wide_row(1), 0.7, 1.0, 40)
        toks = {_hip().sample_filtered(row, 0.7, 1.0, 40, s)
                for s in range(1, 65)}
        assert all(bool(keep[t]) for t in toks) and len(toks) > 4

    @pytest.mark.parametrize("top_p,top_k", [(0.3, 0), (1.0, 5), (0.9, 40)])
    def test_greedy(self, top_p, top_k):
        hip = _hip()
        ties = tie_row(1024)
        want = min(head_index(1024, k) for k in range(8))
        assert hip.sample_filtered(ties.to(DEV), 0.0, top_p, top_k, 9) == want
        wide = _wide_row(2)
        want = int((wide.float() == wide.float().max()).nonzero()[0])
        assert hip.sample_filtered(_wide_row_dev(2), 0.0, top_p, top_k, 9) == want
        assert hip.sample(_wide_row_dev(2), 0.0, 1.0, 9) == want
        st = _State(1, 0.0, top_p, top_k, seed=9)
        st.sample(_wide_row_dev(2))
        assert int(st.hist[0].item()) == want

    def test_unfiltered_kernel_untouched(self):
        """hip.sample for 32 seeds returns the ids recorded from a build of
        the commit before the filtered sampler existed."""
        want = np.load(GOLDEN)
        assert want.shape == (32,)
        row = _wide_row_dev(0)
        got = [_hip().sample(row, 0.7, 1.0, seed) for seed in range(1, 33)]
        assert got == want.tolist()


def _generate_ids(eng, monkeypatch, **kw):
    captured = []
    orig = eng.tokenizer.decode

    def capture(ids):
        captured.append(list(ids))
        return orig(ids)

    monkeypatch.setattr(eng.tokenizer, "decode", capture)
    out = eng.generate("sys", "nucleus prompt", timeout=300, **kw)
    monkeypatch.setattr(eng.tokenizer, "decode", orig)
    return captured[-1], out


class TestEngine:
    def test_filtered_request_is_graphed_and_matches_eager(self, monkeypatch):
        eng = LocalEngine({"name": "nuc", "arch": "tiny"}, device=DEV)
        a, out = _generate_ids(eng, monkeypatch, top_p=0.9, temperature=0.7,
                               max_tokens=24)
        assert eng._graph_state is not None, "filtered decode was not captured"
        assert eng._graph_state["key"][-1] is True
        assert out[2] == len(a) > 0
        monkeypatch.setenv("ADVSPEC_NO_GRAPH", "1")
        eager = LocalEngine({"name": "nuc", "arch": "tiny"}, device=DEV)
        b, _ = _generate_ids(eager, monkeypatch, top_p=0.9, temperature=0.7,
                             max_tokens=24)
        assert eager._graph_state is None
        div = next((i for i, (p, q) in enumerate(zip(a, b)) if p != q), None)
        assert a == b, f"diverge at {div}: graph={a} eager={b}"

    def test_settings_change_without_recapture_and_flip_recaptures(
            self, monkeypatch):
        eng = LocalEngine({"name": "nuc2", "arch": "tiny"}, device=DEV)
        eng.generate("s", "u", max_tokens=16, temperature=0.7, top_p=0.9,
                     timeout=300)
        gs = eng._graph_state
        assert gs is not None
        graph = gs["graph"]
        _, _, n, _ = eng.generate("s", "u", max_tokens=16, temperature=0.7,
                                  top_p=0.5, timeout=300)
        assert n > 0 and eng._graph_state["graph"] is graph
        assert float(gs["top_p_state"].item()) == 0.5
        _, _, n, _ = eng.generate("s", "u", max_tokens=16, temperature=0.7,
                                  top_p=1.0, top_k=7, timeout=300)
        assert n > 0 and eng._graph_state["graph"] is graph
        assert int(gs["top_k_state"].item()) == 7
        # unfiltered: the other graph
        _, _, n, _ = eng.generate("s", "u", max_tokens=16, temperature=0.7,
                                  timeout=300)
        assert n > 0
        assert eng._graph_state is not None
        assert eng._graph_state["graph"] is not graph
        assert eng._graph_state["key"][-1] is False
        assert eng._graph_state["top_p_state"] is None

    def test_unfiltered_step_calls_the_unfiltered_kernel(self, monkeypatch):
        hip = _hip()
        calls = {"plain": 0, "filtered": 0}

        class Spy:
            def __getattr__(self, name):
                return getattr(hip, name)

            def sample_state(self, *a):
                calls["plain"] += 1
                return hip.sample_state(*a)

            def sample_state_filtered(self, *a):
                calls["filtered"] += 1
                return hip.sample_state_filtered(*a)

        monkeypatch.setattr(ops, "_load_hip", lambda: Spy())
        eng = LocalEngine({"name": "nuc3", "arch": "tiny"}, device=DEV)
        eng.generate("s", "u", max_tokens=12, temperature=0.7, timeout=300)
        assert calls["plain"] > 0 and calls["filtered"] == 0
        eng.generate("s", "u", max_tokens=12, temperature=0.7, top_k=5,
                     timeout=300)
        assert calls["filtered"] > 0

    def test_spec_default_top_p_is_honoured(self, monkeypatch):
        eng = LocalEngine({"name": "nuc4", "arch": "tiny", "top_p": 0.9},
                          device=DEV)
        _, _, n, _ = eng.generate("s", "u", max_tokens=16, temperature=0.7,
                                  timeout=300)
        gs = eng._graph_state
        assert n > 0 and gs is not None and gs["key"][-1] is True
        assert abs(float(gs["top_p_state"].item()) - 0.9) < 1e-6
        assert int(gs["top_k_state"].item()) == 0
