"""Decode attention through the combine kernel's two walks vs float64.

`attn_decode_combine_kernel` keeps a wave's split states in registers when
`n_splits <= 64` (every wave owns at most 16 splits) and walks them in two
passes over memory above that. The cases pin the split counts where its
code changes shape:

  n_splits   what it exercises
  2          two waves own one split each, two waves none
  17         one full round of 4 per wave, then a ragged round in wave 0
  18         the most seq=1100 can be cut into (one 64-position tile each)
  64         the last count on the register path: four full rounds per wave
  65         the first count on the two-pass path

Geometry: kh=2, group=4, hd=128. The launcher never cuts a sequence finer
than one 64-position tile per split (n_splits <= ceil(seq / 64)), so
seq=1100 reaches 2 and 18 splits and no more; 17, 64 and 65 splits use the
shortest ragged lengths that reach them (64 * (n - 1) + 12). Every case
asserts its geometry through `decode_split_geometry`.

Reference and tolerance are those of tests/test_attention_edges_gpu.py:
float64 softmax attention over the same bf16 inputs, atol = rtol = 2e-2,
elementwise, zero elements out of bound.
"""

import functools
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from adversarial_spec_amd import ops
    from adversarial_spec_amd.ops import _advspec_hip as _hip
else:  # collected but deselected on CPU
    ops = _hip = None

DEV = "cuda:0"
KH, GROUP, HD, PAGE = 2, 4, 128, 64
DECODE_TOL = dict(atol=2e-2, rtol=2e-2)

# (seq, split_blocks, n_splits)
CASES = [
    (1100, 4, 2),
    (1036, 34, 17),
    (1100, 36, 18),
    (4044, 128, 64),
    (4108, 130, 65),
]


def _bf(x):
    return x.to(torch.bfloat16)


def ref_decode(q, kc, vc, table, seq_len):
    """float64 softmax attention of q [hq, hd] over logical positions
    [0, seq_len) of the paged caches [n_pages, page, kh, hd]; unrounded."""
    page = kc.shape[1]
    n_used = (seq_len + page - 1) // page
    phys = table.cpu()[:n_used].long()
    k = kc.cpu()[phys].reshape(n_used * page, KH, HD)[:seq_len].double()
    v = vc.cpu()[phys].reshape(n_used * page, KH, HD)[:seq_len].double()
    k = k.repeat_interleave(GROUP, dim=1)  # [seq, hq, hd]
    v = v.repeat_interleave(GROUP, dim=1)
    s = torch.einsum("hd,khd->hk", q.cpu().double(), k) / math.sqrt(HD)
    p = torch.softmax(s, dim=-1)
    return torch.einsum("hk,khd->hd", p, v)


def _assert_within(got, want, atol, rtol, name):
    g = got.double().cpu()
    assert g.shape == want.shape, f"{name}: shape {g.shape} vs {want.shape}"
    assert torch.isfinite(g).all(), f"{name}: non-finite output"
    err = (g - want).abs()
    bound = atol + rtol * want.abs()
    n_bad = int((err > bound).sum())
    print(f"{name}: max err {err.max():.4g}, worst err/bound "
          f"{(err / bound).max():.3f}")
    assert n_bad == 0, (
        f"{name}: max err {err.max():.4g}; {n_bad}/{err.numel()} out of tol")


@functools.lru_cache(maxsize=None)
def _inputs(cover):
    """CPU inputs whose cache holds `cover` positions behind a permuted
    page table; built once per length and never written."""
    gen = torch.Generator().manual_seed(cover)
    n_used = (cover + PAGE - 1) // PAGE
    npg = n_used + 2
    table = torch.randperm(npg, generator=gen).to(torch.int32)
    q = _bf(torch.randn(KH * GROUP, HD, generator=gen))
    kc = _bf(torch.randn(npg, PAGE, KH, HD, generator=gen))
    vc = _bf(torch.randn(npg, PAGE, KH, HD, generator=gen))
    return q, kc, vc, table


@functools.lru_cache(maxsize=None)
def _reference(cover, seq):
    return ref_decode(*_inputs(cover), seq)


def _check_geometry(bound, split_blocks, n_splits):
    env = os.environ.get("ADVSPEC_SPLIT_BLOCKS")
    ns, sl = _hip.decode_split_geometry(bound, KH, split_blocks)
    assert env is None and ns == n_splits, (
        f"decode geometry for bound={bound} split_blocks={split_blocks}: "
        f"{ns} splits x split_len {sl}, this case needs {n_splits}. "
        f"ADVSPEC_SPLIT_BLOCKS={env!r} must be unset for these tests.")
    return sl


@pytest.mark.parametrize("seq,split_blocks,n_splits", CASES)
def test_combine_vs_fp64(seq, split_blocks, n_splits):
    _check_geometry(seq, split_blocks, n_splits)
    q, kc, vc, table = (t.to(DEV) for t in _inputs(seq))
    got = ops.attn_decode_paged(q, kc, vc, table, seq,
                                split_blocks=split_blocks)
    _assert_within(got, _reference(seq, seq), **DECODE_TOL,
                   name=f"combine n_splits={n_splits} seq={seq}")


@pytest.mark.parametrize("seq,split_blocks,n_splits", CASES)
def test_graph_mode_equals_host_length(seq, split_blocks, n_splits):
    """The device-position entry at full length launches the same grid and
    must give the same bits as the host-length entry."""
    _check_geometry(seq, split_blocks, n_splits)
    q, kc, vc, table = (t.to(DEV) for t in _inputs(seq))
    host = ops.attn_decode_paged(q, kc, vc, table, seq,
                                 split_blocks=split_blocks)
    pos = torch.tensor([seq - 1], dtype=torch.int32, device=DEV)
    dev = ops.attn_decode_paged(q, kc, vc, table, seq, pos_state=pos,
                                split_blocks=split_blocks)
    assert torch.equal(host, dev)


@pytest.mark.parametrize("bound,split_blocks,n_splits,pos", [
    (4044, 128, 64, 699),   # register path: 11 live splits, 53 empty
    (4044, 128, 64, 0),     # a single live split of one position
    (4108, 130, 65, 699),   # two-pass path, same emptiness
])
def test_trailing_splits_empty(bound, split_blocks, n_splits, pos):
    """Graph mode with the position well below the bound that sizes the
    grid: every split past it publishes an empty state (m = -inf, l = 0)
    that the combine must weigh as zero."""
    sl = _check_geometry(bound, split_blocks, n_splits)
    live = -(-(pos + 1) // sl)
    assert 1 <= live < n_splits - 16, (live, n_splits)
    q, kc, vc, table = (t.to(DEV) for t in _inputs(bound))
    got = ops.attn_decode_paged(
        q, kc, vc, table, bound,
        pos_state=torch.tensor([pos], dtype=torch.int32, device=DEV),
        split_blocks=split_blocks)
    _assert_within(got, _reference(bound, pos + 1), **DECODE_TOL,
                   name=f"combine empty tail n_splits={n_splits} pos={pos}")
