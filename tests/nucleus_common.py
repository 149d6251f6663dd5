"""Hand-built logits rows shared by the top-p / top-k sampling tests.

Every row is bf16, so the CPU reference and the GPU kernel see the same
values. Heads are scattered through the row (stride 131, odd, so a
permutation for any power-of-two vocab) and the rest is padded with a very
negative logit whose probability is zero in any arithmetic.
"""

from __future__ import annotations

import torch

from adversarial_spec_amd.ops import torch_ref

PAD = -1.0e4
# the cut-accuracy bound of the kernel: a group whose strictly-greater mass
# G lies within BAND of top_p may fall on either side
BAND = 1e-4


def _scatter(vocab: int, values: list[float]) -> torch.Tensor:
    assert len(values) <= vocab
    row = torch.full((vocab,), PAD, dtype=torch.float32)
    for k, v in enumerate(values):
        row[(k * 131 + 7) % vocab] = v
    return row.to(torch.bfloat16)


def head_index(vocab: int, k: int) -> int:
    return (k * 131 + 7) % vocab


def geometric_row(vocab: int) -> torch.Tensor:
    """p ~ 0.497, 0.250, 0.126, 0.063, ...: logit_k = -k * 11/16 (exact in
    bf16), ratio exp(-11/16) = 0.5028, so the prefix sums 0.497 / 0.747 /
    0.873 / 0.936 sit well away from top_p = 0.5 and 0.9."""
    n = min(16, vocab)
    return _scatter(vocab, [-k * 0.6875 for k in range(n)])


def tie_row(vocab: int, n_top: int = 8, n_low: int = 4) -> torch.Tensor:
    """n_top tokens share the top logit 0; n_low tokens sit at log(0.5).
    With 8 + 4: p = 0.1 each for the top group, 0.05 each below."""
    return _scatter(vocab, [0.0] * n_top + [-0.6931] * n_low)


def descending_row(vocab: int) -> torch.Tensor:
    """Strictly descending logits -k/4 (exact in bf16), no ties."""
    n = min(32, vocab)
    return _scatter(vocab, [-k * 0.25 for k in range(n)])


def mixed_sign_row(vocab: int = 1024) -> tuple[torch.Tensor, float]:
    """(row, T): +/-1e30, +/-1e-30, both signed zeros and a -3e38 pad, to be
    sampled at T = 1e30 so that logit / T is +1, ~0, -1 and -300.
    Weights: 2 x e, 4 x 1 (+1e-30), 16 x 1 (eight +0.0 and eight -0.0),
    4 x 1 (-1e-30), 4 x 1/e; Z = 30.9. G is 0, 0.176, 0.305, 0.823, 0.952
    down the groups: top_p = 0.5 keeps the zeros only if +0.0 and -0.0 are
    one group (on its own the -0.0 half would have G = 0.564)."""
    vals = ([1e30] * 2 + [1e-30] * 4 + [0.0, -0.0] * 8 + [-1e-30] * 4
            + [-1e30] * 4)
    row = torch.full((vocab,), -3.0e38, dtype=torch.float32)
    for k, v in enumerate(vals):
        row[head_index(vocab, k)] = v
    return row.to(torch.bfloat16), 1e30


def band_count(row: torch.Tensor, temperature: float, top_p: float) -> int:
    """Number of tokens whose float64 G lies within BAND of top_p: must be
    0 for an exact mask comparison to be decided by the contract. The
    argmax group (G == 0) is kept whatever top_p is, so it never counts."""
    g, _ = torch_ref.nucleus_mass_above(row.cpu(), temperature)
    return int((((g - top_p).abs() < BAND) & (g > 0)).sum())
