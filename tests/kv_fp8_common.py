"""Helpers shared by test_kv_fp8_cpu.py and test_kv_fp8_gpu.py: the e4m3fn
grid spacing and the half-step bound of the quantizer contract. Depends on
torch alone."""

import torch


def e4m3_step(y):
    """Spacing of the e4m3fn grid at magnitude |y| (fp32 tensor): 2^-9 in
    the subnormal range below 2^-6, otherwise 2^(floor(log2|y|) - 3)."""
    a = y.abs().double()
    e = torch.floor(torch.log2(a.clamp_min(2.0 ** -20)))
    return torch.where(a < 2.0 ** -6, torch.full_like(a, 2.0 ** -9),
                       torch.pow(2.0, e - 3))


def assert_half_step(x, q8, scale, name=""):
    """|dequant - x| <= scale * step(x/scale)/2 * (1 + 1e-3), elementwise."""
    x = x.double()
    s = scale.double().unsqueeze(-1)
    deq = q8.view(torch.float8_e4m3fn).double() * s
    bound = s * e4m3_step((x / s).float()) / 2 * (1 + 1e-3)
    err = (deq - x).abs()
    worst = (err / bound).max().item()
    print(f"{name} worst err/bound {worst:.4f}")
    assert torch.isfinite(deq).all()
    assert (err <= bound).all(), f"{name}: worst err/bound {worst}"
