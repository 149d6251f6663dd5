"""Decode GEMV kernels (ops/hip/gemv.hip, ops/hip/gemv_fp8.hip) at their loop
tails and row edges, without a numeric tolerance.

  - Inputs built from small integers make every fp32 product and partial sum
    exact in any order (tests/gemv_exact_common.py; the premise is checked in
    test_gemv_exact_cpu.py), so the fp64 result rounded once to bf16 must be
    reproduced bit for bit. Kernels with an inexact fp32 step between the
    exact dot and the store (rsqrtf, __expf, a non-power-of-two scale) must
    land on one of the two bf16 neighbours of the fp64 result.
  - A permutation probe (one-hot weight rows) makes every output name the
    one input element it read.
  - K takes the six lane splits of each kernel's unrolled / remainder loop
    pair, N the row tails of the 8-row and 16-row grids and both sides of the
    N == 8192 kernel switch.
  - Every destination is a slice of a sentinel-filled buffer, so a write
    outside [0, N) shows, in every test here.
  - The rowwise e4m3 quantizer is compared with torch over every bf16 value.
"""

import pytest
import torch

from gemv_exact_common import (
    BF16, BRACKET_OPS, EPS, EXACT_OPS, F8, K_LABELS, N_TAILS, OPS,
    SWITCHING_OPS, Case, bracket_violations, dense_case, e4m3_values, first_bad,
    fold_negative_zero, fp8_norm_probe, fp8_norm_probe_violations, head_rows,
    is_fp8, is_norm, k_cases, materialize, probe_case, quantizer_row,
    reference, rope_geometry, wln_pow2)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from adversarial_spec_amd import ops
else:  # collected but deselected on CPU
    ops = None

DEV = "cuda:0"
PAD = 64          # sentinel elements on either side of a destination
SENTINEL = {torch.bfloat16: 12352.0, torch.uint8: 0xA5, torch.float32: -123.0}
PROBE_KS = ("rem_only", "unrolled_plus_one")
ALL_OPS = tuple(OPS)


class Guarded:
    """A destination of n elements in the middle of a sentinel-filled buffer.
    PAD elements keep the slice 16-byte aligned for every dtype used."""

    def __init__(self, name, n, dtype, init=None):
        self.name, self.n, self.dtype = name, n, dtype
        self.buf = torch.full((n + 2 * PAD,), SENTINEL[dtype], dtype=dtype,
                              device=DEV)
        self.mid = self.buf[PAD:PAD + n]
        if init is not None:
            self.mid.copy_(init.reshape(-1))

    def check(self):
        b = self.buf.cpu()
        want = torch.full((PAD,), SENTINEL[self.dtype], dtype=self.dtype)
        assert torch.equal(b[:PAD], want), f"{self.name}: wrote below [0, N)"
        assert torch.equal(b[PAD + self.n:], want), (
            f"{self.name}: wrote past element N-1")


def run(c):
    """Run c.op on the GPU with every destination guarded. Returns the bf16
    result [N] on the CPU and, for the ops that fill the x8 / xs scratch,
    those too."""
    op, K, N = c.op, c.K, c.N
    d = {k: v.to(DEV) for k, v in materialize(c).items()}
    out = Guarded("out", N, BF16, init=d.get("resid"))
    o = out.mid.view(1, N)
    guards = [out]
    extra = {}
    if op in ("gemv_fp8", "gemv_fp8_res"):
        x8 = Guarded("x8", K, torch.uint8)
        xs = Guarded("xs", 1, torch.float32)
        guards += [x8, xs]
        d["x8"], d["xs"] = x8.mid.view(1, K), xs.mid

    if op == "gemv":
        ops.gemv(d["x"], d["w"], out=o)
    elif op == "gemv_res":
        ops.gemv_res(d["x"], d["w"], o)
    elif op == "gemv_gateup":
        ops.gemv_gateup(d["x"], d["w"], o)
    elif op == "gemv_norm":
        ops.gemv_norm(d["x"], d["wln"], d["w"], EPS, out=o)
    elif op == "gemv_gateup_norm":
        ops.gemv_gateup_norm(d["x"], d["wln"], d["w"], EPS, o)
    elif op == "gemv_norm_rope_kv":
        extra = _run_rope_kv(c, d, o)
    elif op == "gemv_fp8":
        ops.gemv_fp8(d["x"], d["w8"], d["wsc"], d["x8"], d["xs"], o)
    elif op == "gemv_fp8_q":
        ops.gemv_fp8_q(d["x8"], d["xs"], d["w8"], d["wsc"], o)
    elif op == "gemv_fp8_res":
        ops.gemv_fp8_res(d["x"], d["w8"], d["wsc"], d["x8"], d["xs"], o)
    elif op == "gemv_fp8_gateup":
        ops.gemv_fp8_gateup(d["x8"], d["xs"], d["w8"], d["wsc"], o)
    elif op == "gemv_fp8_norm":
        ops.gemv_fp8_norm(d["x"], d["wln"], d["w8"], d["wsc"], EPS, o)
    elif op == "gemv_fp8_resl":
        ops.gemv_fp8_resl(d["x"], d["w8"], d["wsc"], o)
    elif op == "gemv_fp8_gateup_norm":
        ops.gemv_fp8_gateup_norm(d["x"], d["wln"], d["w8"], d["wsc"], EPS, o)
    else:
        raise AssertionError(op)
    torch.cuda.synchronize()
    for g in guards:
        g.check()
    if op in ("gemv_fp8", "gemv_fp8_res"):
        extra = {"x8": x8.mid.cpu(), "xs": xs.mid.cpu()}
    return out.mid.cpu(), extra


def _run_rope_kv(c, d, o):
    """gemv_norm_rope_kv with cos = 1, sin = 0 (the identity rotation, exact
    in the kernel's fma form) at position 1 of a two-page cache whose page
    table is reversed. Returns the cache rows it has to have appended."""
    hq, kh, hd, N = rope_geometry(c.N)
    assert N == c.N
    cos = torch.ones(4, hd // 2, device=DEV)
    sin = torch.zeros(4, hd // 2, device=DEV)
    page = 2
    kc = torch.full((2, page, kh, hd), SENTINEL[BF16], dtype=BF16, device=DEV)
    vc = kc.clone()
    table = torch.tensor([1, 0], dtype=torch.int32, device=DEV)
    ops.gemv_norm_rope_kv(d["x"], d["wln"], d["w"], EPS, cos, sin, kc, vc,
                          table, 1, hq, kh, out=o)
    torch.cuda.synchronize()
    return {"kc": kc.cpu(), "vc": vc.cpu(), "geom": (hq, kh, hd)}


def check(c, got, extra):
    """The assertion of the op's class: bit-exact, or the bf16 bracket."""
    ref = reference(c)[0]
    if c.op in EXACT_OPS:
        want = ref.float().to(BF16)     # exact in fp32, then one rounding
        if not torch.equal(got, want):
            bad = torch.nonzero(got.float() != want.float()).flatten()
            if bad.numel() == 0:       # only the sign of a zero differs
                bad = torch.nonzero(got.view(torch.int16)
                                    != want.view(torch.int16)).flatten()
            n = int(bad[0])
            raise AssertionError(
                f"{first_bad(bad, c)}: got {got[n].item()} want "
                f"{want[n].item()}")
    else:
        bad = bracket_violations(got, ref)
        assert bad.numel() == 0, (
            f"{first_bad(bad, c)}: got {got[int(bad[0])].item()} for fp64 "
            f"{ref[int(bad[0])].item()!r}")
    if "x8" in extra and not hasattr(c, "cols"):
        # the scratch of a self-quantizing op: exact codes, scale exactly 2^j
        assert extra["xs"].item() == 2.0 ** c.j
        assert torch.equal(e4m3_values(extra["x8"]), c.x / 2.0 ** c.j)
    if "kc" in extra:
        hq, kh, hd = extra["geom"]
        for cache, lo in ((extra["kc"], hq * hd), (extra["vc"], (hq + kh) * hd)):
            assert torch.equal(cache[1, 1].reshape(-1), got[lo:lo + kh * hd])
            rest = cache.clone()
            rest[1, 1] = SENTINEL[BF16]
            assert (rest == SENTINEL[BF16]).all(), "cache write off its row"


def _ns(op):
    if op == "gemv_norm_rope_kv":
        return (48, 96)      # N == (hq + 2 * kh) * hd: no ragged row count
    return N_TAILS


def _js(op):
    return (-3, 2) if is_fp8(op) else (0,)


def _sweep(op, K, ns):
    for N in ns:
        for j in _js(op):
            c = dense_case(op, K, N, j=j)
            check(c, *run(c))


@pytest.mark.parametrize("label", K_LABELS)
@pytest.mark.parametrize("op", EXACT_OPS)
def test_exact(op, label):
    """fp32-exact inputs: the fp64 result rounded once to bf16, bit for bit,
    at every lane split and row tail of the 32-lane kernels."""
    _sweep(op, k_cases(OPS[op][0])[label], _ns(op))


@pytest.mark.parametrize("label", K_LABELS)
@pytest.mark.parametrize("op", BRACKET_OPS)
def test_bracket(op, label):
    """Same inputs through the kernels with an inexact fp32 epilogue: each
    output is one of the two bf16 neighbours of the fp64 result."""
    _sweep(op, k_cases(OPS[op][0])[label], _ns(op))


@pytest.mark.parametrize("op", SWITCHING_OPS)
def test_kernel_switch_boundary(op):
    """N == 8192 runs the 32-lane kernel, 8193 the 16-lane one."""
    K = k_cases(OPS[op][0])["rem_only"]
    big = dense_case(op, K, 8193, j=-3)
    for N in (8192, 8193):
        c = head_rows(big, N)
        check(c, *run(c))


@pytest.mark.parametrize("label", K_LABELS)
@pytest.mark.parametrize("op", SWITCHING_OPS)
def test_16_lane_kernels(op, label):
    """The 16-lane kernels only run above N == 8192: their own lane splits,
    at a row count that leaves one row (8193) and eight rows (8200) in the
    last 16-row block."""
    K = k_cases(OPS[op][1])[label]
    big = dense_case(op, K, 8200, j=2)
    for N in (8193, 8200):
        c = head_rows(big, N)
        check(c, *run(c))


def _probe(op, K, N):
    c = probe_case(op, K, N)
    got, extra = run(c)
    if is_fp8(op) and is_norm(op):
        bad = fp8_norm_probe_violations(got, c)
        assert bad.numel() == 0, (
            f"{first_bad(bad, c)}: got {got[int(bad[0])].item()}")
    else:
        check(c, got, extra)
    if "xs" in extra:
        assert extra["xs"].item() == 1.0
        assert torch.equal(e4m3_values(extra["x8"]), c.x)


@pytest.mark.parametrize("label", PROBE_KS)
@pytest.mark.parametrize("op", ALL_OPS)
def test_permutation_probe(op, label):
    """One-hot weight rows over N >= K rows: a dropped, duplicated or shifted
    chunk, or a wrong row, fails at a (row, column) the message names."""
    K = k_cases(OPS[op][0])[label]
    N = rope_geometry(K)[3] if op == "gemv_norm_rope_kv" else K + 1
    _probe(op, K, N)


@pytest.mark.parametrize("label", PROBE_KS)
@pytest.mark.parametrize("op", SWITCHING_OPS)
def test_permutation_probe_16_lane(op, label):
    _probe(op, k_cases(OPS[op][1])[label], 8193)


@pytest.mark.parametrize("op", ALL_OPS)
def test_no_write_outside_destination(op):
    """Ragged row counts with the destination (and the x8 / xs scratch of
    the ops that fill it) inside sentinels; run() asserts they are intact."""
    K = k_cases(OPS[op][0])["rem_only"]
    ns = (48,) if op == "gemv_norm_rope_kv" else (7, 9)
    _sweep(op, K, ns)
    if OPS[op][1] is not None:       # 16-lane kernel: 8193 % 16 == 1
        _sweep(op, k_cases(OPS[op][1])["rem_only"], (8193,))


class TestQuantNormFp8:
    """quant_norm_fp8: the quantization decision sits on an inexact rms, so
    each code is one of the two e4m3 neighbours of the fp64 value."""

    # one active thread; a ragged second pass of the 256-thread block loop
    @pytest.mark.parametrize("K", [8, 264, 2056, 4360])
    def test_codes_and_scale(self, K):
        c = Case(op="quant_norm_fp8", K=K, wln=wln_pow2(K),
                 x=((torch.arange(K) % 251) + 1).double())
        lo, hi, s = fp8_norm_probe(c)
        x8 = Guarded("x8", K, torch.uint8)
        xs = Guarded("xs", 1, torch.float32)
        x = c.x.to(BF16).view(1, K).to(DEV)
        ops.quant_norm_fp8(x, c.wln.to(BF16).to(DEV), x8.mid.view(1, K),
                           xs.mid, EPS)
        torch.cuda.synchronize()
        x8.check()
        xs.check()
        got = e4m3_values(x8.mid.cpu())
        bad = torch.nonzero((got != lo) & (got != hi)).flatten()
        assert bad.numel() == 0, (
            f"K={K}: element {int(bad[0])} quantized to "
            f"{got[int(bad[0])].item()}, neighbours "
            f"{lo[int(bad[0])].item()} / {hi[int(bad[0])].item()}")
        # a handful of fp32 roundings (sum, divide, rsqrt, two products)
        torch.testing.assert_close(xs.mid.cpu().double(),
                                   torch.tensor([s], dtype=torch.float64),
                                   rtol=1e-6, atol=0)


class TestQuantizerExhaustive:
    """quant_fp8 over every bf16 value in [-448, 448] against torch's
    round-to-nearest-even float8_e4m3fn cast, code for code."""

    @pytest.mark.parametrize("shift", [0, -3])
    def test_every_bf16_value(self, shift):
        from adversarial_spec_amd.ops import _advspec_hip

        row = (quantizer_row().float() * 2.0 ** shift).to(BF16)
        K = row.numel()
        scale = 2.0 ** shift             # amax / 448, exact
        assert row.float().abs().max().item() == 448 * scale
        q = Guarded("q", K, torch.uint8)
        sc = Guarded("scale", 1, torch.float32)
        _advspec_hip.quant_fp8(row.view(1, K).to(DEV), q.mid.view(1, K),
                               sc.mid)
        torch.cuda.synchronize()
        q.check()
        sc.check()
        assert sc.mid.item() == scale
        want = (row.float() / scale).to(F8).view(torch.uint8)
        got = fold_negative_zero(q.mid.cpu())
        want = fold_negative_zero(want)
        bad = torch.nonzero(got != want).flatten()
        ties = 0
        if bad.numel():
            v = (row.double() / scale)[bad]
            mid = (e4m3_values(got[bad]) + e4m3_values(want[bad])) / 2
            ties = int((v == mid).sum())
        assert bad.numel() == 0, (
            f"{bad.numel()} codes differ from torch ({ties} exact ties, "
            f"{bad.numel() - ties} not), first: x={row[int(bad[0])].item()} "
            f"got 0x{int(got[bad[0]]):02x} want 0x{int(want[bad[0]]):02x}")


class TestHostChecks:
    """The fp8 GEMV entry points refuse, before any launch, a K that is no
    multiple of 16, an activation of the wrong length and a non-bf16
    destination. Every call here is one the host refuses."""

    def _operands(self, K, N, rows=None):
        rows = rows or N
        return dict(
            x=torch.ones(1, K, dtype=BF16, device=DEV),
            w8=torch.full((rows, K), 0x38, dtype=torch.uint8, device=DEV),
            wsc=torch.ones(rows, device=DEV),
            x8=torch.full((1, K), 0x38, dtype=torch.uint8, device=DEV),
            xs=torch.ones(1, device=DEV),
            out=torch.full((1, N), SENTINEL[BF16], dtype=BF16, device=DEV))

    def _call(self, op, t):
        if op == "gemv_fp8":
            ops.gemv_fp8(t["x"], t["w8"], t["wsc"], t["x8"], t["xs"], t["out"])
        elif op == "gemv_fp8_q":
            ops.gemv_fp8_q(t["x8"], t["xs"], t["w8"], t["wsc"], t["out"])
        elif op == "gemv_fp8_res":
            ops.gemv_fp8_res(t["x"], t["w8"], t["wsc"], t["x8"], t["xs"],
                             t["out"])
        else:
            ops.gemv_fp8_gateup(t["x8"], t["xs"], t["w8"], t["wsc"], t["out"])

    def _refused(self, op, t):
        before = {k: v.clone() for k, v in t.items()}
        with pytest.raises(RuntimeError):
            self._call(op, t)
        torch.cuda.synchronize()
        for k, v in t.items():
            assert torch.equal(v, before[k]), f"{op}: {k} changed"

    OPS4 = ("gemv_fp8", "gemv_fp8_q", "gemv_fp8_res", "gemv_fp8_gateup")

    def _rows(self, op, N):
        return 2 * N if op == "gemv_fp8_gateup" else N

    @pytest.mark.parametrize("op", OPS4)
    def test_k_not_a_multiple_of_16(self, op):
        self._refused(op, self._operands(24, 8, self._rows(op, 8)))

    @pytest.mark.parametrize("op", OPS4)
    def test_activation_length(self, op):
        t = self._operands(32, 8, self._rows(op, 8))
        t["x"] = t["x"][:, :16].contiguous()
        t["x8"] = t["x8"][:, :16].contiguous()
        self._refused(op, t)

    @pytest.mark.parametrize("op", OPS4)
    def test_fp32_destination(self, op):
        t = self._operands(32, 8, self._rows(op, 8))
        t["out"] = torch.full((1, 8), -1.0, device=DEV)
        self._refused(op, t)

    @pytest.mark.parametrize("op", OPS4)
    def test_accepted_shape_still_runs(self, op):
        """The same operands at K = 32 are accepted: 32 codes of 1.0 against
        weight rows of 1.0."""
        t = self._operands(32, 8, self._rows(op, 8))
        if op == "gemv_fp8_res":
            t["out"].zero_()
        self._call(op, t)
        torch.cuda.synchronize()
        want = 32.0 if op != "gemv_fp8_gateup" else 32.0 * 32.0
        assert (t["out"].float() == want).all()
