"""The four prefill MFMA GEMMs (ops/hip/gemm_tiles.h; entries in gemm.hip and
gemm_fp8.hip; gemm256.hip) at their tile, K-tail and dispatch edges, without a
numeric tolerance.

  - Small-integer inputs make every fp32 partial sum exact in any order
    (tests/gemm_exact_common.py; the premises and the coverage of the shape
    lists are checked in test_gemm_exact_cpu.py), so the exact result rounded
    once to bf16 must be reproduced bit for bit: one dropped, doubled or
    misplaced K element changes an output. Where the epilogue multiplies by
    a scale that is no power of two, the result must be one of the two bf16
    neighbours of the fp64 value.
  - A gather probe (one-hot weight rows) makes every output name the one k
    it read.
  - Every operand is an interior row-slice of a parent whose other rows are
    NaN (bf16, f32 scales) or 0x7F, the e4m3 NaN (codes): a read past the
    last row that reaches a stored output shows.
  - The bindings refuse a K they cannot stage whole 16-byte chunks of, and
    operands of the wrong rank, dtype, device or length, before any launch.
"""

import functools

import pytest
import torch

from gemm_exact_common import (
    BF16, F8, SHAPES_128, SHAPES_128_FP8, SHAPES_256, SHAPES_256_FP8,
    SHAPES_DISPATCH, SHAPES_FP8_RANDN, bf16_case, bracket_message,
    dispatch256, e4m3_bytes, first_mismatch, fp8_case, fp8_exact_expected,
    fp8_expected, fp8_randn_case, guarded_rows, probe_case, probe_mismatch,
    randn_premise, wsc_pow2, wsc_random)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from adversarial_spec_amd import ops
else:  # collected but deselected on CPU
    ops = None

DEV = "cuda:0"
GUARD = 256          # poisoned rows on either side of every operand
NAN = float("nan")
F8_NAN = 0x7F


def hip():
    return ops._require_hip()


def guarded(t, fill):
    """t on the GPU, as the interior row-slice of a poisoned parent."""
    if t.dim() == 1:
        return guarded(t[:, None], fill).view(-1)
    parent, _ = guarded_rows(t, fill, GUARD)
    mid = parent.to(DEV)[GUARD:GUARD + t.shape[0]]
    assert mid.is_contiguous() and mid.data_ptr() % 16 == 0
    return mid


@functools.lru_cache(maxsize=None)
def bf16_on_gpu(M, N, K):
    a, b, want, _ = bf16_case(M, N, K)
    return guarded(a, NAN), guarded(b, NAN), want


@functools.lru_cache(maxsize=None)
def probe_on_gpu(M, N, K):
    a, b, perm = probe_case(M, N, K)
    return guarded(a, NAN), guarded(b, NAN), a, perm


@functools.lru_cache(maxsize=None)
def fp8_on_gpu(M, N, K):
    x, codes, e, w, acc, _ = fp8_case(M, N, K)
    return guarded(x, NAN), guarded(e4m3_bytes(w), F8_NAN), e, acc


def assert_exact(got, want, what):
    assert got.dtype == BF16 and got.shape == want.shape
    assert torch.equal(got.cpu(), want), first_mismatch(got, want, what)


def assert_bracket(got, ref64, what):
    msg = bracket_message(got.cpu(), ref64, what)
    assert msg is None, msg


class TestMfmaAnchor:
    def test_integer_inputs_are_exact(self):
        """The premise of every exact test below, on one bare MFMA: integer
        inputs in [-8, 8] give the exact fp32 result."""
        g = torch.Generator().manual_seed(16)
        a = torch.randint(-8, 9, (16, 32), generator=g)
        b = torch.randint(-8, 9, (32, 16), generator=g)
        d = hip().mfma_probe16(a.to(BF16).to(DEV), b.to(BF16).to(DEV))
        assert d.dtype == torch.float32
        assert torch.equal(d.cpu().double(), (a @ b).double())


class TestGemm128:
    @pytest.mark.parametrize("shape", SHAPES_128, ids=str)
    def test_exact(self, shape):
        a, b, want = bf16_on_gpu(*shape)
        assert_exact(hip().gemm_variant(a, b, 128), want, f"gemm128 {shape}")

    @pytest.mark.parametrize("shape", SHAPES_128, ids=str)
    def test_gather_probe(self, shape):
        a, b, a_cpu, perm = probe_on_gpu(*shape)
        msg = probe_mismatch(hip().gemm_variant(a, b, 128), a_cpu, perm)
        assert msg is None, f"gemm128 {shape}: {msg}"


class TestGemm256:
    @pytest.mark.parametrize("shape", SHAPES_256, ids=str)
    def test_exact_and_equal_to_128(self, shape):
        a, b, want = bf16_on_gpu(*shape)
        g256 = hip().gemm_variant(a, b, 256)
        assert_exact(g256, want, f"gemm256 {shape}")
        g128 = hip().gemm_variant(a, b, 128)
        assert torch.equal(g256, g128), first_mismatch(
            g256, g128.cpu(), f"gemm256 vs gemm128 {shape}")

    @pytest.mark.parametrize("shape", SHAPES_256, ids=str)
    def test_gather_probe(self, shape):
        a, b, a_cpu, perm = probe_on_gpu(*shape)
        msg = probe_mismatch(hip().gemm_variant(a, b, 256), a_cpu, perm)
        assert msg is None, f"gemm256 {shape}: {msg}"

    @pytest.mark.parametrize("k", (384, 576))
    def test_refuses_k(self, k):
        a, b, want = bf16_on_gpu(129, 256, k)
        with pytest.raises(RuntimeError, match="gemm256 needs"):
            hip().gemm_variant(a, b, 256)
        assert_exact(hip().gemm_variant(a, b, 128), want, f"after K={k}")


class TestDispatcher:
    @pytest.mark.parametrize("shape", SHAPES_DISPATCH, ids=str)
    def test_gemm(self, shape):
        a, b, want = bf16_on_gpu(*shape)
        got = ops.gemm(a, b)
        assert_exact(got, want, f"gemm {shape}")
        assert torch.equal(got, hip().gemm_variant(a, b, 128))

    @pytest.mark.parametrize("shape", SHAPES_DISPATCH, ids=str)
    def test_gemm_fp8(self, shape):
        M, N, K = shape
        x, w8, e, acc = fp8_on_gpu(M, N, K)
        p2 = wsc_pow2(N)
        got = ops.gemm_fp8(x, w8, guarded(p2, NAN))
        assert_exact(got, fp8_exact_expected(acc, e, p2), f"gemm_fp8 {shape}")


class TestGemmFp8:
    def _run(self, shape):
        M, N, K = shape
        x, w8, e, acc = fp8_on_gpu(M, N, K)
        what = f"gemm_fp8 {shape} ({'256' if dispatch256(*shape) else '128'})"
        p2, rs = wsc_pow2(N), wsc_random(N)
        got = ops.gemm_fp8(x, w8, guarded(p2, NAN))
        assert_exact(got, fp8_exact_expected(acc, e, p2), what + " pow2 wsc")
        got = ops.gemm_fp8(x, w8, guarded(rs, NAN))
        assert_bracket(got, fp8_expected(acc, e, rs), what + " random wsc")

    @pytest.mark.parametrize("shape", SHAPES_128_FP8, ids=str)
    def test_128(self, shape):
        assert not dispatch256(*shape)
        self._run(shape)

    @pytest.mark.parametrize("shape", SHAPES_256_FP8, ids=str)
    def test_256(self, shape):
        assert dispatch256(*shape)
        self._run(shape)

    @pytest.mark.parametrize("shape", SHAPES_FP8_RANDN, ids=str)
    def test_randn_x_from_device_codes(self, shape):
        """The GEMM alone, on whatever the device quantizer makes of a randn
        x: the reference is built from the quant_fp8 binding's own codes and
        scales, so no quantizer rounding enters the comparison."""
        M, N, K = shape
        x_cpu, w = fp8_randn_case(M, N, K)
        x = guarded(x_cpu, NAN)
        q = torch.empty(M, K, dtype=torch.uint8, device=DEV)
        sc = torch.empty(M, dtype=torch.float32, device=DEV)
        hip().quant_fp8(x, q, sc)
        codes = q.cpu().view(F8).double()
        xs = sc.cpu().double()
        assert torch.isfinite(codes).all() and (xs > 0).all()
        assert randn_premise(codes, w) < 2 ** 24, "fp32 accumulation inexact"
        rs = wsc_random(N)
        ref64 = (codes @ w.double().t()) * xs[:, None] * rs.double()[None, :]
        got = ops.gemm_fp8(x, guarded(e4m3_bytes(w), F8_NAN),
                           guarded(rs, NAN))
        assert_bracket(got, ref64, f"gemm_fp8 randn {shape}")


class TestRefusals:
    """Every refusal is followed by a valid call on the same operands' kernel,
    which must still be exact: nothing was launched, nothing is left over."""

    SHAPE = (17, 15, 72)
    SHAPE8 = (17, 15, 80)

    def _ok(self):
        a, b, want = bf16_on_gpu(*self.SHAPE)
        assert_exact(ops.gemm(a, b), want, "gemm after a refusal")
        assert_exact(hip().gemm_variant(a, b, 128), want,
                     "gemm_variant after a refusal")

    def _ok8(self):
        M, N, K = self.SHAPE8
        x, w8, e, acc = fp8_on_gpu(M, N, K)
        p2 = wsc_pow2(N)
        assert_exact(ops.gemm_fp8(x, w8, p2.to(DEV)),
                     fp8_exact_expected(acc, e, p2), "gemm_fp8 after a refusal")

    @pytest.mark.parametrize("fn", ("gemm", "variant128", "variant256"))
    def test_bf16_operands(self, fn):
        call = {"gemm": lambda a, b: hip().gemm(a, b),
                "variant128": lambda a, b: hip().gemm_variant(a, b, 128),
                "variant256": lambda a, b: hip().gemm_variant(a, b, 256)}[fn]
        k = 512
        a = torch.ones(4, k, dtype=BF16, device=DEV)
        b = torch.ones(6, k, dtype=BF16, device=DEV)
        bad = [
            (a[:, :12], b[:, :12]),              # K % 8 != 0
            (a[:, :4], b[:, :4]),
            (a[:, :508], b[:, :508]),
            (a, b[:, :504]),                     # K mismatch
            (a[0], b),                           # 1-D
            (a, b[0]),
            (a[None], b),                        # 3-D
            (a, b[None]),
            (a.cpu(), b), (a, b.cpu()),          # not on the GPU
            (a.float(), b), (a, b.float()),      # not bf16
        ]
        for x, w in bad:
            with pytest.raises(RuntimeError):
                call(x, w)
        assert call(a, b).shape == (4, 6)
        self._ok()

    @pytest.mark.parametrize("which", (0, 64, 127, 129, 255, 512, -128))
    def test_variant_which(self, which):
        a, b, _ = bf16_on_gpu(129, 256, 640)
        with pytest.raises(RuntimeError, match="128 or 256"):
            hip().gemm_variant(a, b, which)
        self._ok()

    def test_fp8_operands(self):
        M, N, K = self.SHAPE8
        x, w8, e, acc = fp8_on_gpu(M, N, K)
        wsc = wsc_pow2(N).to(DEV)
        wide = torch.full((N, 2 * K), 0x38, dtype=torch.uint8, device=DEV)
        twice = torch.ones(2 * N, dtype=torch.float32, device=DEV)
        bad = [
            (x[:, :24], w8[:, :24].contiguous(), wsc),    # K % 16 != 0
            (x[:, :8], w8[:, :8].contiguous(), wsc),
            (x[:, :72], w8[:, :72].contiguous(), wsc),
            (x[:, :64], w8, wsc),                         # K mismatch
            (x[0], w8, wsc),                              # x not 2-D
            (x[None], w8, wsc),
            (x.cpu(), w8, wsc),                           # x not on the GPU
            (x.float(), w8, wsc),                         # x not bf16
            (x, w8.cpu(), wsc),                           # w8 not on the GPU
            (x, w8.reshape(-1), wsc),                     # w8 not 2-D
            (x, w8[None], wsc),
            (x, wide[:, :K], wsc),                        # w8 not contiguous
            (x, w8.view(torch.int8), wsc),                # w8 not uint8
            (x, w8, wsc.cpu()),                           # wsc not on the GPU
            (x, w8, wsc.double()),                        # wsc not f32
            (x, w8, wsc.to(BF16)),
            (x, w8, twice[::2]),                          # wsc not contiguous
            (x, w8, wsc[:N - 1]),                         # wsc too short
        ]
        for args in bad:
            with pytest.raises(RuntimeError):
                hip().gemm_fp8(*args)
        self._ok8()
