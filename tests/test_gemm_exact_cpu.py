"""CPU checks of tests/gemm_exact_common.py: the premises and the coverage
claims the exact GPU tests of the prefill GEMMs (test_gemm_exact_gpu.py)
stand on.

  - the generated inputs make fp32 accumulation exact (every partial sum an
    integer below 2^24), the fp8 activations quantize to the intended codes
    with a row scale of exactly 2^e, and the references agree with a float64
    matmul;
  - the shape lists reach every staging path: all eight (a_edge, b_edge,
    k_edge) triples and 1, 2 and 3 K-tiles of the 128^2 kernels, every tail
    and clamp case of the 256^2 kernels, and both sides of every clause of
    the dispatch rule.
"""

import itertools

import pytest
import torch

from gemm_exact_common import (
    BF16, E_CYCLE, EDGES, F8, KS_128, KS_128_FP8, SHAPES_128, SHAPES_128_FP8,
    SHAPES_256, SHAPES_256_FP8, SHAPES_256_FP8_TO_128, SHAPES_DISPATCH,
    SHAPES_FP8_RANDN, bf16_bracket, bf16_case, bracket_message, dispatch256,
    e4m3_bytes, first_mismatch, fp8_case, fp8_exact_expected, fp8_expected,
    fp8_randn_case, guarded_rows, paths128, paths256, probe_case,
    probe_expected, probe_mismatch, randn_premise, wsc_pow2, wsc_random)

ALL_BF16 = tuple(dict.fromkeys(SHAPES_128 + SHAPES_256 + SHAPES_DISPATCH))
ALL_FP8 = tuple(dict.fromkeys(
    SHAPES_128_FP8 + SHAPES_256_FP8 + SHAPES_DISPATCH))
ALL_TRIPLES = set(itertools.product((False, True), repeat=3))


def rule(M, N, K):
    """The dispatch rule of gemm() and gemm_fp8(), written out."""
    return M > 128 and N >= 256 and K >= 512 and K % 128 == 0


class TestExactInputs:
    @pytest.mark.parametrize("shape", ALL_BF16, ids=str)
    def test_bf16_partial_sums_and_reference(self, shape):
        a, b, want, bound = bf16_case(*shape)
        assert a.dtype == BF16 and b.dtype == BF16 and want.dtype == BF16
        assert a.abs().max() <= 8 and b.abs().max() <= 8
        assert bound < 2 ** 24
        ref64 = a.double() @ b.double().t()
        assert ref64.abs().max() <= bound
        assert torch.equal(ref64.float().to(BF16), want)
        # one rounding of an exact value: it is a neighbour of the fp64 result
        assert bracket_message(want, ref64, "bf16 reference") is None
        # fp32 accumulation is exact whatever the order
        assert torch.equal((a.float() @ b.float().t()).double(), ref64)

    @pytest.mark.parametrize("shape", ALL_FP8, ids=str)
    def test_fp8_rows_quantize_exactly(self, shape):
        M, N, K = shape
        x, codes, e, w, acc, bound = fp8_case(M, N, K)
        assert bound < 2 ** 24
        assert set(e.tolist()) <= set(E_CYCLE)
        assert M < 3 or set(e.tolist()) == set(E_CYCLE)
        # exactly one +-448 per row; every other code a small integer
        big = codes.abs() == 448
        assert torch.equal(big.sum(dim=1), torch.ones(M, dtype=torch.int64))
        assert codes.abs()[~big].max() <= 8
        # the fp32 row scale amax / 448 is exactly 2^e, and so is its inverse
        amax = x.float().abs().amax(dim=1)
        s = amax / torch.tensor(448.0)
        assert s.dtype == torch.float32
        assert torch.equal(s.double(), torch.pow(2.0, e.double()))
        inv = 1.0 / s
        assert torch.equal(inv.double(), torch.pow(2.0, -e.double()))
        # x * inv lies on the e4m3 grid and survives the cast unchanged
        q = x.float() * inv[:, None]
        assert torch.equal(q.to(F8).double(), codes.double())
        assert torch.equal(e4m3_bytes(q).view(F8).double(), codes.double())
        assert w.abs().max() <= 8
        assert torch.equal(e4m3_bytes(w).view(F8).double(), w.double())

    @pytest.mark.parametrize("shape", ALL_FP8, ids=str)
    def test_fp8_references_agree_with_float64(self, shape):
        M, N, K = shape
        x, codes, e, w, acc, bound = fp8_case(M, N, K)
        ref64 = codes.double() @ w.double().t()
        assert torch.equal(acc.double(), ref64)
        # dequantized operands, float64 matmul: the same value
        p2 = wsc_pow2(N)
        assert set(p2.tolist()) <= {0.25, 0.5, 1.0, 2.0, 4.0}
        deq = x.double() @ (w.double() * p2.double()[:, None]).t()
        assert torch.equal(fp8_expected(acc, e, p2), deq)
        want = fp8_exact_expected(acc, e, p2)
        assert bracket_message(want, deq, "fp8 reference") is None
        # the two fp32 products of the epilogue are exact for these scales
        xs = torch.pow(2.0, e.double()).float()
        epi = acc.float() * xs[:, None] * p2[None, :]
        assert torch.equal(epi.to(BF16), want)
        # random scales: the fp32 epilogue stays inside the bracket
        rs = wsc_random(N)
        assert rs.min() >= 0.5 and rs.max() < 2.0
        epi = (acc.float() * xs[:, None] * rs[None, :]).to(BF16)
        assert bracket_message(epi, fp8_expected(acc, e, rs), "random wsc") \
            is None

    @pytest.mark.parametrize("shape", SHAPES_FP8_RANDN, ids=str)
    def test_randn_codes_accumulate_exactly(self, shape):
        M, N, K = shape
        x, w = fp8_randn_case(M, N, K)
        assert w.abs().max() == 1
        xf = x.float()
        s = xf.abs().amax(dim=1) / 448.0
        codes = (xf * (1.0 / s)[:, None]).to(F8).double()
        # a factor of two in hand for whichever neighbouring codes the
        # device quantizer picks
        assert randn_premise(codes, w) < 2 ** 23
        ref64 = codes @ w.double().t()
        assert torch.equal((codes.float() @ w.float().t()).double(), ref64)


class TestProbe:
    @pytest.mark.parametrize("shape", ((17, 15, 72), (145, 145, 136),
                                       (300, 129, 640), (1, 1, 512)), ids=str)
    def test_gather(self, shape):
        M, N, K = shape
        a, b, perm = probe_case(M, N, K)
        assert sorted(perm.tolist()) == list(range(K))
        assert a.abs().max() <= 128
        assert torch.equal(b.sum(dim=1), torch.ones(N, dtype=BF16))
        c = (a.double() @ b.double().t()).to(BF16)
        assert torch.equal(c, probe_expected(a, perm, N))
        assert probe_mismatch(c, a, perm) is None
        if N >= K:       # every k is selected by some output column
            assert set(perm[torch.arange(N) % K].tolist()) == set(range(K))

    def test_columns_are_distinguishable(self):
        a, _, _ = probe_case(300, 129, 640)
        cols = {tuple(a[:, k].tolist()) for k in range(640)}
        assert len(cols) == 640

    def test_message_names_both_columns(self):
        a, b, perm = probe_case(17, 15, 72)
        c = probe_expected(a, perm, 15).clone()
        other = (int(perm[4]) + 9) % 72
        c[:, 4] = a[:, other]
        msg = probe_mismatch(c, a, perm)
        assert "(m, n) = (0, 4)" in msg
        assert f"expected A[0, {int(perm[4])}]" in msg
        assert f"holds column k={other} of A" in msg
        c = probe_expected(a, perm, 15).clone()
        c[3, 2] = 300.0
        assert "no single k" in probe_mismatch(c, a, perm)

    def test_first_mismatch_message(self):
        a, b, want, _ = bf16_case(17, 15, 72)
        got = want.clone()
        got[5, 7] += 1
        assert "(m, n) = (5, 7)" in first_mismatch(got, want, "x")

    def test_guarded_rows(self):
        a, _, _, _ = bf16_case(17, 15, 72)
        parent, mid = guarded_rows(a, float("nan"), 128)
        assert mid.is_contiguous() and torch.equal(mid, a)
        assert mid.data_ptr() % 16 == parent.data_ptr() % 16
        assert torch.isnan(parent[:128].float()).all()
        assert torch.isnan(parent[128 + 17:].float()).all()


class TestCoverage128:
    @pytest.mark.parametrize("shapes,ks", ((SHAPES_128, KS_128),
                                           (SHAPES_128_FP8, KS_128_FP8)),
                             ids=("bf16", "fp8"))
    def test_every_path_and_tile_count(self, shapes, ks):
        triples, ntiles = set(), {}
        for s in shapes:
            t, n = paths128(*s)
            triples |= t
            ntiles.setdefault(n, s)
        assert triples == ALL_TRIPLES
        assert {1, 2, 3} <= set(ntiles)
        assert {s[0] for s in shapes} >= set(EDGES)
        assert {s[1] for s in shapes} >= set(EDGES)
        assert {s[2] for s in shapes} >= set(ks)

    def test_paths_of_known_shapes(self):
        assert paths128(128, 128, 64) == ({(False, False, False)}, 1)
        assert paths128(1, 1, 8) == ({(True, True, True)}, 1)
        assert paths128(128, 128, 72) == (
            {(False, False, False), (False, False, True)}, 2)
        # an interior block and the three kinds of edge block in one grid
        assert paths128(145, 145, 136) == (ALL_TRIPLES, 3)
        assert paths128(128, 1, 136)[0] == {(False, True, False),
                                            (False, True, True)}
        assert paths128(1, 128, 64)[0] == {(True, False, False)}

    def test_fp8_k_values_are_legal(self):
        for M, N, K in SHAPES_128_FP8 + SHAPES_256_FP8 + SHAPES_DISPATCH:
            assert K % 16 == 0
        for M, N, K in SHAPES_128 + SHAPES_256 + SHAPES_DISPATCH:
            assert K % 8 == 0

    def test_fp8_list_stays_on_the_128_kernel(self):
        for s in SHAPES_128_FP8:
            assert not rule(*s), s
        # a grid of more than one block, full tiles only
        assert (256, 128, 576) in SHAPES_128_FP8
        assert paths128(256, 128, 576) == ({(False, False, False)}, 9)


class TestCoverage256:
    def test_every_case_is_named(self):
        p = {s: paths256(*s) for s in SHAPES_256}
        assert p[(256, 256, 512)] == dict(nt=8, m_clamp=False, n_clamp=False,
                                          a_half=False, b_half=False)
        assert p[(257, 256, 640)]["nt"] == 10
        assert p[(385, 511, 1024)]["nt"] == 16
        # M clamp without a fully clamped half-image, and with one
        assert p[(129, 300, 512)]["m_clamp"] and not p[(129, 300, 512)]["a_half"]
        assert p[(257, 256, 640)]["a_half"] and not p[(257, 256, 640)]["n_clamp"]
        assert p[(300, 129, 640)]["n_clamp"] and not p[(300, 129, 640)]["b_half"]
        assert p[(256, 257, 512)]["b_half"] and not p[(256, 257, 512)]["m_clamp"]
        assert p[(1, 1, 512)]["a_half"] and p[(1, 1, 512)]["b_half"]
        for case in ("m_clamp", "n_clamp", "a_half", "b_half"):
            assert any(v[case] for v in p.values()), case
        assert {8, 10} <= {v["nt"] for v in p.values()}

    def test_fp8_sublist(self):
        """gemm_fp8() sends these two to its 128^2 kernel, the rest to the
        256^2 one, and every 256^2 case survives in the rest."""
        assert SHAPES_256_FP8_TO_128 == ((300, 129, 640), (1, 1, 512))
        assert [s for s in SHAPES_256 if rule(*s)] == list(SHAPES_256_FP8)
        assert len(SHAPES_256_FP8) == 5
        p = [paths256(*s) for s in SHAPES_256_FP8]
        for case in ("m_clamp", "n_clamp", "a_half", "b_half"):
            assert any(v[case] for v in p), case
        assert {8, 10} <= {v["nt"] for v in p}


class TestDispatchBoundaries:
    def test_helper_is_the_rule(self):
        for s in SHAPES_128 + SHAPES_256 + SHAPES_DISPATCH + SHAPES_128_FP8:
            assert dispatch256(*s) == rule(*s)

    def test_one_shape_on_each_side_of_every_clause(self):
        on = {s: rule(*s) for s in SHAPES_DISPATCH}
        assert on == {
            (128, 256, 512): False,    # M > 128 fails by one
            (129, 256, 512): True,     # every clause at its boundary
            (129, 255, 512): False,    # N >= 256 fails by one
            (129, 256, 384): False,    # K >= 512 fails, K % 128 == 0 holds
            (129, 256, 576): False,    # K % 128 == 0 fails, K >= 512 holds
            (129, 256, 640): True,     # the next K that passes
        }
        # each rejected shape differs from an accepted one in one clause only
        clauses = lambda M, N, K: (M > 128, N >= 256, K >= 512, K % 128 == 0)
        for s, ok in on.items():
            assert sum(not c for c in clauses(*s)) == (0 if ok else 1)
        failing = {clauses(*s).index(False) for s, ok in on.items() if not ok}
        assert failing == {0, 1, 2, 3}


class TestBracket:
    def test_neighbours(self):
        v = torch.tensor([1.0, 1.0 + 2.0 ** -9, -3.0 - 2.0 ** -8, 0.0],
                         dtype=torch.float64)
        lo, hi = bf16_bracket(v)
        assert lo.tolist() == [1.0, 1.0, -3.015625, 0.0]
        assert hi.tolist()[:3] == [1.0, 1.0078125, -3.0]
