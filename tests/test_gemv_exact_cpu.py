"""CPU checks of tests/gemv_exact_common.py: the premises the exact GPU tests
of the decode GEMVs (test_gemv_exact_gpu.py) stand on.

  - the (L, U, E) table gives K values that really split the lanes of a row
    the way each case is named, under the kernels' own loop inequalities;
  - the generated inputs make fp32 arithmetic exact: every partial sum stays
    below 2^24 and the fp32 and fp64 CPU results agree bit for bit;
  - bf16_bracket and e4m3_bracket return the true neighbours.
"""

import pytest
import torch

from gemv_exact_common import (
    BF16, BRACKET_OPS, EXACT_OPS, K_LABELS, KERNELS, N_TAILS, OPS,
    SWITCHING_OPS, bf16_bracket, bf16_step, bracket_violations, dense_case,
    e4m3_bracket, e4m3_grid, fold_negative_zero, fp8_norm_probe, head_rows,
    is_fp8, is_gateup, is_norm, k_cases, lane_trips, materialize, probe_case,
    quantizer_row, reference, rope_geometry)

ALL_OPS = tuple(OPS)


class TestLaneSplit:
    def test_w32_bf16_k_values(self):
        """The table's example column: 32 lanes, 8-deep, 8 per chunk."""
        assert list(k_cases("gemv_kernel_w32").values()) == [
            8, 264, 1920, 2048, 2056, 4360]
        # the tensor-parallel shard of the issue, 28672 / 8 = 3584 = 448 * 8
        trips = lane_trips(448, 32, 8)
        assert {t[0] for t in trips} == {1} and {t[1] for t in trips} == {6}

    @pytest.mark.parametrize("kernel", sorted(KERNELS))
    def test_each_k_gives_its_split(self, kernel):
        L, U, E = KERNELS[kernel]
        ks = k_cases(kernel)
        assert tuple(ks) == K_LABELS
        split = {}
        for label, K in ks.items():
            assert K % E == 0
            nc = K // E
            trips = lane_trips(nc, L, U)
            # every chunk of the row is read by exactly one lane, once
            assert sorted(c for t in trips for c in t[2]) == list(range(nc))
            split[label] = [(m, r) for m, r, _ in trips]
        idle = [(0, 0)] * (L - 1)
        assert split["one_lane"] == [(0, 1)] + idle
        assert split["rem_only"] == [(0, 2)] + [(0, 1)] * (L - 1)
        assert split["half_unrolled"] == (
            [(1, 0)] * (L // 2) + [(0, U - 1)] * (L // 2))
        assert split["unrolled_only"] == [(1, 0)] * L
        assert split["unrolled_plus_one"] == [(1, 1)] + [(1, 0)] * (L - 1)
        assert split["both_loops"] == [(2, 2)] + [(2, 1)] * (L - 1)

    def test_every_op_names_known_kernels(self):
        for op, (w32, w16) in OPS.items():
            assert KERNELS[w32][0] == 32
            assert w16 is None or KERNELS[w16][0] == 16
            assert (w16 is not None) == (op in SWITCHING_OPS + ("gemv_fp8",))
            assert KERNELS[w32][2] == (16 if is_fp8(op) else 8)
        assert set(EXACT_OPS) | set(BRACKET_OPS) == set(OPS)
        # the fp8 qkv + RoPE kernel has no case of its own: the fusion test
        # pins it to gemv_fp8_q, whose loop it shares
        assert (KERNELS["gemv_fp8_rope_kv_w32_kernel"]
                == KERNELS["gemv_fp8_kernel_w32"])


class TestBf16Bracket:
    def _b(self, vals):
        lo, hi = bf16_bracket(torch.tensor(vals, dtype=torch.float64))
        return lo.double().tolist(), hi.double().tolist()

    def test_representable_values_bracket_themselves(self):
        vals = [1.0, 1.0078125, 448.0, 2.0 ** 127, 2.0 ** -133, -2.0 ** -126,
                -1.5, 65280.0]
        lo, hi = self._b(vals)
        assert lo == vals and hi == vals

    def test_zero(self):
        lo, hi = self._b([0.0, -0.0])
        assert lo == [0.0, 0.0] and hi == [0.0, 0.0]
        # the neighbours of a value just off zero are zero and the smallest
        # subnormal, on either side
        lo, hi = self._b([1e-60, -1e-60])
        assert lo == [0.0, -2.0 ** -133] and hi == [2.0 ** -133, 0.0]

    def test_midpoints_and_near_grid(self):
        step = 2.0 ** -7                      # bf16 spacing in [1, 2)
        lo, hi = self._b([1 + step / 2, 1 + 3 * step / 2, 1 + 1e-12,
                          1 + step - 1e-12])
        assert lo == [1.0, 1 + step, 1.0, 1.0]
        assert hi == [1 + step, 1 + 2 * step, 1 + step, 1 + step]
        # across a binade: below 2 the step is 2^-7, above it 2^-6
        lo, hi = self._b([2 - 1e-9, 2 + 1e-9])
        assert lo == [2 - step, 2.0] and hi == [2.0, 2 + 2 * step]

    def test_negative_values(self):
        step = 2.0 ** -7
        lo, hi = self._b([-(1 + step / 2), -1 - 1e-12, -1 + 1e-12])
        assert lo == [-(1 + step), -(1 + step), -1.0]
        assert hi == [-1.0, -1.0, -(1 - step / 2)]

    def test_random_values_are_bracketed_by_neighbours(self):
        g = torch.Generator().manual_seed(5)
        v = torch.randn(4096, generator=g, dtype=torch.float64) * \
            torch.pow(2.0, torch.randint(-20, 20, (4096,), generator=g))
        lo, hi = bf16_bracket(v)
        lo, hi = lo.double(), hi.double()
        assert ((lo <= v) & (v <= hi) & (lo < hi)).all()
        assert torch.equal(hi - lo, bf16_step(v))

    def test_violations(self):
        ref = torch.tensor([1.0, 1.004, 0.0, 1.004], dtype=torch.float64)
        got = torch.tensor([1.0078125, 1.0078125, -0.0, 1.015625]).to(BF16)
        # exact 1.0 must be hit; 1.004 lies in (1, 1.0078125); -0 == 0
        assert bracket_violations(got, ref).tolist() == [0, 3]


class TestE4m3:
    def test_grid_and_bracket(self):
        grid = e4m3_grid()
        assert grid.numel() == 253 and grid[-1] == 448 and grid[0] == -448
        v = torch.tensor([0.0147, 0.015625, 447.0, -0.001, 17.0, 448.0],
                         dtype=torch.float64)
        lo, hi = e4m3_bracket(v)
        assert lo.tolist() == [0.013671875, 0.015625, 416.0, -2.0 ** -9,
                               16.0, 448.0]
        assert hi.tolist() == [0.015625, 0.015625, 448.0, 0.0, 18.0, 448.0]

    def test_quantizer_row(self):
        row = quantizer_row()
        assert row.numel() % 8 == 0 and row.numel() == 34760
        assert row.float().abs().max() == 448
        assert torch.unique(row.view(torch.int16)).numel() == 2 * 17377
        codes = row.float().to(torch.float8_e4m3fn).view(torch.uint8)
        assert (fold_negative_zero(codes) != 0x80).all()
        assert torch.isfinite(codes.view(torch.float8_e4m3fn).float()).all()


def _ns(op):
    if op == "gemv_norm_rope_kv":
        return (48, 96)
    return N_TAILS


class TestExactPremise:
    """Every partial sum below 2^24, fp32 == fp64."""

    def _check(self, c):
        materialize(c)        # asserts every operand exact in its wire dtype
        y64, bound, d64 = reference(c, torch.float64)
        y32, _, d32 = reference(c, torch.float32)
        assert bound < 2 ** 24, (c.op, c.K, c.N, bound)
        assert torch.equal(d32.double(), d64), (c.op, c.K, c.N)
        if c.op in EXACT_OPS:
            assert torch.equal(y32.double(), y64), (c.op, c.K, c.N)
        else:
            torch.testing.assert_close(y32.double(), y64, rtol=1e-5, atol=0)
        if is_gateup(c.op):
            gate = reference(c, pre_activation=True)[0]
            assert gate.abs().max() <= 64
        return y64

    @pytest.mark.parametrize("op", ALL_OPS)
    def test_dense_cases(self, op):
        for K in k_cases(OPS[op][0]).values():
            for N in _ns(op):
                for j in ((-3, 2) if is_fp8(op) else (0,)):
                    self._check(dense_case(op, K, N, j=j))

    @pytest.mark.parametrize("op", SWITCHING_OPS)
    def test_dense_case_16_lane(self, op):
        K = k_cases(OPS[op][1])["both_loops"]
        c = dense_case(op, K, 8200, j=-3)
        y = self._check(c)
        assert torch.equal(self._check(head_rows(c, 8193)), y[:8193])

    def test_scale_of_a_self_quantizing_case_is_a_power_of_two(self):
        for j in (-3, 2):
            c = dense_case("gemv_fp8", 528, 9, j=j)
            x = materialize(c)["x"].float()
            assert x.abs().max() / 448.0 == 2.0 ** j
            codes = (x / 2.0 ** j).to(torch.float8_e4m3fn).float()
            assert torch.equal(codes, x / 2.0 ** j)

    def test_a_dropped_chunk_changes_the_result(self):
        """Sensitivity: zeroing one 8-element chunk of x moves nearly every
        output of an exact case off its reference."""
        c = dense_case("gemv", 264, 17)
        want = reference(c)[0].float().to(BF16)
        c.x[256:264] = 0
        got = reference(c)[0].float().to(BF16)
        assert (got != want).float().mean() > 0.8


class TestProbe:
    @pytest.mark.parametrize("op", ALL_OPS)
    def test_every_column_is_selected_once_per_k_rows(self, op):
        for label in ("rem_only", "unrolled_plus_one"):
            K = k_cases(OPS[op][0])[label]
            N = rope_geometry(K)[3] if op == "gemv_norm_rope_kv" else K + 1
            c = probe_case(op, K, N)
            materialize(c)
            assert sorted(c.cols[:K].tolist()) == list(range(K))
            assert (c.w.sum(1) == 1).all() and (c.w.max(1).values == 1).all()
            # consecutive rows select different chunks
            E = KERNELS[OPS[op][0]][2]
            assert (c.cols[1:] // E != c.cols[:-1] // E).all()
            if is_fp8(op) and is_norm(op):
                lo, hi, s = fp8_norm_probe(c)
                v = c.x * c.wln * 448.0 / (c.x * c.wln).abs().max()
                assert ((lo <= v) & (v <= hi)).all() and s > 0
                # both the on-grid and the bracketed decision occur
                assert (lo == hi).any() and (lo < hi).any()
            else:
                y = reference(c)[0]
                if not is_gateup(op) and not is_norm(op):
                    # the output names the element it read
                    sc = 1.0 if c.wsc is None else c.wsc.double()
                    r = 0.0 if c.resid is None else c.resid
                    assert torch.equal(y, c.x[c.cols] * sc + r)

    def test_rope_geometry(self):
        assert rope_geometry(1) == (1, 1, 16, 48)
        assert rope_geometry(264) == (15, 1, 16, 272)
        assert rope_geometry(2056) == (127, 1, 16, 2064)
