"""Decode/prefill attention edge cases vs a float64 reference.

tests/test_ops_gpu.py walks one 64-position tile per decode block and only
`kv_offset == 0` prefill. This module drives the paths the engine really
takes: multi-tile splits (counted DMA wait, buffer restage, cross-tile
online-softmax rescale), the split/combine walk at ragged split counts, odd
GQA groups, other page sizes, the identity-table template, the graph-mode
device-position entry, chunked prefill offsets, non-causal prefill and the
deferred-max softmax branch.

The reference (`ref_attention`, `ref_decode`) is plain float64 softmax
attention over the same bf16-rounded inputs, output unrounded; it is checked
on its own by tests/test_attention_reference_cpu.py. Tolerances are the
project's existing ones (decode atol=rtol=2e-2, prefill atol=2.5e-2
rtol=2e-2), compared elementwise with zero elements out of bound.

Every decode test asserts the launch geometry it claims to exercise through
`_advspec_hip.decode_split_geometry` (the binding over the launcher's own
`split_geometry`), so a later tuning change cannot silently turn these
cases back into single-tile ones.
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
KH = 2
DTILE = 64  # positions per staged decode tile (attention.hip)

DECODE_TOL = dict(atol=2e-2, rtol=2e-2)
PREFILL_TOL = dict(atol=2.5e-2, rtol=2e-2)


def _bf(x):
    return x.to(torch.bfloat16)


# ---------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------

def ref_attention(q, k, v, scale=None, causal=True, kv_offset=0):
    """Softmax attention in float64. q [tq, hq, hd]; k, v [tk, kh, hd];
    query row i sits at absolute position kv_offset + i and, when causal,
    sees keys 0..kv_offset+i. Returns float64 [tq, hq, hd], unrounded."""
    tq, hq, hd = q.shape
    tk, kh, _ = k.shape
    if scale is None:
        scale = 1.0 / math.sqrt(hd)
    group = hq // kh
    qd = q.double().cpu()
    kd = k.double().cpu().repeat_interleave(group, dim=1)  # [tk, hq, hd]
    vd = v.double().cpu().repeat_interleave(group, dim=1)
    s = torch.einsum("qhd,khd->hqk", qd, kd) * scale
    if causal:
        qpos = torch.arange(tq).unsqueeze(1) + kv_offset
        kpos = torch.arange(tk).unsqueeze(0)
        s = s.masked_fill((kpos > qpos).unsqueeze(0), float("-inf"))
    s = s - s.amax(dim=-1, keepdim=True)
    p = s.exp()
    p = p / p.sum(dim=-1, keepdim=True)
    return torch.einsum("hqk,khd->qhd", p, vd)


def ref_decode(q, kc, vc, table, seq_len, scale=None):
    """Paged single-token decode in float64. q [hq, hd]; kc, vc
    [n_pages, page, kh, hd]; attends logical positions [0, seq_len)."""
    page = kc.shape[1]
    n_used = (seq_len + page - 1) // page
    phys = table.cpu()[:n_used].long()
    k = kc.cpu()[phys].reshape(n_used * page, *kc.shape[2:])[:seq_len]
    v = vc.cpu()[phys].reshape(n_used * page, *vc.shape[2:])[:seq_len]
    return ref_attention(q.cpu().unsqueeze(0), k, v, scale, causal=False)[0]


def _assert_within(got, want, atol, rtol, name):
    """Same form as test_ops_gpu._assert_close: elementwise, zero elements
    out of bound; the figures are printed before asserting."""
    g = got.double().cpu()
    w = want.double().cpu()
    assert g.shape == w.shape, f"{name}: shape {g.shape} vs {w.shape}"
    assert torch.isfinite(g).all(), f"{name}: non-finite output"
    err = (g - w).abs()
    bound = atol + rtol * w.abs()
    n_bad = int((err > bound).sum())
    print(f"{name}: max err {err.max():.4g}, worst err/bound "
          f"{(err / bound).max():.3f}")
    assert n_bad == 0, (
        f"{name}: max err {err.max():.4g}; {n_bad}/{err.numel()} out of tol"
    )


# ---------------------------------------------------------------------------
# decode helpers
# ---------------------------------------------------------------------------

def _tiles(seq, n_splits, split_len):
    """64-position tiles each split block walks for a true length `seq`."""
    return [
        max(0, -(-(min(seq, (i + 1) * split_len) - i * split_len) // DTILE))
        for i in range(n_splits)
    ]


def _check_geometry(seq, split_blocks, want_tiles, bound=None):
    """Assert the launch geometry of a decode call: `want_tiles` lists the
    tiles per split. `bound` is the length that sizes the grid (graph mode:
    max_seq); the tiles are those of the true length `seq`."""
    ns, sl = _hip.decode_split_geometry(bound or seq, KH, split_blocks)
    got = _tiles(seq, ns, sl)
    env = os.environ.get("ADVSPEC_SPLIT_BLOCKS")
    assert env is None and got == list(want_tiles), (
        f"decode geometry for seq={seq} bound={bound} split_blocks="
        f"{split_blocks}: {ns} splits x split_len {sl} -> tiles {got}, "
        f"this case needs {list(want_tiles)}. ADVSPEC_SPLIT_BLOCKS={env!r} "
        "overrides the per-call block target and must be unset for these "
        "tests."
    )
    return ns, sl


@functools.lru_cache(maxsize=None)
def _decode_inputs(seq, hd, group, page=64, identity=False, nan_fill=False,
                   cover=0):
    """CPU inputs for one decode case, built once and shared: (q, kc, vc,
    table). `cover` >= seq is the number of positions the cache must hold
    (graph mode sizes its grid by max_seq). With `nan_fill`, every cache
    position >= seq and every physical page the table does not reach holds
    NaN."""
    gen = torch.Generator().manual_seed(
        seq * 100003 + hd * 1009 + group * 101 + page * 7 + cover)
    n_used = (max(seq, cover) + page - 1) // page
    npg = n_used + 2
    if identity:
        table = torch.arange(npg, dtype=torch.int32)
    else:
        table = torch.randperm(npg, generator=gen).to(torch.int32)
    q = _bf(torch.randn(KH * group, hd, generator=gen))
    caches = []
    for _ in range(2):
        logical = torch.randn(n_used * page, KH, hd, generator=gen)
        if nan_fill:
            logical[seq:] = float("nan")
            c = torch.full((npg, page, KH, hd), float("nan"))
        else:
            c = torch.randn(npg, page, KH, hd, generator=gen)
        c[table[:n_used].long()] = logical.view(n_used, page, KH, hd)
        caches.append(_bf(c))
    return q, caches[0], caches[1], table


def _dev(*ts):
    return tuple(t.to(DEV) for t in ts)


def _pos_state(pos):
    return torch.tensor([pos], dtype=torch.int32, device=DEV)


HD_GROUP = [(128, 4), (64, 8), (32, 2)]


class TestDecodeMultiTile:
    # A: one split walking ceil(seq/64) tiles, output written directly by
    # the split kernel (no combine). 3+ tiles restage a consumed buffer.
    @pytest.mark.parametrize("seq,tiles", [(64, 1), (65, 2), (128, 2),
                                           (129, 3), (193, 4), (577, 10)])
    @pytest.mark.parametrize("hd,group", HD_GROUP)
    def test_single_split(self, seq, tiles, hd, group):
        _check_geometry(seq, 2, [tiles])
        cpu = _decode_inputs(seq, hd, group)
        q, kc, vc, table = _dev(*cpu)
        got = ops.attn_decode_paged(q, kc, vc, table, seq, split_blocks=2)
        _assert_within(got, ref_decode(*cpu, seq), **DECODE_TOL,
                       name=f"decode A s={seq} hd={hd} g={group}")

    # B: two multi-tile splits merged by the combine kernel.
    @pytest.mark.parametrize("seq,tiles", [(300, [3, 2]), (700, [6, 5])])
    @pytest.mark.parametrize("hd,group", [(128, 4), (64, 8)])
    def test_two_splits_combine(self, seq, tiles, hd, group):
        _check_geometry(seq, 4, tiles)
        cpu = _decode_inputs(seq, hd, group)
        q, kc, vc, table = _dev(*cpu)
        got = ops.attn_decode_paged(q, kc, vc, table, seq, split_blocks=4)
        _assert_within(got, ref_decode(*cpu, seq), **DECODE_TOL,
                       name=f"decode B s={seq} hd={hd}")

    # C: combine walk — 4 waves stride the splits 16 at a time, then a
    # ragged remainder; hd=128 uses both blockIdx.y halves, hd=32 the
    # dd >= hd early return.
    @pytest.mark.parametrize("n", [2, 3, 5, 13, 17, 29, 54])
    @pytest.mark.parametrize("hd,group", [(128, 4), (32, 2)])
    def test_combine_walk(self, n, hd, group):
        seq = 64 * n - 5
        ns, _ = _check_geometry(seq, 0, [1] * n)
        assert ns == n
        cpu = _decode_inputs(seq, hd, group)
        q, kc, vc, table = _dev(*cpu)
        got = ops.attn_decode_paged(q, kc, vc, table, seq)
        _assert_within(got, ref_decode(*cpu, seq), **DECODE_TOL,
                       name=f"decode C n_splits={n} hd={hd}")


class TestDecodeGroups:
    # D: GQA groups other than 2/4/8 — the kernel template rounds the
    # group up, idle waves skip, and the q image load clamps its last
    # piece.
    CASES = [(128, 1), (128, 3), (128, 5), (128, 6), (128, 7),
             (32, 1), (32, 3)]
    SEQ = 200

    @pytest.mark.parametrize("split_blocks,tiles", [(2, [4]), (0, [1] * 4)])
    @pytest.mark.parametrize("hd,group", CASES)
    def test_vs_ref(self, hd, group, split_blocks, tiles):
        seq = self.SEQ
        _check_geometry(seq, split_blocks, tiles)
        cpu = _decode_inputs(seq, hd, group)
        q, kc, vc, table = _dev(*cpu)
        got = ops.attn_decode_paged(q, kc, vc, table, seq,
                                    split_blocks=split_blocks)
        _assert_within(got, ref_decode(*cpu, seq), **DECODE_TOL,
                       name=f"decode D hd={hd} g={group} sb={split_blocks}")

    @pytest.mark.parametrize("split_blocks,tiles", [(2, [4]), (0, [1] * 4)])
    @pytest.mark.parametrize("hd,group", [(128, 3), (128, 7), (32, 3)])
    def test_head_alone_equals_head_in_group(self, hd, group, split_blocks,
                                             tiles):
        """A head's output does not depend on which wave owns it: computed
        alone (group=1, its own q row) or inside a larger group over the
        same K/V. Tolerance, not bitwise: a different wave and a different
        lane layout accumulate it."""
        seq = self.SEQ
        _check_geometry(seq, split_blocks, tiles)
        q, kc, vc, table = _dev(*_decode_inputs(seq, hd, group))
        full = ops.attn_decode_paged(q, kc, vc, table, seq,
                                     split_blocks=split_blocks)
        for j in range(group):
            rows = [g * group + j for g in range(KH)]
            alone = ops.attn_decode_paged(q[rows].contiguous(), kc, vc, table,
                                          seq, split_blocks=split_blocks)
            _assert_within(alone, full[rows], **DECODE_TOL,
                           name=f"decode D alone hd={hd} g={group} j={j}")


class TestDecodePages:
    # E: page sizes 16 and 256 (the engine's) with a permuted table.
    @pytest.mark.parametrize("split_blocks,tiles", [(2, [5]), (0, [1] * 5)])
    @pytest.mark.parametrize("page", [16, 256])
    @pytest.mark.parametrize("hd,group", [(32, 2), (128, 4)])
    def test_page_size(self, hd, group, page, split_blocks, tiles):
        seq = 300
        _check_geometry(seq, split_blocks, tiles)
        cpu = _decode_inputs(seq, hd, group, page=page)
        q, kc, vc, table = _dev(*cpu)
        got = ops.attn_decode_paged(q, kc, vc, table, seq,
                                    split_blocks=split_blocks)
        _assert_within(got, ref_decode(*cpu, seq), **DECODE_TOL,
                       name=f"decode E page={page} hd={hd} sb={split_blocks}")


class TestDecodeIdentity:
    # F: identity=True replaces the table read by address math and nothing
    # else, so with page_table == arange it is bitwise equal to the
    # general template (and both match the reference).
    @pytest.mark.parametrize("seq,split_blocks,tiles", [
        (129, 2, [3]), (577, 2, [10]), (300, 4, [3, 2]), (700, 4, [6, 5])])
    @pytest.mark.parametrize("hd,group", HD_GROUP)
    def test_identity_bitwise(self, seq, split_blocks, tiles, hd, group):
        _check_geometry(seq, split_blocks, tiles)
        cpu = _decode_inputs(seq, hd, group, identity=True)
        q, kc, vc, table = _dev(*cpu)
        assert torch.equal(table.cpu(), torch.arange(table.numel(),
                                                     dtype=torch.int32))
        a = ops.attn_decode_paged(q, kc, vc, table, seq, identity=True,
                                  split_blocks=split_blocks)
        b = ops.attn_decode_paged(q, kc, vc, table, seq, identity=False,
                                  split_blocks=split_blocks)
        _assert_within(a, ref_decode(*cpu, seq), **DECODE_TOL,
                       name=f"decode F s={seq} hd={hd} sb={split_blocks}")
        assert torch.equal(a, b), (
            f"identity=True differs from identity=False: max diff "
            f"{(a.float() - b.float()).abs().max():.4g}")


class TestDecodeGraphMode:
    # G: the device-position entry. The grid is sized by max_seq, the true
    # length is read on device, trailing splits are empty.
    MAX_SEQ = 1024

    @pytest.mark.parametrize("split_blocks,tiles", [(0, [1] * 5), (2, [5])])
    @pytest.mark.parametrize("hd,group", HD_GROUP)
    def test_full_length_bitwise_equals_host_length(self, hd, group,
                                                    split_blocks, tiles):
        s = 257
        _check_geometry(s, split_blocks, tiles)
        q, kc, vc, table = _dev(*_decode_inputs(s, hd, group))
        host = ops.attn_decode_paged(q, kc, vc, table, s,
                                     split_blocks=split_blocks)
        dev = ops.attn_decode_paged(q, kc, vc, table, s,
                                    pos_state=_pos_state(s - 1),
                                    split_blocks=split_blocks)
        assert torch.equal(host, dev), (
            f"graph mode differs: max diff "
            f"{(host.float() - dev.float()).abs().max():.4g}")

    @pytest.mark.parametrize("hd,group", HD_GROUP)
    def test_positions_descending_on_one_cache(self, hd, group):
        """Positions run in descending order on ONE cache, so the per-cache
        workspace carries the longer call's split state into the shorter
        one; an empty split must still publish its own (empty) state."""
        ms = self.MAX_SEQ
        cpu = _decode_inputs(ms, hd, group)
        q, kc, vc, table = _dev(*cpu)

        plan = [
            # (split_blocks, pos, tiles per split)
            (0, 1023, [1] * 16),
            (0, 500, [1] * 8 + [0] * 8),
            (0, 64, [1, 1] + [0] * 14),
            (0, 63, [1] + [0] * 15),
            (0, 62, [1] + [0] * 15),
            (0, 0, [1] + [0] * 15),
            (2, 200, [4]),            # one split, limit mid-tile
            (4, 600, [8, 2]),         # second split non-empty
            (4, 100, [2, 0]),         # second split empty after non-empty
        ]
        for split_blocks, pos, tiles in plan:
            _check_geometry(pos + 1, split_blocks, tiles, bound=ms)
            got = ops.attn_decode_paged(q, kc, vc, table, ms,
                                        pos_state=_pos_state(pos),
                                        split_blocks=split_blocks)
            _assert_within(
                got, ref_decode(*cpu, pos + 1), **DECODE_TOL,
                name=f"decode G hd={hd} sb={split_blocks} pos={pos}")

    @pytest.mark.parametrize("split_blocks,tiles", [(0, [1] * 4 + [0] * 12),
                                                    (2, [4])])
    def test_out_written_in_place(self, split_blocks, tiles):
        ms, pos, hd, group = self.MAX_SEQ, 200, 128, 4
        _check_geometry(pos + 1, split_blocks, tiles, bound=ms)
        cpu = _decode_inputs(ms, hd, group)
        q, kc, vc, table = _dev(*cpu)
        fresh = ops.attn_decode_paged(q, kc, vc, table, ms,
                                      pos_state=_pos_state(pos),
                                      split_blocks=split_blocks)
        out = torch.full_like(fresh, 7.0)
        ret = ops.attn_decode_paged(q, kc, vc, table, ms,
                                    pos_state=_pos_state(pos), out=out,
                                    split_blocks=split_blocks)
        assert ret.data_ptr() == out.data_ptr() and ret.shape == out.shape
        assert torch.equal(out, fresh)
        _assert_within(out, ref_decode(*cpu, pos + 1), **DECODE_TOL,
                       name=f"decode G out= sb={split_blocks}")


class TestDecodeMasking:
    # H: nothing at or past seq_len is ever loaded — positions past
    # seq_len - 1 clamp to the last valid row — so NaN there (and in the
    # pages the table never reaches) must not reach the output.
    @pytest.mark.parametrize("seq,tiles", [(1, 1), (7, 1), (65, 2)])
    @pytest.mark.parametrize("hd,group", HD_GROUP)
    def test_nan_past_seq_len_single_split(self, seq, tiles, hd, group):
        _check_geometry(seq, 2, [tiles])
        cpu = _decode_inputs(seq, hd, group, nan_fill=True)
        q, kc, vc, table = _dev(*cpu)
        got = ops.attn_decode_paged(q, kc, vc, table, seq, split_blocks=2)
        _assert_within(got, ref_decode(*cpu, seq), **DECODE_TOL,
                       name=f"decode H s={seq} hd={hd}")

    @pytest.mark.parametrize("seq,tiles", [(1, 1), (7, 1), (65, 2)])
    @pytest.mark.parametrize("hd,group", HD_GROUP)
    def test_nan_past_seq_len_graph_mode(self, seq, tiles, hd, group):
        ms = TestDecodeGraphMode.MAX_SEQ
        _check_geometry(seq, 0, [1] * tiles + [0] * (16 - tiles), bound=ms)
        cpu = _decode_inputs(seq, hd, group, nan_fill=True, cover=ms)
        q, kc, vc, table = _dev(*cpu)
        got = ops.attn_decode_paged(q, kc, vc, table, ms,
                                    pos_state=_pos_state(seq - 1))
        _assert_within(got, ref_decode(*cpu, seq), **DECODE_TOL,
                       name=f"decode H graph s={seq} hd={hd}")


class TestDecodeUnifiedEntry:
    # K: host-length and device-position calls go through ONE entry with one
    # set of argument checks. kh=2, hq=4, hd=32, page=16 over 4 pages at
    # seq=17 is the smallest geometry that crosses a page boundary, so the
    # page table is really walked. A refused call raises before anything is
    # launched: the sentinel `out` it was handed stays untouched.
    HD, GROUP, PAGE, SEQ = 32, 2, 16, 17

    def _inputs(self):
        q, kc, vc, table = _dev(*_decode_inputs(self.SEQ, self.HD, self.GROUP,
                                                page=self.PAGE))
        assert kc.shape == (4, self.PAGE, KH, self.HD) and q.shape[0] == 4
        return q, kc, vc, table

    def test_pos_state_bitwise_equals_host_length(self):
        q, kc, vc, table = self._inputs()
        host = ops.attn_decode_paged(q, kc, vc, table, self.SEQ)
        dev = ops.attn_decode_paged(q, kc, vc, table, self.SEQ,
                                    pos_state=_pos_state(self.SEQ - 1))
        assert torch.equal(host, dev)
        cpu = _decode_inputs(self.SEQ, self.HD, self.GROUP, page=self.PAGE)
        _assert_within(host, ref_decode(*cpu, self.SEQ), **DECODE_TOL,
                       name="decode K host")

    def test_out_written_in_place_both_modes(self):
        q, kc, vc, table = self._inputs()
        want = ops.attn_decode_paged(q, kc, vc, table, self.SEQ)
        for pos_state in (None, _pos_state(self.SEQ - 1)):
            out = torch.full_like(want, 7.0)
            ret = ops.attn_decode_paged(q, kc, vc, table, self.SEQ,
                                        pos_state=pos_state, out=out)
            assert ret.data_ptr() == out.data_ptr()
            assert torch.equal(out, want)

    @pytest.mark.parametrize("case", [
        "pos_state int64", "pos_state on cpu", "float16 cache", "hq=3",
        "hd=48", "out wrong shape", "seq_len past the cache",
        "seq_len past the cache, graph mode",
    ])
    def test_refused_on_the_host(self, case):
        q, kc, vc, table = self._inputs()
        seq, kw = self.SEQ, {}
        out = torch.full((4, self.HD), 7.0, dtype=torch.bfloat16, device=DEV)
        if case == "pos_state int64":
            kw["pos_state"] = torch.tensor([seq - 1], device=DEV)
        elif case == "pos_state on cpu":
            kw["pos_state"] = torch.tensor([seq - 1], dtype=torch.int32)
        elif case == "float16 cache":
            kc, vc = kc.to(torch.float16), vc.to(torch.float16)
        elif case == "hq=3":
            q, out = q[:3].contiguous(), out[:3].contiguous()
        elif case == "hd=48":
            q = _bf(torch.randn(4, 48)).to(DEV)
            kc = _bf(torch.randn(4, self.PAGE, KH, 48)).to(DEV)
            vc = kc.clone()
            out = torch.full((4, 48), 7.0, dtype=torch.bfloat16, device=DEV)
        elif case == "out wrong shape":
            out = torch.full((4, self.HD + 8), 7.0, dtype=torch.bfloat16,
                             device=DEV)
        elif case == "seq_len past the cache":
            seq = 4 * self.PAGE + 1
        else:
            seq = 4 * self.PAGE + 1
            kw["pos_state"] = _pos_state(self.SEQ - 1)
        with pytest.raises(RuntimeError):
            ops.attn_decode_paged(q, kc, vc, table, seq, out=out, **kw)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), f"{case}: out written despite refusal"


# ---------------------------------------------------------------------------
# prefill
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _prefill_inputs(tq, tk, hq, kh, hd):
    gen = torch.Generator().manual_seed(tq * 100003 + tk * 1009 + hd)
    q = _bf(torch.randn(tq, hq, hd, generator=gen))
    k = _bf(torch.randn(tk, kh, hd, generator=gen))
    v = _bf(torch.randn(tk, kh, hd, generator=gen))
    return q, k, v


# (63, 16) makes the first wave's first tile exactly unmasked
# (kv_offset + q0 + 1 == 64, the mask-skipping fast path); (62, 16) is one
# key short of it, the case an off-by-one in that predicate would get wrong.
OFFSETS_MFMA = [(1, 1), (63, 16), (64, 42), (65, 128), (200, 130), (127, 129),
                (62, 16)]


class TestPrefillOffset:
    # I: chunked-prefill geometry on the MFMA kernel (hd=128, causal).
    @pytest.mark.parametrize("kv_offset,tq", OFFSETS_MFMA)
    def test_mfma_kv_offset(self, kv_offset, tq):
        cpu = _prefill_inputs(tq, kv_offset + tq, 4, 2, 128)
        q, k, v = _dev(*cpu)
        got = ops.attn_prefill(q, k, v, kv_offset=kv_offset)
        _assert_within(got, ref_attention(*cpu, kv_offset=kv_offset),
                       **PREFILL_TOL, name=f"prefill I off={kv_offset} tq={tq}")

    # J: the same kind of offsets through the simple kernel.
    @pytest.mark.parametrize("kv_offset,tq", [(5, 7), (64, 33)])
    @pytest.mark.parametrize("hd", [32, 64])
    def test_simple_kv_offset(self, hd, kv_offset, tq):
        cpu = _prefill_inputs(tq, kv_offset + tq, 4, 2, hd)
        q, k, v = _dev(*cpu)
        got = ops.attn_prefill(q, k, v, kv_offset=kv_offset)
        _assert_within(got, ref_attention(*cpu, kv_offset=kv_offset),
                       **PREFILL_TOL,
                       name=f"prefill J hd={hd} off={kv_offset} tq={tq}")

    def test_simple_anchor_hd128(self):
        kv_offset, tq, hd = 65, 128, 128
        cpu = _prefill_inputs(tq, kv_offset + tq, 4, 2, hd)
        q, k, v = _dev(*cpu)
        scale = 1.0 / math.sqrt(hd)
        simple = _hip.attn_prefill_simple(q, k, v, scale, True, kv_offset)
        mfma = _hip.attn_prefill(q, k, v, scale, True, kv_offset)
        _assert_within(simple, ref_attention(*cpu, kv_offset=kv_offset),
                       **PREFILL_TOL, name="prefill J anchor simple vs ref")
        _assert_within(mfma, simple, **PREFILL_TOL,
                       name="prefill J anchor mfma vs simple")

    # K: 298 rows as 128 + 128 + 42 with K/V prefixes sliced the way the
    # model's chunked prefill slices its cache view.
    def test_chunked_equals_single_shot(self):
        n, hq, kh, hd = 298, 4, 2, 128
        cpu = _prefill_inputs(n, n, hq, kh, hd)
        q, k, v = _dev(*cpu)
        want = ref_attention(*cpu)
        single = ops.attn_prefill(q, k, v)
        _assert_within(single, want, **PREFILL_TOL, name="prefill K single")
        pos0 = 0
        for t in (128, 128, 42):
            qc = q[pos0:pos0 + t]
            k_all, v_all = k[:pos0 + t], v[:pos0 + t]
            if pos0 == 0:
                got = ops.attn_prefill(qc, k_all, v_all)
            else:
                got = ops.attn_prefill(qc, k_all, v_all, kv_offset=pos0)
            _assert_within(got, want[pos0:pos0 + t], **PREFILL_TOL,
                           name=f"prefill K chunk@{pos0} vs ref")
            _assert_within(got, single[pos0:pos0 + t], **PREFILL_TOL,
                           name=f"prefill K chunk@{pos0} vs single-shot")
            pos0 += t
        assert pos0 == n


class TestPrefillNonCausal:
    # L: causal=False always takes the simple kernel, hd=128 included.
    @pytest.mark.parametrize("tq,tk,hd", [(5, 77, 32), (5, 77, 64),
                                          (5, 77, 128), (70, 70, 128)])
    def test_vs_ref(self, tq, tk, hd):
        cpu = _prefill_inputs(tq, tk, 4, 2, hd)
        q, k, v = _dev(*cpu)
        got = ops.attn_prefill(q, k, v, causal=False)
        _assert_within(got, ref_attention(*cpu, causal=False), **PREFILL_TOL,
                       name=f"prefill L tq={tq} tk={tk} hd={hd}")


DEFER_THR = 8.0  # nats; attn_prefill_mfma.hip keeps a stale max up to this


def _ramp_inputs(c):
    """q, k, v (bf16, CPU) whose scaled score of key j is about
    c * floor(j / 64) for every query: all vectors share one unit
    direction, keys carry the ramp in their magnitude."""
    tq = tk = 320
    hq, kh, hd = 2, 1, 128
    gen = torch.Generator().manual_seed(int(c * 10))
    u = torch.randn(hd, generator=gen)
    u = u / u.norm()
    qmag = 4.0
    scale = 1.0 / math.sqrt(hd)
    kmag = c * (torch.arange(tk) // 64).float() / (scale * qmag)
    q = u * qmag + 0.02 * torch.randn(tq, hq, hd, generator=gen)
    k = u * kmag.view(tk, 1, 1) + 0.1 * torch.randn(tk, kh, hd, generator=gen)
    v = torch.randn(tk, kh, hd, generator=gen)
    return _bf(q), _bf(k), _bf(v)


def _defer_trace(q, k, head=0):
    """Replay the kernel's wave-uniform defer decision from float64 scores:
    for every 16-row wave and every 64-key tile it visits, the largest
    growth (nats) of a row max over the running max the kernel holds, and
    whether the kernel keeps the stale max. Tiles within 0.1 nat of the
    threshold are reported as 'edge' and count for neither side."""
    tq, hq, hd = q.shape
    tk = k.shape[0]
    s = torch.einsum("qd,kd->qk", q[:, head].double(),
                     k[:, 0].double()) / math.sqrt(hd)
    s = s.masked_fill(torch.arange(tk)[None, :] > torch.arange(tq)[:, None],
                      float("-inf"))
    trace = []
    for r0 in range(0, tq, 16):
        kmax = min(tk, (r0 // 128) * 128 + 128)
        m = torch.full((min(16, tq - r0),), float("-inf"), dtype=torch.float64)
        for kt in range(0, kmax, 64):
            mx = s[r0:r0 + 16, kt:kt + 64].amax(dim=1)
            growth = torch.where(torch.isinf(mx) & (mx < 0),
                                 torch.full_like(mx, float("-inf")), mx - m)
            g = float(growth.max())
            if g <= DEFER_THR - 0.1:
                kind = "defer"
            elif g >= DEFER_THR + 0.1:
                kind = "rescale"
                m = torch.maximum(m, mx)
            else:
                kind = "edge"
                m = torch.maximum(m, mx)
            trace.append((r0, kt, g, kind))
    return trace


class TestPrefillDeferredMax:
    # M: the running max grows by a few nats per tile, so P reaches e^c
    # .. e^8 against a stale max before a rescale is forced.
    @pytest.mark.parametrize("c", [3.0, 7.5, 9.0])
    def test_ramp(self, c):
        cpu = _ramp_inputs(c)
        trace = [t for t in _defer_trace(cpu[0], cpu[1]) if t[1] > 0]
        assert not [t for t in trace if t[3] == "edge"], trace
        last_wave = [t for t in trace if t[0] == 304 and t[1] < 320]
        kinds = [t[3] for t in last_wave]
        if c == 9.0:
            # every tile raises the max past the threshold
            assert kinds == ["rescale"] * 4, last_wave
        else:
            # stale max kept while P grows to >= e^c, then a forced rescale
            grown = [t for t in last_wave if t[3] == "defer" and t[2] >= c - 1]
            assert grown and "rescale" in kinds[kinds.index("defer"):], (
                last_wave)
        q, k, v = _dev(*cpu)
        got = ops.attn_prefill(q, k, v)
        _assert_within(got, ref_attention(*cpu), **PREFILL_TOL,
                       name=f"prefill M c={c}")
