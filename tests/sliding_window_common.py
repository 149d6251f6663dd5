"""What tests/test_sliding_window_cpu.py and tests/test_sliding_window_gpu.py
share: the float64 sliding-window reference, the input builders whose values
make a leak unmissable, and the constants of the end-to-end case. Nothing
here needs a GPU; the CPU module checks all of it.

`window = W >= 1`: the query at absolute position i sees keys
max(0, i - W + 1) .. i; 0 = off.

Tolerances, `_assert_within` and the small helpers are those of
tests/test_attention_edges_gpu.py, loaded from that file (decode
atol=rtol=2e-2, prefill atol=2.5e-2 / rtol=2e-2, zero elements out of bound).

What is outside a window must not merely be down-weighted, so the inputs make
a leak unmissable, with finite values only (`0 * inf` in PV is not something
the kernels promise to survive on real rows):

  - decode: every cache row outside [lo, seq_len), below the window and past
    the sequence alike, has a K row that is a large multiple of the query
    direction (score about 30 nats above anything in the window) and a V row
    of 1e3. One leaked row moves the output by about 1e3.
  - prefill: a key is inside the window of its own query, so no key can be
    poisoned for every row. In the `ramp` inputs the score of key j falls by
    RAMP_C nats per position for every query: each key below a row's window
    outweighs every key in it, a leaked one takes most of the softmax and the
    output moves by O(1) (V rows are independent normals). The same ramp
    makes the lowest key of the window the heaviest, so masking one key too
    many shows just as clearly. The `plain` inputs (normal q, k, v) weigh the
    newest keys as much as the oldest.
"""

import dataclasses
import functools
import importlib.util
import math
import os

import torch

from adversarial_spec_amd.models import LlamaModel, get_config
from adversarial_spec_amd.ops import torch_ref

_spec = importlib.util.spec_from_file_location(
    "_attention_edges_for_window",
    os.path.join(os.path.dirname(__file__), "test_attention_edges_gpu.py"))
edges = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(edges)

DEV = edges.DEV
KH = edges.KH
DTILE = edges.DTILE
DECODE_TOL = edges.DECODE_TOL
PREFILL_TOL = edges.PREFILL_TOL
_bf, _dev, _pos_state = edges._bf, edges._dev, edges._pos_state
_assert_within = edges._assert_within


# ---------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------

def ref_attention_w(q, k, v, scale=None, kv_offset=0, window=0):
    """Causal softmax attention in float64 with a sliding window, by a
    brute-force mask. q [tq, hq, hd]; k, v [tk, kh, hd]; query row i sits at
    absolute position p = kv_offset + i and sees key j iff j <= p and (window
    == 0 or j >= p - window + 1). Returns float64 [tq, hq, hd]."""
    tq, hq, hd = q.shape
    tk, kh, _ = k.shape
    if scale is None:
        scale = 1.0 / math.sqrt(hd)
    group = hq // kh
    out = torch.zeros(tq, hq, hd, dtype=torch.float64)
    qd, kd, vd = q.double().cpu(), k.double().cpu(), v.double().cpu()
    for i in range(tq):
        p = kv_offset + i
        seen = [j for j in range(tk)
                if j <= p and (window == 0 or j >= p - window + 1)]
        for h in range(hq):
            s = (kd[seen, h // group] @ qd[i, h]) * scale
            w = (s - s.max()).exp()
            out[i, h] = (w / w.sum()) @ vd[seen, h // group]
    return out


def ref_decode_w(q, k_rows, v_rows, seq_len, window=0):
    """Single-token decode over logical rows k_rows, v_rows [n, kh, hd]: the
    query is at position seq_len - 1 and sees the last `window` of the
    first seq_len rows (all of them when window == 0)."""
    return ref_attention_w(q.unsqueeze(0), k_rows[:seq_len], v_rows[:seq_len],
                           kv_offset=seq_len - 1, window=window)[0]


# ---------------------------------------------------------------------------
# prefill inputs
# ---------------------------------------------------------------------------

RAMP_C = 0.5   # nats by which key j outweighs key j + 1, for every query
QMAG = 4.0     # length of the shared direction in every q row


@functools.lru_cache(maxsize=None)
def prefill_inputs(kind, n, hq, kh, hd):
    """q [n, hq, hd], k, v [n, kh, hd] (bf16, CPU), built once per shape."""
    gen = torch.Generator().manual_seed(n * 1009 + hd * 7 + len(kind))
    v = torch.randn(n, kh, hd, generator=gen)
    if kind == "plain":
        q = torch.randn(n, hq, hd, generator=gen)
        k = torch.randn(n, kh, hd, generator=gen)
    else:
        assert kind == "ramp"
        u = torch.randn(hd, generator=gen)
        u = u / u.norm()
        scale = 1.0 / math.sqrt(hd)
        kmag = RAMP_C * (n - 1 - torch.arange(n)).float() / (scale * QMAG)
        q = u * QMAG + 0.02 * torch.randn(n, hq, hd, generator=gen)
        k = u * kmag.view(n, 1, 1) + 0.1 * torch.randn(n, kh, hd,
                                                       generator=gen)
    return _bf(q), _bf(k), _bf(v)


@functools.lru_cache(maxsize=None)
def prefill_ref(kind, n, hq, kh, hd, window):
    return ref_attention_w(*prefill_inputs(kind, n, hq, kh, hd),
                           window=window)


# ---------------------------------------------------------------------------
# decode inputs
# ---------------------------------------------------------------------------

POISON_NATS = 30.0   # score of a poisoned K row above a typical one
POISON_V = 1e3


@functools.lru_cache(maxsize=None)
def decode_case(seq, window, hd, group, fp8=False, identity=False, cover=0,
                page=64):
    """CPU inputs of one decode case: dict with q [KH*group, hd] bf16, the
    cache tensors laid out through `table` (kc, vc bf16, or uint8 plus ks, vs
    for fp8), `k_rows`, `v_rows` = the logical rows as the kernel reads them
    (bf16-rounded, or dequantized, in float64) and `lo`. Rows outside
    [lo, seq) and every page the table does not reach are poison."""
    gen = torch.Generator().manual_seed(
        seq * 100003 + window * 917 + hd * 1009 + group * 101 + cover)
    n_used = (max(seq, cover) + page - 1) // page
    npg = n_used + 2
    if identity:
        table = torch.arange(npg, dtype=torch.int32)
    else:
        table = torch.randperm(npg, generator=gen).to(torch.int32)
    used = table[:n_used].long()
    u = torch.randn(KH, hd, generator=gen)
    u = u / u.norm(dim=-1, keepdim=True)
    q = (u.unsqueeze(1) * QMAG
         + 0.5 * torch.randn(KH, group, hd, generator=gen)).reshape(
             KH * group, hd)
    kp = POISON_NATS * math.sqrt(hd) / QMAG
    lo = max(0, seq - window) if window else 0
    n = n_used * page
    outside = torch.ones(n, dtype=torch.bool)
    outside[lo:seq] = False
    k = torch.randn(n, KH, hd, generator=gen)
    v = torch.randn(n, KH, hd, generator=gen)
    k[outside] = u * kp
    v[outside] = POISON_V
    case = {"q": _bf(q), "table": table, "lo": lo}
    pools = {}
    for name, rows, fill in (("k", k, u * kp), ("v", v, None)):
        pool = torch.empty(npg, page, KH, hd)
        pool[:] = POISON_V if fill is None else fill
        pool[used] = rows.view(n_used, page, KH, hd)
        pools[name] = pool
    if fp8:
        for name in ("k", "v"):
            c8, cs = torch_ref.quantize_kv_fp8(pools[name])
            case[name + "c"] = c8
            case[name + "s"] = cs.permute(0, 2, 1).contiguous()
            deq = c8.view(torch.float8_e4m3fn).double() * cs.double().unsqueeze(-1)
            case[name + "_rows"] = deq[used].reshape(n, KH, hd)
    else:
        for name in ("k", "v"):
            case[name + "c"] = _bf(pools[name])
            case[name + "_rows"] = case[name + "c"][used].reshape(
                n, KH, hd).double()
    return case


def decode_ref(case, seq, window):
    return ref_decode_w(case["q"], case["k_rows"], case["v_rows"], seq, window)


def walked_tiles(seq, window, n_splits, split_len):
    """64-position tiles each split block walks at true length `seq`."""
    lo = max(0, seq - window) if window else 0
    base = lo // DTILE * DTILE
    tiles = []
    for i in range(n_splits):
        start = base + i * split_len
        limit = min(seq, start + split_len)
        tiles.append(max(0, -(-(limit - start) // DTILE)))
    return tiles


# ---------------------------------------------------------------------------
# end-to-end constants (fixed on the CPU by test_sliding_window_cpu.py)
# ---------------------------------------------------------------------------

E2E_WINDOW = 96
E2E_SEED = 13
E2E_PROMPT = 70
E2E_STEPS = 80
# decode steps whose logits are compared (step i reads a cache of
# E2E_PROMPT + i rows): one between the window and the first tile boundary,
# the rest past both. At these steps the CPU model's top-1 leads by >= 0.2
# on logits of size ~1.4, and the windowed logits have cosine <= 0.98 with
# the window=0 ones.
E2E_CHECK_STEPS = (56, 71, 76, 78)
E2E_COS = 0.99   # test_engine_gpu.py: top-1 agreement and cosine > 0.99


def e2e_tokens():
    gen = torch.Generator().manual_seed(E2E_SEED)
    return torch.randint(0, 1024, (E2E_PROMPT + E2E_STEPS,), generator=gen)


def e2e_config(window=E2E_WINDOW):
    return dataclasses.replace(get_config("tiny"), sliding_window=window)


def e2e_logits(model, kv_dtype="bf16"):
    """Prefill the prompt, then teacher-forced decode_one steps: logits
    [1 + E2E_STEPS, vocab] as float32 on the CPU; row 0 is the prefill's."""
    toks = e2e_tokens().to(model.device)
    cache = model.new_cache(256, kv_dtype=kv_dtype)
    rows = [model.prefill(toks[:E2E_PROMPT], cache)]
    for tok in toks[E2E_PROMPT:].tolist():
        rows.append(model.decode_one(tok, cache))
    return torch.stack(rows).float().cpu()


def e2e_within(a, b):
    """The engine test's criterion on two logit rows."""
    cos = torch.nn.functional.cosine_similarity(
        a.unsqueeze(0), b.unsqueeze(0)).item()
    return a.argmax().item() == b.argmax().item() and cos > E2E_COS, cos


@functools.lru_cache(maxsize=None)
def e2e_cpu_model(window):
    return LlamaModel(e2e_config(window), device="cpu",
                      seed=E2E_SEED).init_random()


@functools.lru_cache(maxsize=None)
def e2e_cpu_logits(window, kv_dtype="bf16"):
    return e2e_logits(e2e_cpu_model(window), kv_dtype)
