"""Helpers shared by test_gemv_exact_cpu.py and test_gemv_exact_gpu.py: the
loop geometry of the decode GEMV kernels, inputs for which their fp32
arithmetic is exact, fp64 references, and the bf16 / e4m3 bracket rules.
Everything here runs on the CPU and depends on torch alone."""

import math

import torch

BF16 = torch.bfloat16
F8 = torch.float8_e4m3fn

# (L lanes per row, U unroll depth, E elements per 16-byte chunk) of every
# decode GEMV kernel. This mirrors the loop pair each kernel in
# ops/hip/gemv.hip and ops/hip/gemv_fp8.hip runs per lane, with nc = K / E
# and c starting at the lane's index sl in [0, L):
#     for (; c + (U - 1) * L < nc; c += U * L)   // unrolled
#     for (; c < nc; c += L)                     // remainder
# e.g. gemv_kernel_w32: `c + 224 < nc; c += 256` then `c < nc; c += 32`.
KERNELS = {
    # gemv.hip (bf16, 8 elements per chunk)
    "gemv_kernel_w32": (32, 8, 8),
    "gemv_kernel": (16, 4, 8),
    "gemv_gateup_kernel": (32, 4, 8),
    "gemv_norm_w32_kernel": (32, 8, 8),
    "gemv_norm_kernel": (16, 4, 8),
    "gemv_norm_rope_kv_w32_kernel": (32, 8, 8),
    "gemv_res_w32_kernel": (32, 8, 8),
    "gemv_gateup_norm_kernel": (32, 4, 8),
    # gemv_fp8.hip (e4m3, 16 elements per chunk)
    "gemv_fp8_kernel_w32": (32, 4, 16),
    "gemv_fp8_kernel": (16, 4, 16),
    "gemv_fp8_rope_kv_w32_kernel": (32, 4, 16),
    "gemv_fp8_res_w32_kernel": (32, 4, 16),
    "gemv_fp8_gateup_kernel": (32, 4, 16),
    "gemv_fp8_norm_w32_kernel": (32, 4, 16),
    "gemv_fp8_norm_kernel": (16, 4, 16),
    "gemv_fp8_resl_w32_kernel": (32, 4, 16),
    "gemv_fp8_gateup_norm_kernel": (32, 4, 16),
}

# op (the name in adversarial_spec_amd.ops) -> (kernel for N <= 8192, kernel
# for N > 8192 or None where the binding refuses such an N or has one kernel)
OPS = {
    "gemv": ("gemv_kernel_w32", "gemv_kernel"),
    "gemv_res": ("gemv_res_w32_kernel", None),
    "gemv_gateup": ("gemv_gateup_kernel", None),
    "gemv_norm": ("gemv_norm_w32_kernel", "gemv_norm_kernel"),
    "gemv_norm_rope_kv": ("gemv_norm_rope_kv_w32_kernel", None),
    "gemv_gateup_norm": ("gemv_gateup_norm_kernel", None),
    "gemv_fp8": ("gemv_fp8_kernel_w32", "gemv_fp8_kernel"),
    "gemv_fp8_q": ("gemv_fp8_kernel_w32", "gemv_fp8_kernel"),
    "gemv_fp8_res": ("gemv_fp8_res_w32_kernel", None),
    "gemv_fp8_gateup": ("gemv_fp8_gateup_kernel", None),
    "gemv_fp8_norm": ("gemv_fp8_norm_w32_kernel", "gemv_fp8_norm_kernel"),
    "gemv_fp8_resl": ("gemv_fp8_resl_w32_kernel", None),
    "gemv_fp8_gateup_norm": ("gemv_fp8_gateup_norm_kernel", None),
}

# every output is bf16-exact and must match bit for bit
EXACT_OPS = ("gemv", "gemv_res", "gemv_fp8_q", "gemv_fp8", "gemv_fp8_res",
             "gemv_fp8_resl")
# an inexact fp32 step (rsqrtf, __expf, a scale product) sits between the
# exact dot and the bf16 store: the bracket rule
BRACKET_OPS = ("gemv_norm", "gemv_gateup", "gemv_gateup_norm",
               "gemv_norm_rope_kv", "gemv_fp8_gateup", "gemv_fp8_norm",
               "gemv_fp8_gateup_norm")
# the four ops whose launcher switches kernels at N == 8192
SWITCHING_OPS = ("gemv", "gemv_norm", "gemv_fp8_q", "gemv_fp8_norm")

N_TAILS = (1, 7, 8, 9, 17)   # row tails of the 8-row and the 16-row grids
N_SWITCH = 8192              # launchers: N <= 8192 -> 32 lanes per row
EPS = 1e-5
K_LABELS = ("one_lane", "rem_only", "half_unrolled", "unrolled_only",
            "unrolled_plus_one", "both_loops")


def k_cases(kernel):
    """label -> K for the six lane splits worth running (nc = K / E)."""
    L, U, E = KERNELS[kernel]
    ncs = (1, L + 1, U * L - L // 2, U * L, U * L + 1, 2 * U * L + L + 1)
    return {label: nc * E for label, nc in zip(K_LABELS, ncs)}


def lane_trips(nc, L, U):
    """Per lane sl: (unrolled iterations, remainder iterations, chunks read),
    walking the same inequalities as the kernels."""
    trips = []
    for sl in range(L):
        c, main, rem, chunks = sl, 0, 0, []
        while c + (U - 1) * L < nc:
            chunks += [c + L * u for u in range(U)]
            main += 1
            c += U * L
        while c < nc:
            chunks.append(c)
            rem += 1
            c += L
        trips.append((main, rem, chunks))
    return trips


# ---- bf16 / e4m3 grids -----------------------------------------------------

def bf16_bracket(ref64):
    """(lo, hi): the largest bf16 <= ref and the smallest bf16 >= ref, for a
    finite fp64 tensor. lo == hi exactly where ref is representable."""
    ref64 = ref64.double()
    # one of the two neighbours, whichever way the two roundings fall
    b = ref64.float().to(BF16)
    assert torch.isfinite(b.float()).all()
    bits = b.view(torch.int16).to(torch.int32) & 0xFFFF
    mag = bits & 0x7FFF
    neg = (bits & 0x8000) != 0
    zero = mag == 0
    # next towards +inf / -inf on the sign-magnitude grid
    up = torch.where(zero, torch.full_like(bits, 0x0001),
                     torch.where(neg, bits - 1, bits + 1))
    dn = torch.where(zero, torch.full_like(bits, 0x8001),
                     torch.where(neg, bits + 1, bits - 1))

    def as_bf16(i32):
        i16 = torch.where(i32 >= 0x8000, i32 - 0x10000, i32).to(torch.int16)
        return i16.view(BF16)

    bd = b.double()
    lo = torch.where(bd <= ref64, b, as_bf16(dn))
    hi = torch.where(bd >= ref64, b, as_bf16(up))
    return lo, hi


def bracket_violations(got, ref64):
    """Flat indices where a bf16 result is neither neighbour of ref64 (an
    exactly representable ref, zero included, must be hit exactly)."""
    lo, hi = bf16_bracket(ref64.reshape(-1))
    g = got.reshape(-1).cpu().double()
    ok = (g == lo.double()) | (g == hi.double())
    return torch.nonzero(~ok).flatten()


def bf16_step(v64):
    """Spacing of the bf16 grid at magnitude |v| (2^-133 in the subnormals)."""
    a = v64.double().abs().clamp_min(2.0 ** -126)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - 7)


def e4m3_grid():
    """Every finite e4m3fn value, ascending (fp64), zero once."""
    v = torch.arange(256, dtype=torch.int16).to(torch.uint8).view(F8).double()
    return torch.unique(v[torch.isfinite(v)])


def e4m3_bracket(v64):
    """(lo, hi) e4m3fn grid points around v (|v| <= 448), as fp64."""
    grid = e4m3_grid()
    v64 = v64.double()
    assert (v64.abs() <= 448).all()
    hi_i = torch.searchsorted(grid, v64)          # first grid >= v
    hi = grid[hi_i]
    lo = torch.where(hi == v64, hi, grid[(hi_i - 1).clamp_min(0)])
    return lo, hi


def e4m3_codes(vals):
    """The e4m3fn bytes of values that lie on the grid (asserted)."""
    q = vals.float().to(F8)
    assert torch.equal(q.double(), vals.double()), "value off the e4m3 grid"
    return q.view(torch.uint8)


def e4m3_values(codes):
    return codes.view(F8).double()


# ---- inputs ------------------------------------------------------------------

def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(shape, lim, g, dtype=torch.float64):
    return torch.randint(-lim, lim + 1, shape, generator=g).to(dtype)


def wsc_pow2(n_rows):
    """A power-of-two scale per weight row that varies with the row, so a
    wrong-row scale read shows."""
    n = torch.arange(n_rows)
    return torch.pow(2.0, ((n % 5) - 2).double()).float()


def wln_pow2(k):
    """rmsnorm weights in {0.5, 1, 2}: x * wln stays exact in bf16."""
    return torch.tensor([0.5, 1.0, 2.0]).double()[torch.arange(k) % 3]


class Case:
    """One problem: master copies of every operand (fp64; the weight fp32,
    which holds its small integers exactly at half the memory), all of them
    exactly representable in the dtype the kernel reads, plus the scales."""

    def __init__(self, **kw):
        self.wln = self.resid = None
        self.xs = 1.0          # activation scale of the pre-quantized ops
        self.gate_shift = 0    # gate rows are scaled by 2^-gate_shift
        self.wsc = None        # fp8 weight-row scales (float32 tensor)
        self.rows = None       # weight rows (2 * N for the gate_up ops)
        self.__dict__.update(kw)


def is_fp8(op):
    return "fp8" in op


def is_gateup(op):
    return "gateup" in op


def is_norm(op):
    return "norm" in op


def has_resid(op):
    return "res" in op


def self_quantizing(op):
    return op in ("gemv_fp8", "gemv_fp8_res", "gemv_fp8_resl",
                  "gemv_fp8_norm", "gemv_fp8_gateup_norm")


def dense_case(op, K, N, seed=0, j=0):
    """Small-integer operands: every product and partial sum of the dot is an
    exact fp32 integer times a power of two, in any summation order.

    bf16 ops: x, W integers in [-8, 8]. fp8 ops: integers in [-16, 16] (exact
    in e4m3). Pre-quantized ops take xs = 2^j; self-quantizing ops take x
    scaled by 2^j with one element 448 * 2^j, which makes the row scale
    exactly 2^j and every code exact. The norm ops multiply by wln in
    {0.5, 1, 2} (the fp8 ones draw x from [-8, 8] so that x * wln stays on the
    e4m3 grid). Gate rows of the gate_up ops are scaled down by a power of two
    (in the bf16 weight, or in the fp8 row scale) so that silu's argument
    stays far from the fp32 overflow of exp."""
    g = _gen(seed * 7919 + K * 31 + N)
    f8 = is_fp8(op)
    rows = 2 * N if is_gateup(op) else N
    lim = 16 if f8 else 8
    c = Case(op=op, K=K, N=N, rows=rows, j=j)
    xlim = 8 if (f8 and is_norm(op)) else lim
    c.x = _ints((K,), xlim, g)
    c.w = _ints((rows, K), lim, g, torch.float32)
    if is_norm(op):
        c.wln = wln_pow2(K)
    if f8:
        c.wsc = wsc_pow2(rows)
        if self_quantizing(op):
            pin = int(torch.randint(0, K, (1,), generator=g))
            c.x[pin] = 448.0
            if c.wln is not None:
                c.wln[pin] = 1.0
            c.x = c.x * 2.0 ** j
        else:
            c.xs = 2.0 ** j
    if is_gateup(op):
        # |gate dot| grows like sqrt(K); keep silu's argument within +-64
        c.gate_shift = gate_shift(c)
    if has_resid(op):
        c.resid = _ints((N,), 8, g)
    return c


def gate_shift(c):
    """Smallest power-of-two shift bringing every gate pre-activation of the
    case (before the shift) to at most 64 in magnitude."""
    g = reference(c, pre_activation=True)[0].abs().max().item()
    return max(0, math.ceil(math.log2(max(g, 1.0) / 64.0)))


def materialize(c):
    """The case's operands as the CPU tensors the op takes, in the kernel's
    own dtypes; every conversion is asserted exact."""

    def bf(t):
        b = t.to(BF16)
        assert torch.equal(b.double(), t.double()), "operand not exact in bf16"
        return b

    m = {}
    gate = torch.ones(c.rows, dtype=torch.float64)
    if is_gateup(c.op):
        gate[:c.N] = 2.0 ** -c.gate_shift
    if is_fp8(c.op):
        m["w8"] = e4m3_codes(c.w)
        wsc = (c.wsc.double() * gate).float()
        assert torch.equal(wsc.double(), c.wsc.double() * gate)
        m["wsc"] = wsc
        if self_quantizing(c.op):
            m["x"] = bf(c.x).view(1, -1)
        else:
            m["x8"] = e4m3_codes(c.x).view(1, -1)
            m["xs"] = torch.tensor([c.xs], dtype=torch.float32)
    else:
        m["x"] = bf(c.x).view(1, -1)
        m["w"] = bf(c.w * gate[:, None].float())
    if c.wln is not None:
        m["wln"] = bf(c.wln)
    if c.resid is not None:
        m["resid"] = bf(c.resid).view(1, -1)
    return m


def probe_stride(K, E):
    """First stride >= 2E + 5 coprime to K: consecutive rows then select
    columns of different chunks, and N >= K rows select every column."""
    s = 2 * E + 5
    while math.gcd(s, K) != 1:
        s += 1
    return s


def probe_columns(K, rows, E):
    return (torch.arange(rows) * probe_stride(K, E)) % K


def probe_case(op, K, N):
    """Permutation probe: weight row n is one-hot (1.0) at column
    (n * stride) % K and x[k] is a distinct-ish exactly representable value,
    so every output names the one input element it read."""
    f8 = is_fp8(op)
    E = 16 if f8 else 8
    rows = 2 * N if is_gateup(op) else N
    assert N >= K, "the probe needs a row for every column"
    c = Case(op=op, K=K, N=N, rows=rows, j=0)
    c.cols = probe_columns(K, rows, E)
    c.w = torch.zeros(rows, K, dtype=torch.float32)
    c.w[torch.arange(rows), c.cols] = 1.0
    k = torch.arange(K)
    if f8 and not is_norm(op):
        # the 126 positive finite e4m3 values, 448 (code 126) among them: a
        # self-quantizing op then finds the row scale exactly 1
        assert K >= 126
        c.x = e4m3_values(((k % 126) + 1).to(torch.uint8))
    else:
        c.x = ((k % 251) + 1).double()
    if is_norm(op):
        c.wln = wln_pow2(K)
    if f8:
        # the norm-fused ops quantize on top of an inexact rms: wsc = 1 there
        c.wsc = (torch.ones(rows) if is_norm(op) else wsc_pow2(rows)).float()
    if has_resid(op):
        c.resid = -(torch.arange(N) % 5).double()
    return c


# ---- references ----------------------------------------------------------------

def reference(c, dtype=torch.float64, pre_activation=False, chunk=2048):
    """The op's result before the bf16 store, computed in `dtype` on the CPU
    (fp64 is the reference; fp32 checks that the inputs make fp32 exact).
    Returns (result [N], max over rows of sum_k |x_k * w_nk| — a bound on
    every partial sum of the dot in any order, in the integer units of the
    operands —, the raw dots [rows] in the same units).

    The fp8 norm-fused ops are only supported for dense cases, where the
    quantization is exact by construction (asserted)."""
    op = c.op
    x = c.x.to(dtype)
    if c.wln is not None:
        xe = x * c.wln.to(dtype)
    else:
        xe = x
    unit = 1.0
    if is_fp8(op) and self_quantizing(op):
        # the codes: x * wln * 448 / amax must lie on the e4m3 grid
        amax = xe.abs().max()
        codes = xe.double() * 448.0 / amax.double()
        e4m3_codes(codes)
        unit = (amax.double() / 448.0).item()      # dequant scale before rms
        xe = codes.to(dtype)
    dots = torch.empty(c.rows, dtype=dtype)
    bound = 0.0
    for r0 in range(0, c.rows, chunk):
        wr = c.w[r0:r0 + chunk].to(dtype)
        dots[r0:r0 + chunk] = wr @ xe
        bound = max(bound, (wr.abs() @ xe.abs()).max().item())
    y = dots * torch.tensor(unit * c.xs, dtype=dtype)
    if c.wsc is not None:
        y = y * c.wsc.to(dtype)
    if is_norm(op):
        eps = torch.tensor(EPS, dtype=torch.float32).to(dtype)
        rms = torch.rsqrt((x * x).sum() / c.K + eps)
        y = y * rms
    if is_gateup(op):
        gate, up = y[:c.N] * 2.0 ** -c.gate_shift, y[c.N:]
        if pre_activation:
            return gate, bound, dots
        y = gate / (1.0 + torch.exp(-gate)) * up
    if c.resid is not None:
        y = c.resid.to(dtype) + y
    return y, bound, dots


def fp8_norm_probe(c):
    """For a probe case of an fp8 norm-fused op, where the quantization
    decision sits on top of an inexact rms: (lo, hi, s) with lo/hi [K] the
    e4m3 grid points around the fp64 pre-quantization value
    v = x * wln * 448 / amax(x * wln) and s = amax * rms / 448 the fp64
    dequantization scale."""
    xe = c.x * c.wln
    amax = xe.abs().max()
    lo, hi = e4m3_bracket(xe * 448.0 / amax)
    eps = torch.tensor(EPS, dtype=torch.float32).double()
    rms = torch.rsqrt((c.x * c.x).sum() / c.K + eps)
    return lo, hi, (amax * rms / 448.0).item()


def fp8_norm_probe_violations(got, c):
    """Rows of a probe result that are not, to within one bf16 step, what
    either e4m3 neighbour of the selected element(s) gives."""
    lo, hi, s = fp8_norm_probe(c)
    g = got.reshape(-1).cpu().double()
    ok = torch.zeros(c.N, dtype=torch.bool)
    cg = c.cols[:c.N]
    for a in (lo, hi):
        if not is_gateup(c.op):
            cands = [a[cg] * s]
        else:
            gate = a[cg] * s
            silu = gate / (1.0 + torch.exp(-gate))
            cands = [silu * b[c.cols[c.N:]] * s for b in (lo, hi)]
        for cand in cands:
            ok |= (g - cand).abs() <= bf16_step(cand)
    return torch.nonzero(~ok).flatten()


def first_bad(bad, c):
    """Assertion text naming the first failing row (and, for a probe, the
    column(s) that row selects)."""
    n = int(bad[0])
    msg = f"{c.op} K={c.K} N={c.N}: {bad.numel()} rows wrong, first n={n}"
    if hasattr(c, "cols"):
        msg += f" (n, column) = ({n}, {int(c.cols[n])})"
        if is_gateup(c.op):
            msg += f", up column {int(c.cols[n + c.N])}"
    return msg


def head_rows(c, n):
    """The same problem restricted to its first n weight rows (ops without a
    gate_up weight or a residual)."""
    assert not is_gateup(c.op) and c.resid is None and n <= c.N
    d = Case(**c.__dict__)
    d.N = d.rows = n
    d.w = c.w[:n]
    if c.wsc is not None:
        d.wsc = c.wsc[:n]
    if hasattr(c, "cols"):
        d.cols = c.cols[:n]
    return d


def rope_geometry(n_min):
    """(hq, kh, hd, N): the smallest fused-qkv row count >= n_min that the
    RoPE-epilogue GEMV accepts, N == (hq + 2 * kh) * hd with hd == 16."""
    slots = max(3, -(-n_min // 16))
    return slots - 2, 1, 16, slots * 16


def quantizer_row():
    """One row holding every bf16 value in [-448, 448] (both zeros included),
    padded with zeros to a multiple of 8. Its amax is 448, so a rowwise e4m3
    quantizer finds the scale exactly 1."""
    top = torch.tensor(448.0).to(BF16).view(torch.int16).item()   # 0x43E0
    pos = torch.arange(top + 1, dtype=torch.int32)
    bits = torch.cat([pos, pos + 0x8000 - 0x10000]).to(torch.int16)
    row = bits.view(BF16)
    pad = (-row.numel()) % 8
    return torch.cat([row, torch.zeros(pad, dtype=BF16)])


def fold_negative_zero(codes):
    """e4m3 bytes with -0 (0x80) mapped to +0: the sign of a zero is the one
    thing two correct quantizers may differ in."""
    return torch.where(codes == 0x80, torch.zeros_like(codes), codes)
