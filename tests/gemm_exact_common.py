"""Helpers shared by test_gemm_exact_cpu.py and test_gemm_exact_gpu.py: the
staging paths of the four prefill MFMA GEMMs (the two tile loops of
ops/hip/gemm_tiles.h, instantiated in gemm.hip and gemm_fp8.hip, and the bf16
256^2 loop written out in gemm256.hip), the shape lists that pin each of
them, inputs for which their fp32 accumulation is exact, references, and a
gather probe.
Everything here runs on the CPU and depends on torch alone."""

import functools

import torch

from gemv_exact_common import bf16_bracket, bracket_violations  # noqa: F401

BF16 = torch.bfloat16
F8 = torch.float8_e4m3fn

TILE128, TILE256, TILE_K = 128, 256, 64
EDGES = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 145)   # M and N values
E_CYCLE = (0, -2, 3)      # activation row m is scaled by 2^E_CYCLE[m % 3]
FP8_PIN = 448.0           # the e4m3 maximum: one per row fixes the row scale


# ---- the dispatch rule and the paths a shape takes ---------------------------

def dispatch256(M, N, K):
    """use_gemm256() in ops/hip/bindings.hip, which gemm() and gemm_fp8() both
    call: True -> the 256^2 8-phase kernel, False -> the 128^2 two-barrier
    kernel."""
    return M > 128 and N >= 256 and K >= 512 and K % 128 == 0


def paths128(M, N, K):
    """(triples, ntiles) of a 128^2 kernel (gemm_nt_kernel, gemm_fp8_kernel):
    the set of (a_edge, b_edge, k_edge) a stage() call sees anywhere in the
    grid, walking the kernels' own predicates per block and per K tile, and
    the K-tile count (1: no prefetch, 2: both buffers, 3: a buffer reused)."""
    ntiles = (K + TILE_K - 1) // TILE_K
    triples = set()
    for m0 in range(0, M, TILE128):
        a_edge = (M - m0) < TILE128
        for n0 in range(0, N, TILE128):
            b_edge = (N - n0) < TILE128
            for kt in range(ntiles):
                triples.add((a_edge, b_edge, (kt + 1) * TILE_K > K))
    return triples, ntiles


def paths256(M, N, K):
    """What a 256^2 kernel (gemm_nt256_kernel, gemm_fp8_256_kernel) meets at
    a shape: nt K-tiles (the main loop runs nt - 2 of them, two are peeled),
    whether any block clamps a source row of A (m_clamp) or of B (n_clamp),
    and whether some block has a [128][64] half-image made of clamped rows
    only (a_half: M - m0 <= 128, so rows 128..255 of the tile are all the
    last row of A; b_half likewise for B)."""
    assert K % 128 == 0 and K >= 512
    m_left = [M - m0 for m0 in range(0, M, TILE256)]
    n_left = [N - n0 for n0 in range(0, N, TILE256)]
    return {
        "nt": K // TILE_K,
        "m_clamp": any(v < TILE256 for v in m_left),
        "n_clamp": any(v < TILE256 for v in n_left),
        "a_half": any(v <= 128 for v in m_left),
        "b_half": any(v <= 128 for v in n_left),
    }


# ---- shape lists (M, N, K) --------------------------------------------------

# 128^2 bf16 kernel, forced with gemm_variant(a, b, 128). M and N each take
# every value of EDGES; K in {8, 56, 64, 72, 120, 128, 136, 200}.
SHAPES_128 = (
    (1, 1, 8), (15, 17, 56), (16, 16, 64), (17, 15, 72), (63, 65, 120),
    (64, 64, 128), (65, 63, 136), (127, 129, 200), (128, 128, 64),
    (128, 128, 72), (129, 127, 128), (1, 128, 64), (128, 1, 136),
    (16, 145, 8), (145, 16, 120),
    (145, 145, 136),   # an interior block and edge blocks in one grid
)
KS_128 = (8, 56, 64, 72, 120, 128, 136, 200)

# 256^2 kernels: gemm_variant(a, b, 256) takes all of them, gemm_fp8() sends
# the ones dispatch256() accepts to gemm_fp8_256_kernel.
SHAPES_256 = (
    (256, 256, 512), (257, 256, 640), (256, 257, 512), (129, 300, 512),
    (300, 129, 640), (1, 1, 512), (385, 511, 1024),
)
SHAPES_256_FP8 = tuple(s for s in SHAPES_256 if dispatch256(*s))
SHAPES_256_FP8_TO_128 = tuple(s for s in SHAPES_256 if not dispatch256(*s))

# one shape on each side of every clause of the rule
SHAPES_DISPATCH = (
    (128, 256, 512), (129, 256, 512), (129, 255, 512), (129, 256, 384),
    (129, 256, 576), (129, 256, 640),
)

# 128^2 fp8 kernel, reached through gemm_fp8(); K in {16, 48, 64, 80, 128,
# 144}, and one multi-block grid of full tiles (K = 576 keeps it off the
# 256^2 kernel, as does N < 256).
SHAPES_128_FP8 = (
    (1, 1, 16), (15, 17, 48), (16, 16, 64), (17, 15, 80), (63, 65, 128),
    (64, 64, 144), (65, 63, 16), (127, 129, 48), (128, 128, 64),
    (128, 128, 80), (129, 127, 128), (1, 128, 64), (128, 1, 144),
    (16, 145, 48), (145, 16, 80), (145, 145, 144),
    (256, 128, 576),
) + SHAPES_256_FP8_TO_128
KS_128_FP8 = (16, 48, 64, 80, 128, 144)

# device-quantized randn activations: one shape per fp8 kernel
SHAPES_FP8_RANDN = ((65, 129, 144), (257, 256, 640))


# ---- inputs ----------------------------------------------------------------

def _gen(*key):
    seed = 0
    for v in key:
        seed = seed * 1000003 + int(v)
    return torch.Generator().manual_seed(seed)


def _ints(shape, lim, g):
    return torch.randint(-lim, lim + 1, shape, generator=g)


def _exact(t, dtype):
    q = t.to(dtype)
    assert torch.equal(q.double(), t.double()), f"value not exact in {dtype}"
    return q


@functools.lru_cache(maxsize=None)
def bf16_case(M, N, K):
    """(A [M, K] bf16, B [N, K] bf16, expected [M, N] bf16, bound). A and B
    hold integers in [-8, 8]: every partial sum of a dot is an integer of
    magnitude <= bound = max sum_k |a b| <= 64 K, exact in fp32 in any order
    while below 2^24. expected is the exact integer result rounded once."""
    g = _gen(1, M, N, K)
    a, b = _ints((M, K), 8, g), _ints((N, K), 8, g)
    acc = a @ b.t()
    bound = int((a.abs() @ b.abs().t()).max())
    return (_exact(a, BF16), _exact(b, BF16), acc.float().to(BF16), bound)


def row_exponents(M):
    return torch.tensor(E_CYCLE)[torch.arange(M) % len(E_CYCLE)]


def wsc_pow2(N):
    """A power-of-two weight-row scale that varies with the row."""
    return torch.pow(2.0, ((torch.arange(N) % 5) - 2).double()).float()


def wsc_random(N):
    """Weight-row scales in [0.5, 2) with full fp32 mantissas."""
    return (0.5 + 1.5 * torch.rand(N, generator=_gen(3, N),
                                   dtype=torch.float64)).float()


@functools.lru_cache(maxsize=None)
def fp8_case(M, N, K):
    """(x [M, K] bf16, codes [M, K] int64, e [M], w [N, K] int64, acc [M, N]
    int64, bound).

    Row m of x is codes[m] * 2^e[m]: integers in [-8, 8] with one element
    +-448 at a random position, so the rowwise quantizer finds amax / 448 =
    2^e[m] exactly, its inverse exactly, and the e4m3 codes it writes are
    codes[m]. w holds the integer values of the weight codes, in [-8, 8].
    acc = codes @ w^T and bound = max sum_k |codes w| < 2^24."""
    g = _gen(2, M, N, K)
    codes = _ints((M, K), 8, g)
    pin = torch.randint(0, K, (M,), generator=g)
    sign = torch.randint(0, 2, (M,), generator=g) * 2 - 1
    codes[torch.arange(M), pin] = sign * int(FP8_PIN)
    e = row_exponents(M)
    x = _exact(codes.double() * torch.pow(2.0, e.double())[:, None], BF16)
    w = _ints((N, K), 8, g)
    acc = codes @ w.t()
    bound = int((codes.abs() @ w.abs().t()).max())
    return x, codes, e, w, acc, bound


def e4m3_bytes(vals):
    """The e4m3fn bytes of values that lie on the grid (asserted)."""
    return _exact(vals.float(), F8).view(torch.uint8)


def fp8_expected(acc, e, wsc):
    """fp64 value of acc[m, n] * 2^e[m] * wsc[n] — what the epilogue computes
    with two fp32 products before its bf16 store."""
    return (acc.double() * torch.pow(2.0, e.double())[:, None]
            * wsc.double()[None, :])


def fp8_exact_expected(acc, e, wsc):
    """The bf16 result for power-of-two wsc: both fp32 products are exact,
    so the store is the one rounding of an exact value."""
    v = fp8_expected(acc, e, wsc)
    assert torch.equal(v.float().double(), v), "not exact in fp32"
    return v.float().to(BF16)


@functools.lru_cache(maxsize=None)
def fp8_randn_case(M, N, K):
    """(x [M, K] bf16 randn, w [N, K] int64 in {-1, 0, 1}, one in eight
    nonzero). Whatever codes a rowwise e4m3 quantizer gives x are multiples
    of 2^-9 of magnitude <= 448; the sparse unit weights keep sum_k |code w|
    below 2^15, so every partial sum is a multiple of 2^-9 below 2^24 * 2^-9
    and the fp32 accumulation is exact (randn_premise checks it on the codes
    actually used)."""
    g = _gen(4, M, N, K)
    x = torch.randn(M, K, generator=g).to(BF16)
    sign = torch.randint(0, 2, (N, K), generator=g) * 2 - 1
    w = sign * (torch.rand(N, K, generator=g) < 0.125)
    return x, w


def randn_premise(xcodes64, w):
    """max over outputs of sum_k |code w|, in units of 2^-9 (the e4m3
    subnormal step, which every code is a multiple of): below 2^24 the fp32
    accumulation is exact in any order."""
    assert torch.equal(torch.round(xcodes64 * 512.0), xcodes64 * 512.0)
    return float((xcodes64.abs() @ w.abs().double().t()).max()) * 512.0


# ---- gather probe ------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def probe_case(M, N, K):
    """(A [M, K] bf16, B [N, K] bf16, perm [K]). B[n] is one-hot at column
    perm[n % K], so C[m, n] must be A[m, perm[n % K]] and every output names
    the one k it read. A[m, k] = ((3 m + 5 k + 7 m (k // 251)) % 251) - 125:
    columns less than 251 apart differ in every row, columns a multiple of
    251 apart differ in every row but m = 0 (mod 251)."""
    perm = torch.randperm(K, generator=_gen(5, K))
    m = torch.arange(M)[:, None]
    k = torch.arange(K)[None, :]
    a = ((3 * m + 5 * k + 7 * m * (k // 251)) % 251) - 125
    assert int(a.abs().max()) <= 128
    b = torch.zeros(N, K, dtype=torch.int64)
    b[torch.arange(N), perm[torch.arange(N) % K]] = 1
    return _exact(a, BF16), _exact(b, BF16), perm


def probe_expected(a, perm, N):
    return a[:, perm[torch.arange(N) % perm.numel()]]


def probe_mismatch(got, a, perm):
    """None if got [M, N] is the gather of a by perm; otherwise a message
    naming the first wrong (m, n), the k it should have read and the k whose
    value it holds (the column of a equal to the whole output column where
    there is one, else a k that matches in row m, else none)."""
    got = got.cpu()
    N = got.shape[1]
    want = probe_expected(a, perm, N)
    bad = torch.nonzero(got.float() != want.float())
    if bad.numel() == 0:
        return None
    m, n = (int(v) for v in bad[0])
    k_want = int(perm[n % perm.numel()])
    col = (a.float() == got[:, n:n + 1].float()).all(dim=0)
    row = a[m].float() == got[m, n].float()
    if col.any():
        found = f"holds column k={int(torch.nonzero(col)[0])} of A"
    elif row.any():
        ks = [int(v) for v in torch.nonzero(row).flatten()[:4]]
        found = f"holds A[{m}, k] for k in {ks}"
    else:
        found = "holds the value of no single k"
    return (f"{bad.shape[0]} of {got.numel()} outputs wrong, first (m, n) = "
            f"({m}, {n}): got {float(got[m, n])}, expected A[{m}, {k_want}] = "
            f"{float(want[m, n])}; {found}")


def first_mismatch(got, want, what):
    """Assertion text for a bit-exact comparison that failed."""
    got, want = got.cpu(), want.cpu()
    bad = torch.nonzero(got.float() != want.float())
    if bad.numel() == 0:      # differ only in a NaN or the sign of a zero
        bad = torch.nonzero(got.view(torch.int16) != want.view(torch.int16))
    m, n = (int(v) for v in bad[0])
    return (f"{what}: {bad.shape[0]} of {got.numel()} outputs wrong, first "
            f"(m, n) = ({m}, {n}): got {float(got[m, n])}, expected "
            f"{float(want[m, n])}")


def bracket_message(got, ref64, what):
    """None if every element of got is one of the two bf16 neighbours of
    ref64, otherwise the assertion text."""
    bad = bracket_violations(got, ref64)
    if bad.numel() == 0:
        return None
    i = int(bad[0])
    m, n = divmod(i, got.shape[1])
    return (f"{what}: {bad.numel()} of {got.numel()} outputs off the bracket, "
            f"first (m, n) = ({m}, {n}): got {float(got.reshape(-1)[i])}, "
            f"fp64 value {float(ref64.reshape(-1)[i])}")


# ---- guarded operands --------------------------------------------------------

def guarded_rows(t, fill, guard):
    """t [R, C] as the interior row-slice of a parent with `guard` rows of
    `fill` on either side: (parent, slice). The slice is contiguous and, as
    guard * C elements are a multiple of 16 bytes here, 16-byte aligned."""
    R, C = t.shape
    parent = torch.full((R + 2 * guard, C), fill, dtype=t.dtype)
    parent[guard:guard + R] = t
    return parent, parent[guard:guard + R]
