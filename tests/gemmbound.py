"""TEST INFRASTRUCTURE: bit-exact and per-element checks for the GEMM kernels (tests/test_gemm_exact.py, tests/test_gemm_elements.py; tested on itself by
tests/test_gemmbound.py).  The counterpart of tests/rowbound.py and tests/headbound.py for csrc/gemm.hip, gemm_w4.hip, gemm_f32.hip and gemm_fp8.hip.

A whole-tensor Frobenius ratio over Gaussian operands cannot see one zeroed 8-element store, one k index missing from a 32x32 sub-tile or a truncating 16-bit store
under the 3e-3 / 4e-3 bounds of every 16-bit output (tests/test_gemmbound.py shows the three passing).  This module supplies two families of checks that can:

  * EXACT.  Operands drawn from {+-1, +-2, +-3} (`exact_operands`): every product is an integer of at most 9, every partial sum in ANY order -- across tiles, k-tile
    pairs, split-K slabs, stream-K partials -- is an integer below 9 K < 2^24 and therefore exact in the fp32 accumulator.  The correct result is ONE bit pattern per
    element; a dropped, duplicated or misplaced product moves that element by at least 1.  The epilogue operands (`exact_bias`, `exact_residual`, `exact_col_scale`,
    `exact_row_scale`, alpha in {1, 0.5}) keep every intermediate of the epilogue exact in fp32 (`expected` asserts it step by step, so that a contracted fma and
    separate instructions agree), and a 16-bit output is the single round-to-nearest-even of an exact value.  `check_exact` compares bit patterns and names the
    256x256 tile and the 32x32 sub-tile of the first difference.
  * GELU-class epilogues on an exact pre-activation (B scaled by 2^-4: u = acc / 16 + bias is exact and spreads over GELU's curved range): the saved pre-activation is
    bit-exact; what passes through erf / exp obeys the HALF-ULP RULE `check_half_ulp`: |got - g64| <= |RNE16(g64) - g64| + slack, i.e. got is the round-to-nearest
    of some value within `slack` of the float64 result.  slack = LSE_FACTOR x max(E32, eps32 |g64|) (`act_slack`), E32 = the worst absolute error of torch's float32
    evaluation of the same quantity against float64 on the same inputs -- from torch alone, never from a kernel; LSE_FACTOR (8) is rowbound.py's: fast erf / exp in
    another evaluation order against torch's.
  * ARITHMETIC.  Gaussian operands, for what integers cannot show (a slab or partial kept in 16 bits, an fp16 accumulator, a wrong rounding mode).  The unit is
    S = |alpha| |A| |B|^T (+ |bias| + |residual|) per element (`arith_unit`); an fp32 output obeys |got - ref64| <= 2 (K + 4) 2^-24 S (`arith_bound`): the a-priori bound
    of any fp32 accumulation of K products (K roundings of at most 2^-24 of the running sum of absolute values; + 4 for alpha, bias, residual and the store), doubled
    for accumulator adds that need not round to nearest.  A derived condition, not a measurement.  16-bit outputs: the half-ulp rule with that bound as the slack.

`plant` applies the faults of the self-test to a correct result."""
from __future__ import annotations

import math

import torch

from tests.rowbound import LSE_FACTOR

EPS32 = torch.finfo(torch.float32).eps
U32 = 2.0 ** -24
TILE, SUB = 256, 32
VALUES = (-3.0, -2.0, -1.0, 1.0, 2.0, 3.0)
COL_SCALES = (2.0 ** -20, 0.5, 1.0, 2.0)         # 2^-20 stands for ConvNeXt's 1e-6-class gamma
ROW_SCALES = (0.0, 1.0, 1.25)
GELU_SHIFT = 4                                   # B x 2^-4 for the GELU-class cases
GELU_GRAD_MAX = 1.13                             # max |GELU'| (1.129 at u = sqrt(2)): GELU's Lipschitz constant


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _pick(values, shape, g):
    return torch.tensor(values, dtype=torch.float64)[torch.randint(0, len(values), shape, generator=g)]


# ---------------------------------------------------------------------------------------------------------------- exact family: operands
def exact_operands(M, N, K, dtype, seed, b_shift=0):
    """-> (a [M, K], b [N, K]) in `dtype` (bf16, fp16, fp32, float8_e4m3fn, float8_e5m2) with entries from {+-1, +-2, +-3} -- never a zero, so every product counts --,
    b times 2^-b_shift.  All of these are exact in every one of the formats."""
    g = _gen(seed)
    a = _pick(VALUES, (M, K), g)
    b = _pick(VALUES, (N, K), g) * 2.0 ** -b_shift
    ad, bd = a.float().to(dtype), b.float().to(dtype)
    assert torch.equal(ad.double(), a) and torch.equal(bd.double(), b), "operand values are not exact in " + str(dtype)
    return ad, bd


def exact_bias(N, seed):
    """integer bias in [-8, 8], float32 [N]"""
    return torch.randint(-8, 9, (N,), generator=_gen(seed + 101)).float()


def exact_residual(M, N, seed):
    """multiples of 0.25 in [-4, 4], float32 [M, N]"""
    return torch.randint(-16, 17, (M, N), generator=_gen(seed + 202)).float() * 0.25


def exact_col_scale(N, seed):
    return _pick(COL_SCALES, (N,), _gen(seed + 303)).float()


def exact_row_scale(n, seed):
    """one factor per sample from {0, 1, 1.25}; neighbours differ (entry i is never entry i - 1), so that a factor taken from the neighbouring sample shows"""
    g = _gen(seed + 404)
    idx = torch.randint(0, 3, (n,), generator=g)
    for i in range(1, n):
        if idx[i] == idx[i - 1]:
            idx[i] = (idx[i] + 1 + int(torch.randint(0, 2, (1,), generator=g))) % 3
    return torch.tensor(ROW_SCALES, dtype=torch.float32)[idx]


# ---------------------------------------------------------------------------------------------------------------- exact family: expected results
def assert_f32_exact(x64, what):
    assert torch.equal(x64.float().double(), x64), f"{what}: not exactly representable in fp32 (the case's operands must keep it exact)"


def acc_exact(a, b, b_kmajor=False, a_kmajor=False, b_shift=0):
    """float64 product a . b^T of exact operands ([M, K] x [N, K]; *_kmajor: the operand lies as [K, .]).  Asserts that every sum of absolute values stays below 2^24
    units of 2^-b_shift (|acc| <= 9 K), i.e. every partial sum in any order is exact in an fp32 accumulator; float64 holds integers below 2^53 exactly, so this IS the
    integer result."""
    A = a.double().cpu().t() if a_kmajor else a.double().cpu()
    B = b.double().cpu() if b_kmajor else b.double().cpu().t()
    K = A.shape[1]
    unit = 2.0 ** -b_shift
    assert float(A.abs().max()) <= 3.0 and float(B.abs().max()) <= 3.0 * unit and 9 * K < 2 ** 24, "operands outside the exact family"
    acc = A @ B
    assert torch.equal(acc / unit, torch.round(acc / unit)) and float(acc.abs().max()) <= 9.0 * K * unit
    assert_f32_exact(acc, "accumulator")
    return acc


def epilogue_exact(acc, *, alpha=1.0, col_scale=None, bias=None, row_scale=None, rows_per_scale=0, residual=None):
    """float64 C = residual + row_scale[m // rows_per_scale] * (alpha * acc * col_scale + bias), the order of include/visiondk.h, with every intermediate asserted to be
    exact in fp32 -- the result then does not depend on which of the steps a compiler contracts into an fma"""
    v = acc * alpha
    assert_f32_exact(v, "alpha * acc")
    if col_scale is not None:
        v = v * col_scale.double().cpu()
        assert_f32_exact(v, "acc * col_scale")
    if bias is not None:
        v = v + bias.double().cpu()
        assert_f32_exact(v, "+ bias")
    if row_scale is not None:
        rows = torch.arange(v.shape[0]) // rows_per_scale
        v = v * row_scale.double().cpu()[rows][:, None]
        assert_f32_exact(v, "* row_scale")
    if residual is not None:
        v = v + residual.double().cpu()
        assert_f32_exact(v, "+ residual")
    return v


def to_out(x64, dtype):
    """an fp32-exact float64 tensor in the output format: itself in fp32, its single round-to-nearest-even in a 16-bit format"""
    assert_f32_exact(x64, "expected result")
    return x64.float() if dtype == torch.float32 else x64.float().to(dtype)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def where(row, col):
    """the 256x256 tile and the 32x32 sub-tile (inside that tile) that hold (row, col)"""
    return (row // TILE, col // TILE), ((row % TILE) // SUB, (col % TILE) // SUB)


def check_exact(got, want, what=""):
    """bit patterns equal; on failure: the number of differing elements, the first (row, col), its 256x256 tile and its 32x32 sub-tile"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    diff = bits(got) != bits(want)
    n = int(diff.sum())
    if n == 0:
        return
    if diff.dim() != 2:
        diff = diff.reshape(-1, diff.shape[-1])
        got, want = got.reshape(diff.shape), want.reshape(diff.shape)
    r, c = (int(x) for x in torch.nonzero(diff)[0])
    tile, sub = where(r, c)
    raise AssertionError(f"{what}: {n} of {diff.numel()} elements differ in their bits; first at (row {r}, col {c}) = tile {tile}, 32x32 sub-tile {sub}: "
                         f"got {float(got[r, c])!r}, want {float(want[r, c])!r}; {int(diff.any(1).sum())} rows, {int(diff.any(0).sum())} columns touched")


# ---------------------------------------------------------------------------------------------------------------- the half-ulp rule
def half_ulp_distance(x64, dtype):
    """|RNE16(x) - x| in float64: the distance from x to the nearest value of the 16-bit format.  (torch converts float64 through float32, which can round twice; the
    minimum over the converted value and its two neighbours in the format is the true nearest.)"""
    t = x64.float().to(dtype)
    b = t.view(torch.int16)
    d = (t.double() - x64).abs()
    mag = b & 0x7FFF
    up = (b + 1).view(dtype).double()                                   # next larger magnitude
    d = torch.minimum(d, torch.where(mag < 0x7F7F if dtype == torch.bfloat16 else mag < 0x7BFF, (up - x64).abs(), d))
    dn = torch.where(mag > 0, b - 1, b).view(dtype).double()            # next smaller magnitude
    return torch.minimum(d, (dn - x64).abs())


def _worst(ratio):
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    i = int(ratio.argmax())
    return float(ratio.reshape(-1)[i]), tuple(int(x) for x in torch.unravel_index(torch.tensor(i), ratio.shape))


def _check(err, bound, what, label):
    """assert err <= bound element-wise; prints and returns the worst err / bound (0 / 0 counts as 0)"""
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    m, at = _worst(ratio)
    print(f"gemm {what} {label}: worst |err| / bound {m:.3f} at {at} (|err| {float(err[at]):.3e}, bound {float(bound[at]):.3e})")
    if not m <= 1.0:
        tile, sub = where(at[-2], at[-1]) if len(at) >= 2 else ((0, 0), (0, 0))
        raise AssertionError(f"{what} {label}: {int((ratio > 1).sum())} elements beyond their bound, worst {m:.3f} x at {at} = tile {tile}, 32x32 sub-tile {sub}: "
                             f"|err| {float(err[at]):.3e}, bound {float(bound[at]):.3e}")
    return m


def check_half_ulp(got, g64, slack, what=""):
    """16-bit `got`: |got - g64| <= |RNE16(g64) - g64| + slack element-wise -- got is the round-to-nearest of a value within slack of g64"""
    assert got.dtype in (torch.bfloat16, torch.float16) and got.shape == g64.shape
    err = (got.detach().cpu().double() - g64).abs()
    return _check(err, half_ulp_distance(g64, got.dtype) + slack, what, "half-ulp rule")


def check_within(got, g64, slack, what=""):
    """fp32 `got`: |got - g64| <= slack element-wise"""
    assert got.dtype == torch.float32 and got.shape == g64.shape
    return _check((got.detach().cpu().double() - g64).abs(), slack + torch.zeros_like(g64), what, "fp32 bound")


def act_slack(f32, g64):
    """LSE_FACTOR x max(E32, eps32 |g64|) element-wise; E32 = max |f32 - g64|, f32 = torch's float32 evaluation of the quantity whose float64 value is g64.
    -> (slack, E32)"""
    e32 = float((f32.double() - g64).abs().max())
    return LSE_FACTOR * torch.maximum(torch.full_like(g64, e32), EPS32 * g64.abs()), e32


def gelu(x):
    return torch.nn.functional.gelu(x)


def gelu_grad(x):
    """torch's autograd derivative of its exact-erf GELU, in the dtype of x"""
    xx = x.detach().clone().requires_grad_(True)
    torch.nn.functional.gelu(xx).sum().backward()
    return xx.grad


# ---------------------------------------------------------------------------------------------------------------- arithmetic family
def arith_unit(a, b, alpha=1.0, bias=None, residual=None, b_kmajor=False, a_kmajor=False):
    """S = |alpha| |A| |B|^T (+ |bias| + |residual|) per element, float64"""
    A = a.double().cpu().t() if a_kmajor else a.double().cpu()
    B = b.double().cpu() if b_kmajor else b.double().cpu().t()
    S = abs(alpha) * (A.abs() @ B.abs())
    if bias is not None:
        S = S + bias.double().cpu().abs()
    if residual is not None:
        S = S + residual.double().cpu().abs()
    return S


def arith_bound(S, K):
    return 2.0 * (K + 4) * U32 * S


def check_arith(got, ref64, S, K, what="", extra=None):
    """fp32 output: |got - ref64| <= 2 (K + 4) 2^-24 S; 16-bit output: the half-ulp rule with that bound as the slack.  `extra`: added to the slack (the activation's own
    slack where one follows the accumulation).  Prints and returns the worst ratio to the bound."""
    slack = arith_bound(S, K) if extra is None else arith_bound(S, K) + extra
    if got.dtype == torch.float32:
        return check_within(got, ref64, slack, what)
    return check_half_ulp(got, ref64, slack, what)


# ---------------------------------------------------------------------------------------------------------------- planted faults (self-test)
FAULTS = ("store8_zeroed", "product_dropped", "k_dropped_subtile", "row_shifted_32", "column_duplicated", "truncated_store", "slab_rounded_bf16", "bias_missing_column",
          "row_scale_neighbour")


def plant(name, a, b, *, out_dtype=torch.float32, bias=None, residual=None, row_scale=None, rows_per_scale=0, splits=1, at=(300, 264)):
    """the result of C = residual + row_scale * (a . b^T + bias) in `out_dtype` -- products and sums in float64, ONE rounding at the end -- with the fault `name` applied
    where it arises: at element / sub-tile / row / column `at` = (row, col).  a [M, K], b [N, K]."""
    A, B = a.double().cpu(), b.double().cpu()
    M, K = A.shape
    N = B.shape[0]
    r, c = at
    r0, c0 = r // SUB * SUB, c // SUB * SUB
    assert name in FAULTS and r + SUB < M and c + 8 < N
    acc = A @ B.t()
    if name == "product_dropped":
        acc[r, c] -= A[r, 5] * B[c, 5]
    elif name == "k_dropped_subtile":
        acc[r0:r0 + SUB, c0:c0 + SUB] -= A[r0:r0 + SUB, 5:6] @ B[c0:c0 + SUB, 5:6].t()
    elif name == "slab_rounded_bf16":
        assert splits > 1
        kc = (K + splits - 1) // splits
        acc = sum(((A[:, s:s + kc] @ B[:, s:s + kc].t()).float().bfloat16().double() if s == kc else A[:, s:s + kc] @ B[:, s:s + kc].t()) for s in range(0, K, kc))
    v = acc
    if bias is not None:
        bb = bias.double().cpu().clone()
        if name == "bias_missing_column":
            assert bb[c] != 0
            bb[c] = 0.0
        v = v + bb
    else:
        assert name != "bias_missing_column"
    if row_scale is not None:
        rs = row_scale.double().cpu()
        idx = torch.arange(M) // rows_per_scale
        if name == "row_scale_neighbour":
            s = r // rows_per_scale
            assert rs[s] != rs[s - 1]
            idx[idx == s] = s - 1
        v = v * rs[idx][:, None]
    else:
        assert name != "row_scale_neighbour"
    if residual is not None:
        v = v + residual.double().cpu()
    if name == "truncated_store":
        assert out_dtype == torch.bfloat16
        out = (v.float().view(torch.int32) & -65536).view(torch.float32).bfloat16()         # round toward zero: the low 16 bits dropped
    else:
        out = v.float() if out_dtype == torch.float32 else v.float().to(out_dtype)
    if name == "store8_zeroed":
        out[r, c // 8 * 8:c // 8 * 8 + 8] = 0
    elif name == "row_shifted_32":
        out[r + SUB] = out[r].clone()
    elif name == "column_duplicated":
        out[:, c + 1] = out[:, c].clone()
    return out
