"""The GEMM checks of tests/gemmbound.py, tested on themselves (CPU only, no kernel): every planted fault fails the check it belongs to, the unfaulted reference
passes all of them, and the first three faults pass the whole-tensor ratio `_rel(...) < 4e-3` of tests/test_gemm.py -- the gap the element-wise checks close."""
import pytest
import torch

from tests import gemmbound as gb

M, N, K = 1300, 776, 256          # the suite's own ragged walk shape
SEED = 20
RPS = 49


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


@pytest.fixture(scope="module")
def exact():
    a, b = gb.exact_operands(M, N, K, torch.bfloat16, SEED)
    return dict(a=a, b=b, acc=gb.acc_exact(a, b), bias=gb.exact_bias(N, SEED), res=gb.exact_residual(M, N, SEED), rs=gb.exact_row_scale((M + RPS - 1) // RPS, SEED))


@pytest.fixture(scope="module")
def gauss():
    g = torch.Generator().manual_seed(SEED)
    a = torch.randn(M, K, generator=g).bfloat16(); b = torch.randn(N, K, generator=g).bfloat16()
    return dict(a=a, b=b, ref64=a.double() @ b.double().t(), S=gb.arith_unit(a, b))


def _fails(name, fn):
    with pytest.raises(AssertionError) as e:
        fn()
    print(f"planted fault {name}: caught -- {str(e.value)[:200]}")


def test_exact_operands_have_no_zero_and_fit_every_format():
    for dt in (torch.bfloat16, torch.float16, torch.float32, torch.float8_e4m3fn, torch.float8_e5m2):
        a, b = gb.exact_operands(40, 24, 64, dt, 3, b_shift=gb.GELU_SHIFT)
        assert set(a.float().abs().unique().tolist()) == {1.0, 2.0, 3.0} and set((b.float().abs() * 16).unique().tolist()) == {1.0, 2.0, 3.0}
    assert set(gb.exact_col_scale(4000, 1).tolist()) == set(gb.COL_SCALES) and set(gb.exact_bias(4000, 1).tolist()) == set(float(i) for i in range(-8, 9))
    rs = gb.exact_row_scale(200, 1)
    assert set(rs.tolist()) == {0.0, 1.0, 1.25} and bool((rs[1:] != rs[:-1]).all())


def test_expected_results_are_exact_and_inexact_epilogues_are_refused(exact):
    acc = exact["acc"]
    assert float(acc.abs().max()) <= 9 * K
    cs = gb.exact_col_scale(N, SEED)
    gb.to_out(gb.epilogue_exact(acc, col_scale=cs, bias=exact["bias"], residual=exact["res"]), torch.float32)
    gb.to_out(gb.epilogue_exact(acc, alpha=0.5, bias=exact["bias"], row_scale=exact["rs"], rows_per_scale=RPS, residual=exact["res"]), torch.float32)
    with pytest.raises(AssertionError):       # 2^-21 under a bias of 8 and a factor 1.25 needs more than 24 bits
        gb.epilogue_exact(acc, alpha=0.5, col_scale=torch.full((N,), 2.0 ** -20), bias=torch.full((N,), 8.0), row_scale=torch.full_like(exact["rs"], 1.25), rows_per_scale=RPS)
    with pytest.raises(AssertionError):       # Gaussian operands are not in the family
        gb.acc_exact(torch.randn(8, 8), torch.randn(8, 8))


@pytest.mark.parametrize("fault", ["store8_zeroed", "product_dropped", "k_dropped_subtile", "row_shifted_32", "column_duplicated"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_exact_check_catches_misplaced_and_missing_products(exact, fault, dtype):
    want = gb.to_out(exact["acc"], dtype)
    _fails(fault, lambda: gb.check_exact(gb.plant(fault, exact["a"], exact["b"], out_dtype=dtype), want, fault))


def test_exact_check_reports_tile_and_subtile(exact):
    want = gb.to_out(exact["acc"], torch.float32)
    with pytest.raises(AssertionError) as e:
        gb.check_exact(gb.plant("k_dropped_subtile", exact["a"], exact["b"], at=(300, 264)), want, "report")
    msg = str(e.value)
    assert "1024 of" in msg and "(row 288, col 256)" in msg and "tile (1, 1)" in msg and "sub-tile (1, 0)" in msg


def test_exact_check_catches_truncation_bias_and_row_scale(exact):
    a, b, bias, res, rs = exact["a"], exact["b"], exact["bias"], exact["res"], exact["rs"]
    want16 = gb.to_out(exact["acc"], torch.bfloat16)
    _fails("truncated_store", lambda: gb.check_exact(gb.plant("truncated_store", a, b, out_dtype=torch.bfloat16), want16, "truncated_store"))
    # (a slab of K / 3 integer products seldom leaves bf16's exact integers, |sum| <= 256: slab rounding belongs to the arithmetic check below)
    col = int(torch.nonzero(bias)[40])
    wantb = gb.to_out(gb.epilogue_exact(exact["acc"], bias=bias), torch.bfloat16)
    gb.check_exact(gb.plant("product_dropped", a, b, out_dtype=torch.bfloat16, bias=bias)[:200], wantb[:200], "rows above the fault")
    _fails("bias_missing_column", lambda: gb.check_exact(gb.plant("bias_missing_column", a, b, out_dtype=torch.bfloat16, bias=bias, at=(300, col)), wantb, "bias_missing_column"))
    wantr = gb.to_out(gb.epilogue_exact(exact["acc"], bias=bias, row_scale=rs, rows_per_scale=RPS, residual=res), torch.float32)
    _fails("row_scale_neighbour", lambda: gb.check_exact(gb.plant("row_scale_neighbour", a, b, bias=bias, residual=res, row_scale=rs, rows_per_scale=RPS), wantr, "row_scale_neighbour"))


def test_unfaulted_reference_passes_every_check(exact, gauss):
    a, b, ref64, S = gauss["a"], gauss["b"], gauss["ref64"], gauss["S"]
    f32 = a.float() @ b.float().t()                                   # torch's own fp32 accumulation: another correct order
    assert gb.check_arith(f32, ref64, S, K, "torch fp32") < 0.25
    assert gb.check_arith(f32.bfloat16(), ref64, S, K, "torch fp32 -> bf16") <= 1.0
    assert gb.check_arith(f32.half(), ref64, S, K, "torch fp32 -> fp16") <= 1.0
    # the GELU-class rules on an exact pre-activation, with torch's float32 evaluation standing in for a kernel
    ag, bg = gb.exact_operands(M, N, K, torch.bfloat16, SEED, b_shift=gb.GELU_SHIFT)
    u = gb.epilogue_exact(gb.acc_exact(ag, bg, b_shift=gb.GELU_SHIFT), bias=exact["bias"])
    g64 = gb.gelu(u)
    slack, e32 = gb.act_slack(gb.gelu(u.float()), g64)
    assert 0 < e32 < 2e-6
    gb.check_half_ulp(gb.gelu(u.float()).bfloat16(), g64, slack, "torch gelu -> bf16")
    gb.check_within(gb.gelu(u.float()), g64, slack, "torch gelu fp32")
    d64 = gb.gelu_grad(u)
    slack, _ = gb.act_slack(gb.gelu_grad(u.float()), d64)
    gb.check_half_ulp(gb.gelu_grad(u.float()).half(), d64, slack, "torch gelu' -> fp16")
    slack, _ = gb.act_slack(gb.gelu(u.float()), g64)
    trunc = (gb.gelu(u.float()).view(torch.int32) & -65536).view(torch.float32).bfloat16()
    _fails("gelu stored by truncation", lambda: gb.check_half_ulp(trunc, g64, slack, "truncated gelu"))
    _fails("tanh-approximated gelu", lambda: gb.check_half_ulp(torch.nn.functional.gelu(u.float(), approximate="tanh").bfloat16(), g64, slack, "tanh gelu"))


def test_half_ulp_distance_is_to_the_nearest_16_bit_value():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -9, 257.0, -3.5, 0.0, 1.0 + 2.0 ** -8 + 2.0 ** -30], dtype=torch.float64)
    d = gb.half_ulp_distance(x, torch.bfloat16)
    assert d.tolist() == [0.0, 2.0 ** -8, 2.0 ** -9, 1.0, 0.0, 0.0, 2.0 ** -8 - 2.0 ** -30]      # the last one rounds twice through float32


@pytest.mark.parametrize("fault", ["store8_zeroed", "k_dropped_subtile", "truncated_store", "slab_rounded_bf16", "row_shifted_32", "column_duplicated"])
def test_arithmetic_check_catches(gauss, fault):
    a, b, ref64, S = gauss["a"], gauss["b"], gauss["ref64"], gauss["S"]
    dtype = torch.float32 if fault == "slab_rounded_bf16" else torch.bfloat16
    _fails(fault, lambda: gb.check_arith(gb.plant(fault, a, b, out_dtype=dtype, splits=3), ref64, S, K, fault))


@pytest.mark.parametrize("fault", ["store8_zeroed", "product_dropped", "k_dropped_subtile"])
def test_whole_tensor_ratio_does_not_see_the_first_three_faults(gauss, fault):
    """what tests/test_gemm.py asserts of every 16-bit output: Gaussian bf16 operands, the result rounded to bf16, one Frobenius ratio < 4e-3 (on this seed)"""
    a, b = gauss["a"], gauss["b"]
    ref = a.float() @ b.float().t()
    bad = gb.plant(fault, a, b, out_dtype=torch.bfloat16)
    r = _rel(bad.float(), ref)
    print(f"planted fault {fault}: whole-tensor ratio {r:.2e} < 4e-3, unfaulted {_rel(ref.bfloat16().float(), ref):.2e}")
    assert r < 4e-3
    assert _rel(gb.plant("truncated_store", a, b, out_dtype=torch.bfloat16).float(), ref) < 4.5e-3      # truncation: only just beyond it
