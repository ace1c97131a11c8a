"""tests/lnbound.py tested on itself (CPU only): a float32 torch evaluation passes every check at every shape of tests/test_layernorm_forms.py, every planted fault is
flagged, and the whole-tensor norm of tests/test_rowops.py is set beside the same faults.

What the whole-tensor norm does with them (figures of `test_whole_tensor_norm_beside_the_element_bound`, bf16 dy):
  * one column missing from ONE row's mean_c g (the row's smallest |g|) moves the whole row by rstd |g| / C: |dx' - dx| / |dx| falls as 1 / (C sqrt(T)) -- 8.7e-7 at
    1024 x 4096, which PASSES the 2e-6 of test_layernorm_fwd_bwd, and 8.6e-6 at 16392 x 128, 3.7e-5 at 19 x 768, which fail it but pass every model-level tolerance
    (3e-2 .. 8e-2) by three orders of magnitude; the element bound sees it at 42 x (C = 4096) to 15000 x (C = 8) its size at any T;
  * one row missing from dgamma or dbeta is 1 / sqrt(T) of the norm: 0.23 at T = 19, 7.6e-3 at T = 16392.  That never passes 2e-6 -- the kernel-level norm catches a dropped
    row wherever a test REACHES the path that drops it -- but it passes the model-level tolerances from T of about 1100 rows on, which is every real batch; the element bound
    sees it at 32 x its size at T = 16392."""
import pytest
import torch

from tests import lnbound as L

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
SHAPES = [(L.T_RAGGED, C) for C in L.WIDTHS] + list(L.SMALL) + list(L.TALL) + [(21, 128), (21, 260), (21, 772)]


def _rel(a, b):      # tests/test_rowops.py
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _case(T, C, dy_dtype, **kw):
    inp = L.inputs(T, C, dy_dtype, seed=1000 * T + C, rps=7 if T == 21 else 0, **kw)
    ref = L.reference64(inp)
    B, e32 = L.bounds(inp, ref)
    return inp, ref, B, e32


def _flagged(got, inp, ref, B, e32, what):
    with pytest.raises(AssertionError):
        L.check_backward(got, inp, ref, B, e32, what)


@pytest.mark.parametrize("T,C", SHAPES)
def test_float32_evaluation_passes(T, C):
    for dy_dtype, out16 in ((BF, BF), (HF, HF), (F32, BF)):
        inp, ref, B, e32 = _case(T, C, dy_dtype)
        L.assert_sensitive(inp, ref, B, out16, colsum=True, what=f"{T} x {C}")
        ok = L.evaluate(inp, F32, out16)
        L.check_backward(ok, inp, ref, B, e32, f"float32 {T} x {C}")
        L.check_backward({**ok, "dx": None}, inp, ref, B, e32, f"float32 {T} x {C}, dx = NULL")          # the half-ulp rule against float64
    for kw in ({"dres": False}, {"dres": False, "dy_scale": True}, {"dres16": True}):
        inp, ref, B, e32 = _case(T, C, HF, **kw)
        L.assert_sensitive(inp, ref, B, HF, colsum=True, what=f"{T} x {C} {kw}")
        L.check_backward(L.evaluate(inp, F32, HF), inp, ref, B, e32, f"float32 {T} x {C} {kw}")


@pytest.mark.parametrize("T,C", [(L.T_RAGGED, 8), (L.T_RAGGED, 132), (L.T_RAGGED, 772), (L.T_RAGGED, 4096), (21, 128), (21, 772), (3, 260), (16392, 8), (16392, 128)])
@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_every_planted_fault_is_flagged(T, C, dtype):
    inp, ref, B, e32 = _case(T, C, dtype)
    for name in L.FAULTS:
        if name in ("colsum_before_scale", "row_scale_neighbour") and inp["rs"] is None:
            continue
        bad = L.plant(name, inp, dtype)
        _flagged(bad, inp, ref, B, e32, f"{name} {T} x {C}")
        if name in ("truncated_store", "row_scale_neighbour"):          # also without the kernel's own dx to compare with
            _flagged({**bad, "dx": None}, inp, ref, B, e32, f"{name} {T} x {C}, dx = NULL")
    # every row of the ragged tail and both sides of the block edge, not only the default place
    for r in sorted({0, T - 1, min(L.BLOCK_ROWS, T - 1), T // 2}):
        for name in ("mean_column_dropped", "dgamma_row_missing", "dbeta_row_missing", "colsum_row_missing"):
            if name == "colsum_row_missing" and inp["rs"] is not None and L.row_factor(inp)[r] == 0:
                continue
            _flagged(L.plant(name, inp, dtype, at=(r, C - 1)), inp, ref, B, e32, f"{name} row {r}")


def test_forward_checker():
    eps = 1e-6
    for T, C in ((L.T_RAGGED, 8), (L.T_RAGGED, 260), (L.T_RAGGED, 4096)):
        inp = L.inputs(T, C, BF, seed=T + C, far_rows=True)
        ref = L.forward64(inp, eps)
        B, e32 = L.forward_bounds(inp, ref, eps)
        L.check_forward(L.forward32(inp, eps), ref, B, e32, f"float32 forward {T} x {C}")
        with pytest.raises(AssertionError):          # E[x^2] - E[x]^2 in float32 on the rows whose mean is 100 standard deviations
            L.check_forward(L.forward32(inp, eps, one_pass=True), ref, B, e32, f"one-pass forward {T} x {C}")


def test_whole_tensor_norm_beside_the_element_bound():
    """see the module docstring: the figures are asserted here"""
    model_tol = 3e-2          # the tightest of tests/test_vit.py's whole-tensor tolerances
    for (T, C), col_passes_2e6 in (((19, 768), False), ((16392, 128), False), ((1024, 4096), True)):
        inp, ref, B, e32 = _case(T, C, BF)
        c = int((inp["dy"][T - 1].double() * inp["gamma"].double()).abs().argmin())          # the row's smallest contribution: the hardest column to miss
        bad = L.plant("mean_column_dropped", inp, at=(T - 1, c))
        rel = _rel(bad["dx"], ref["dx"])
        print(f"whole-tensor norm, one column out of one row's mean at {T} x {C}: {rel:.3e}")
        assert rel < model_tol and (rel < 2e-6) == col_passes_2e6
        _flagged(bad, inp, ref, B, e32, f"mean column {T} x {C}")
        for name, k in (("dgamma_row_missing", "dgamma"), ("dbeta_row_missing", "dbeta")):
            bad = L.plant(name, inp, at=(T - 1, 0))
            rel = _rel(bad[k], ref[k])
            print(f"whole-tensor norm, one row out of {k} at {T} x {C}: {rel:.3e} (1 / sqrt(T) = {T ** -0.5:.3e})")
            assert 0.5 * T ** -0.5 < rel < 2.0 * T ** -0.5 and (rel < model_tol) == (T > 2000)
            _flagged(bad, inp, ref, B, e32, f"{name} {T} x {C}")
