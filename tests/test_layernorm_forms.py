"""Every form of ln_bwd_kernel that ln_bwd_impl can launch (csrc/norm_loss.hip), element by element against float64 (tests/lnbound.py): the plain forms through the public
vdk_layernorm_bwd, the forms only the engines reach (column sums of the stored 16-bit copy, its fp8 copy and amax, the 16-bit residual gradient, dy_scale, the stochastic-depth
factor of the copy, the deferred dgamma | dbeta job) through the test-only vdk_debug_layernorm_bwd_forms, the column-sum pass with its fp8 copy through vdk_debug_colsum16_q8,
and the forward on the same grid.  Outputs start out as NaN; every call is made twice and must give the same bits (every reduction here has a fixed order).

Which instantiation a case reaches (MAXJ, rows per wave): C <= 128: 1, 2 x 2 (HALF); <= 256: 1, 2; <= 512: 2, 2; <= 768: 3, 1; <= 1024: 4, 1; else 16, 1 (no column sums);
the fp8 copy and dres16: MAXJ 3 (C <= 768) or 4.  Blocks hold at most 16 rows until T passes 16 x 1024 and ln_bwd_blocks evens them out: T = 19 is blocks of 10 and 9 rows (a
wave's ragged pass reaches into the next block's rows, `row < r1`), T = 21 blocks of 11 and 10 (the edge inside the second of three 7-row samples), and T = 16392 gives 965
blocks of 17 rows: a HALF wave's second pass holds one row and its odd half-wave sees the next block's row."""
import ctypes as C
import functools

import pytest
import torch

from tests import gemmbound
from tests import lnbound as L
from visiondk_amd import _abi, ops

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
IDS = {BF: "bf16", HF: "fp16", F32: "f32"}
DT = {BF: _abi.BF16, HF: _abi.F16_, F32: _abi.F32_}
EINVAL = -1
T0 = L.T_RAGGED


@functools.lru_cache(maxsize=None)
def case(T, Cc, dy_dtype, out16, colsum=False, **kw):
    """inputs, float64 reference, bounds (and the preconditions, asserted from float64 alone) of one case: computed once, shared by the backends, never modified"""
    inp = L.inputs(T, Cc, dy_dtype, seed=1000 * T + Cc, **kw)
    ref = L.reference64(inp)
    B, e32 = L.bounds(inp, ref)
    L.assert_sensitive(inp, ref, B, out16, colsum=colsum, what=f"{T} x {Cc} {IDS[dy_dtype]}")
    return inp, ref, B, e32


def nan_out(shape, dtype, dev):
    if dtype == torch.uint8:
        return torch.full(shape, 0xFF, dtype=dtype, device=dev)
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def call(be, dev, inp, *, public=False, dx=True, out16=BF, colsum=False, fp8=None, scale=None, amax0=0.0, ldo8=None, deferred=True, adjacent=True, rs=True, opf=None):
    """one call -> dict of CPU outputs (dx, dxb, dgamma, dbeta, colsum, out8, amax), or the refusal's code.  out16 None: no 16-bit copy."""
    T, Cc = inp["T"], inp["C"]
    d = lambda t: None if t is None else t.to(dev).contiguous()
    dy, x, mean, rstd, gamma = (d(inp[k]) for k in ("dy", "x", "mean", "rstd", "gamma"))
    dres16 = d(inp["dres"]) if inp["dres"] is not None and inp["dres"].dtype == HF else None
    dres = d(inp["dres"]) if dres16 is None else None
    o_dx = nan_out((T, Cc), F32, dev) if dx else None
    o_dxb = nan_out((T, Cc), out16, dev) if out16 is not None else None
    gb = nan_out((3 * Cc,), F32, dev)
    o_dg, o_db = gb[:Cc], (gb[Cc:2 * Cc] if adjacent else gb[2 * Cc:])
    need = C.c_size_t(0)
    be.check(be.lib.vdk_layernorm_bwd_workspace_bytes(T, Cc, C.byref(need)), "vdk_layernorm_bwd_workspace_bytes")
    assert need.value % 4 == 0
    ws = nan_out((need.value // 4,), F32, dev)
    head = (be.ptr(dy), Cc, DT[inp["dy"].dtype], be.ptr(x), Cc, be.ptr(mean), be.ptr(rstd), be.ptr(gamma), be.ptr(dres), Cc, T, Cc, be.ptr(o_dx), Cc, be.ptr(o_dxb), Cc,
            be.ptr(o_dg), be.ptr(o_db), be.ptr(ws), need.value, be.stream())
    o_cs = o8 = am = sc = dsc = rsv = None
    if public:
        assert not colsum and fp8 is None and dres16 is None and inp["dy_scale"] is None and inp["rs"] is None
        rc = be.lib.vdk_layernorm_bwd(*head)
    else:
        o_cs = nan_out((Cc,), F32, dev) if colsum else None
        if fp8 is not None:
            ldo8 = Cc if ldo8 is None else ldo8
            o8 = nan_out((T, ldo8), torch.uint8, dev)
            am = torch.full((1,), amax0, dtype=F32, device=dev)
            sc = torch.full((1,), scale, dtype=F32, device=dev)
        dsc = torch.full((1,), inp["dy_scale"], dtype=F32, device=dev) if inp["dy_scale"] is not None else None
        rsv = d(inp["rs"]) if rs else None
        if opf is None:
            opf = 1 if out16 == HF else 0
        rc = be.lib.vdk_debug_layernorm_bwd_forms(*head, be.ptr(o_cs), be.ptr(o8), ldo8 or 0, fp8 or 0, be.ptr(sc), be.ptr(am), opf, be.ptr(dsc), be.ptr(rsv),
                                                  inp["rps"] or 1, be.ptr(dres16), int(deferred))
    if rc != 0:
        return rc
    if be.device_only:
        torch.cuda.synchronize()
    out = {"dx": o_dx, "dxb": o_dxb, "dgamma": o_dg, "dbeta": o_db, "colsum": o_cs, "out8": o8, "amax": am}
    return {k: v.detach().cpu().clone() for k, v in out.items() if v is not None}


def same_bits(a, b, what, keys=None):
    for k in (keys or a.keys()):
        assert torch.equal(gemmbound.bits(a[k]), gemmbound.bits(b[k])), (what, k, "differs between two runs")


def twice(be, dev, inp, what, **kw):
    a, b = call(be, dev, inp, **kw), call(be, dev, inp, **kw)
    assert isinstance(a, dict), (what, "refused with code", a)
    same_bits(a, b, what)
    return a


def check_fp8(be, dev, got, fmt, scale, amax0, what):
    """out8 = vdk_quant_fp8 of the kernel's own stored dxb, bit for bit; amax = max(preset, max |dxb|) exactly"""
    st = got["dxb"]
    flat = torch.zeros((st.numel() + 15) // 16 * 16, dtype=st.dtype)
    flat[:st.numel()] = st.reshape(-1)
    ref8 = ops.quant_fp8(flat.to(dev), torch.full((1,), scale, dtype=F32, device=dev), fmt, None, backend=be).cpu()[:st.numel()].reshape(st.shape)
    gemmbound.check_exact(got["out8"][:, :st.shape[1]], ref8, what + " fp8 copy")
    want = max(amax0, float(st.float().abs().max()))
    assert float(got["amax"][0]) == want, (what, "amax", float(got["amax"][0]), want)


# ---------------------------------------------------------------------------------------------------------------- plain forms, public entry
@pytest.mark.parametrize("dy_dtype", [BF, HF, F32], ids=IDS.get)
@pytest.mark.parametrize("T,Cc", [(T0, Cw) for Cw in L.WIDTHS] + list(L.SMALL))
def test_plain_forms_element_by_element(be, dev, T, Cc, dy_dtype):
    out16 = BF if dy_dtype == F32 else dy_dtype
    for dres in (True, False):
        inp, ref, B, e32 = case(T, Cc, dy_dtype, out16, dres=dres)
        what = f"{be.name} plain {T} x {Cc} {IDS[dy_dtype]} dres={int(dres)}"
        got = twice(be, dev, inp, what, public=True, out16=out16)
        L.check_backward(got, inp, ref, B, e32, what)


@pytest.mark.parametrize("T,Cc", L.TALL)          # (one to two seconds on the emulator)
def test_tall_half_wave_second_pass(be, dev, T, Cc):
    for dy_dtype in (BF, F32):
        inp, ref, B, e32 = case(T, Cc, dy_dtype, BF, dres=True)
        what = f"{be.name} tall {T} x {Cc} {IDS[dy_dtype]}"
        got = twice(be, dev, inp, what, public=True, out16=BF)
        L.check_backward(got, inp, ref, B, e32, what)


@pytest.mark.parametrize("Cc", [8, 260, 772, 4096])
def test_null_outputs_public(be, dev, Cc):
    """dx = NULL (the engines' 16-bit residual path: dxb against float64 by the half-ulp rule) and dxb = NULL; what remains has the bits of the full call"""
    inp, ref, B, e32 = case(T0, Cc, BF, BF, dres=True)
    full = twice(be, dev, inp, "full", public=True, out16=BF)
    for kw in ({"dx": False, "out16": BF}, {"dx": True, "out16": None}):
        what = f"{be.name} {T0} x {Cc} {kw}"
        got = twice(be, dev, inp, what, public=True, **kw)
        L.check_backward(got, inp, ref, B, e32, what)
        same_bits(got, full, what + " against the full call", keys=got.keys())


@pytest.mark.parametrize("Cc", [8, 256, 512, 768, 1024, 4096])
def test_f32_dy_with_an_fp16_copy(be, dev, Cc):
    """the ConvNeXt stem's call: fp32 dy, no dx, the copy in fp16 by `opf`"""
    inp, ref, B, e32 = case(T0, Cc, F32, HF, dres=False)
    what = f"{be.name} f32 dy, fp16 copy {T0} x {Cc}"
    got = twice(be, dev, inp, what, dx=False, out16=HF, deferred=False)
    assert got["dxb"].dtype == HF
    L.check_backward(got, inp, ref, B, e32, what)
    full = twice(be, dev, inp, what, dx=True, out16=HF)
    L.check_backward(full, inp, ref, B, e32, what + " with dx")
    same_bits(got, full, what, keys=got.keys())


# ---------------------------------------------------------------------------------------------------------------- engine-only forms
@pytest.mark.parametrize("dy_dtype", [BF, HF, F32], ids=IDS.get)
@pytest.mark.parametrize("T", [1, T0])
@pytest.mark.parametrize("Cc", [8, 128, 256, 260, 516, 768, 772, 1024])          # (256 and 768 beyond the issue's list: MAXJ = 1 without HALF, and the upper edge of MAXJ = 3)
def test_column_sums(be, dev, Cc, T, dy_dtype):
    for out16 in ((BF, HF) if dy_dtype == F32 else (dy_dtype,)):
        inp, ref, B, e32 = case(T, Cc, dy_dtype, out16, True, dres=True)
        what = f"{be.name} colsum {T} x {Cc} {IDS[dy_dtype]}->{IDS[out16]}"
        got = twice(be, dev, inp, what, out16=out16, colsum=True)
        L.check_backward(got, inp, ref, B, e32, what)
        plain = twice(be, dev, inp, what, out16=out16, colsum=False)
        same_bits(plain, got, what + " against the form without column sums", keys=plain.keys())


@pytest.mark.parametrize("fmt", [ops.FP8_E4M3, ops.FP8_E5M2], ids=["e4m3", "e5m2"])
@pytest.mark.parametrize("Cc", [8, 260, 768, 772, 1024])
def test_fp8_copy(be, dev, Cc, fmt):
    inp, ref, B, e32 = case(T0, Cc, BF, BF, True, dres=True)
    scale = 2.0
    base = twice(be, dev, inp, "no fp8", out16=BF, colsum=True)
    for amax0 in (0.0, 64.0):
        what = f"{be.name} fp8 {T0} x {Cc} fmt {fmt} preset {amax0}"
        got = twice(be, dev, inp, what, out16=BF, colsum=True, fp8=fmt, scale=scale, amax0=amax0, ldo8=Cc + 4)
        assert float(got["dxb"].float().abs().max()) < 64.0
        L.check_backward(got, inp, ref, B, e32, what)
        check_fp8(be, dev, got, fmt, scale, amax0, what)
        assert bool((got["out8"][:, Cc:] == 0xFF).all()), "the padding of the fp8 rows was written"
        if Cc > 512:          # (narrower rows: the form without the copy holds two rows per wave, another order of the column partials)
            same_bits(base, got, what + " against the form without the copy", keys=base.keys())


@pytest.mark.parametrize("Cc", [516, 768, 772, 1024])
def test_dres16(be, dev, Cc):
    inp, ref, B, e32 = case(T0, Cc, HF, HF, True, dres16=True)
    what = f"{be.name} dres16 {T0} x {Cc}"
    got = twice(be, dev, inp, what, out16=HF, colsum=True)
    L.check_backward(got, inp, ref, B, e32, what)
    nodx = twice(be, dev, inp, what, dx=False, out16=HF, colsum=True)          # as the ViT engine calls it: the 16-bit copy IS the stream
    L.check_backward(nodx, inp, ref, B, e32, what + " dx = NULL")
    same_bits(nodx, got, what, keys=nodx.keys())


@pytest.mark.parametrize("Cc", [96, 192, 384, 768])
def test_dy_scale(be, dev, Cc):
    """ConvNeXt's layer-scale branch under fp16: dx only, deferred or not (csrc/convnext_engine.hip)"""
    inp, ref, B, e32 = case(T0, Cc, HF, None, dres=False, dy_scale=True)
    res = []
    for deferred in (True, False):
        what = f"{be.name} dy_scale {T0} x {Cc} deferred={int(deferred)}"
        res.append(twice(be, dev, inp, what, out16=None, deferred=deferred))
        L.check_backward(res[-1], inp, ref, B, e32, what)
    same_bits(res[0], res[1], "deferred against not deferred")


@pytest.mark.parametrize("dtype", [BF, HF], ids=IDS.get)
@pytest.mark.parametrize("Cc", [128, 260, 772])
def test_dxb_row_scale(be, dev, Cc, dtype):
    """3 samples x 7 rows: the block edge (11 + 10 rows) falls inside the second sample.  The factor goes into the 16-bit copy only, the column sums are sums of the scaled values"""
    T = 21
    inp, ref, B, e32 = case(T, Cc, dtype, dtype, True, dres=True, rps=7)
    unscaled = twice(be, dev, inp, "no dxb_rs", out16=dtype, colsum=True, rs=False)
    for colsum in (True, False):
        what = f"{be.name} dxb_rs {T} x {Cc} {IDS[dtype]} colsum={int(colsum)}"
        got = twice(be, dev, inp, what, out16=dtype, colsum=colsum)
        L.check_backward(got, inp, ref, B, e32, what)
        same_bits(got, unscaled, what + ": dx, dgamma, dbeta against the run without dxb_rs", keys=("dx", "dgamma", "dbeta"))
        nodx = twice(be, dev, inp, what, dx=False, out16=dtype, colsum=colsum)
        L.check_backward(nodx, inp, ref, B, e32, what + " dx = NULL")
        same_bits(nodx, got, what, keys=nodx.keys())
    assert not torch.equal(gemmbound.bits(got["dxb"]), gemmbound.bits(unscaled["dxb"]))


@pytest.mark.parametrize("dtype", [BF, F32], ids=IDS.get)
@pytest.mark.parametrize("Cc", [8, 260, 772, 4096])
def test_dgamma_dbeta_jobs(be, dev, Cc, dtype):
    """adjacent (the deferred 2C-wide job), not adjacent, not deferred: the same bits"""
    inp, ref, B, e32 = case(T0, Cc, dtype, BF, dres=True)
    runs = [twice(be, dev, inp, f"{be.name} jobs {Cc} {kw}", out16=BF, **kw) for kw in ({"deferred": True, "adjacent": True}, {"deferred": True, "adjacent": False},
                                                                                         {"deferred": False, "adjacent": True}, {"deferred": False, "adjacent": False})]
    L.check_backward(runs[0], inp, ref, B, e32, f"{be.name} deferred job {T0} x {Cc}")
    for r in runs[1:]:
        same_bits(runs[0], r, "dgamma | dbeta job forms")
    same_bits(runs[0], twice(be, dev, inp, "public", public=True, out16=BF), "the debug entry against the public one")


def test_refusals(be, dev):
    bf = lambda Cc, **kw: case(T0, Cc, BF, BF, True, **kw)[0]
    hf = lambda Cc, **kw: case(T0, Cc, HF, HF, True, **kw)[0]
    f32 = case(T0, 772, F32, BF, True, dres=True)[0]
    q = dict(fp8=ops.FP8_E4M3, scale=2.0)
    assert call(be, dev, case(T0, 1028, BF, BF, dres=True)[0], out16=BF, colsum=True) == EINVAL                     # column sums beyond C = 1024
    assert call(be, dev, f32, out16=BF, colsum=True, **q) == EINVAL                                                  # the fp8 copy: f32 dy
    assert call(be, dev, hf(772, dres=True), out16=HF, colsum=True, **q) == EINVAL                                   # ... fp16
    assert call(be, dev, bf(772, dres=True), out16=BF, colsum=False, **q) == EINVAL                                  # ... without column sums
    assert call(be, dev, bf(772, dres=True), out16=BF, colsum=True, ldo8=774, **q) == EINVAL                         # ... ldo8 % 4 != 0
    assert call(be, dev, case(T0, 512, HF, HF, True, dres16=True)[0], out16=HF, colsum=True) == EINVAL              # dres16 at C = 512
    assert call(be, dev, hf(772, dres16=True), out16=HF, colsum=False) == EINVAL                                     # ... without column sums
    bad = dict(bf(772, dres=True)); bad["dres"] = bad["dres"].half()
    assert call(be, dev, bad, out16=BF, colsum=True) == EINVAL                                                       # ... with bf16 dy
    assert isinstance(call(be, dev, bf(772, dres=True), out16=BF, colsum=True, ldo8=776, **q), dict)                 # and the neighbours of the refusals are served
    assert isinstance(call(be, dev, hf(772, dres16=True), out16=HF, colsum=True), dict)


# ---------------------------------------------------------------------------------------------------------------- the column-sum pass with its fp8 copy
def colsum16(be, dev, x, fmt=None, scale=2.0, amax0=0.0, opf=None):
    T, N = x.shape
    xd = x.to(dev).contiguous()
    need = C.c_size_t(0)
    be.check(be.lib.vdk_colsum_bf16_workspace_bytes(T, N, C.byref(need)), "vdk_colsum_bf16_workspace_bytes")
    ws = nan_out((need.value // 4,), F32, dev)
    out = nan_out((N,), F32, dev)
    o8 = nan_out((T, N + 8), torch.uint8, dev) if fmt is not None else None
    am = torch.full((1,), amax0, dtype=F32, device=dev) if fmt is not None else None
    sc = torch.full((1,), scale, dtype=F32, device=dev) if fmt is not None else None
    rc = be.lib.vdk_debug_colsum16_q8(be.ptr(xd), N, T, N, be.ptr(out), be.ptr(ws), need.value, be.ptr(o8), N + 8, fmt or 0, be.ptr(sc), be.ptr(am),
                                      (1 if x.dtype == HF else 0) if opf is None else opf, be.stream())
    if rc != 0:
        return rc
    if be.device_only:
        torch.cuda.synchronize()
    return {k: v.cpu() for k, v in (("colsum", out), ("out8", o8), ("amax", am)) if v is not None}


@pytest.mark.parametrize("T,N", [(1, 8), (33, 264), (300, 72), (2100, 2304)])          # one split; a ragged tail behind the 32-row loop; a ragged last column block; many splits
@pytest.mark.parametrize("form", ["bf16", "fp16", "bf16-e4m3", "bf16-e5m2"])
def test_colsum16_q8(be, dev, T, N, form):
    dtype = HF if form == "fp16" else BF
    fmt = {"bf16-e4m3": ops.FP8_E4M3, "bf16-e5m2": ops.FP8_E5M2}.get(form)
    x = torch.randn(T, N, generator=torch.Generator().manual_seed(T + N), dtype=torch.float64).float().to(dtype)
    what = f"{be.name} colsum16 {T} x {N} {form}"
    for amax0 in ((0.0, 64.0) if fmt is not None else (0.0,)):
        a, b = colsum16(be, dev, x, fmt, amax0=amax0), colsum16(be, dev, x, fmt, amax0=amax0)
        same_bits(a, b, what)
        L.check_colsum(a["colsum"], x, what)
        if dtype == BF:
            assert torch.equal(gemmbound.bits(a["colsum"]), gemmbound.bits(ops.colsum_bf16(x.to(dev), backend=be).cpu())), (what, "differs from vdk_colsum_bf16")
        if fmt is not None:
            check_fp8(be, dev, {"dxb": x, **a}, fmt, 2.0, amax0, what)
            assert bool((a["out8"][:, N:] == 0xFF).all())
    if dtype == HF:
        assert colsum16(be, dev, x, ops.FP8_E4M3) == EINVAL          # the fp8 copy goes with bf16 tensors


# ---------------------------------------------------------------------------------------------------------------- forward, same grid
@pytest.mark.parametrize("T,Cc", [(T0, Cw) for Cw in L.WIDTHS] + list(L.SMALL))
def test_forward_element_by_element(be, dev, T, Cc):
    eps = 1e-6
    inp = L.inputs(T, Cc, BF, seed=7 * T + Cc, far_rows=True)          # every third row: mean = 100 standard deviations
    ref = L.forward64(inp, eps)
    B, e32 = L.forward_bounds(inp, ref, eps)
    x, g, b = (inp[k].to(dev) for k in ("x", "gamma", "beta"))
    runs = [ops.layernorm_fwd(x, g, b, eps=eps, out_dtype=F32, backend=be) for _ in range(2)]
    got = dict(zip(("y", "mean", "rstd"), (t.cpu() for t in runs[0])))
    same_bits(got, dict(zip(("y", "mean", "rstd"), (t.cpu() for t in runs[1]))), "forward")
    L.check_forward(got, ref, B, e32, f"{be.name} forward {T} x {Cc}")
    for dtype in (BF, HF):
        y16, m16, r16 = ops.layernorm_fwd(x, g, b, eps=eps, out_dtype=dtype, backend=be)
        gemmbound.check_exact(y16.cpu(), L.rne16(got["y"], dtype), f"forward {IDS[dtype]} y = RNE16(f32 y)")
        same_bits({"mean": m16.cpu(), "rstd": r16.cpu()}, got, "forward statistics", keys=("mean", "rstd"))
