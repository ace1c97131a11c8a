"""The engine-only forms of the LayerNorm backward and the column-sum pass with its fp8 copy (csrc/norm_loss.hip, through the test-only entries of csrc/vdk_internal.h) read and
write nothing outside their operands' extents (tests/extent.py, as tests/test_layerscale_residual_extent.py): guard-banded operands with every pitch padded, filled with
0x00 / 0xFF / 0x7B -- I1 guards intact, I2 outputs bit-identical across the fills, I3 the same bits as the contiguous call -- and a workspace of exactly the reported size (a
guarded flat buffer: one byte past it is guard).  The column-sum, fp8 and dres16 forms at 19 x 772 (a ragged second block, a partly filled fourth slab), dxb_rs at 21 x 128
(the half-wave form, the block edge inside a sample), the column-sum entry at 33 x 264 (a ragged tail behind the 32-row loop, a ragged last column block)."""
import ctypes as C

import pytest
import torch

from tests import lnbound as L
from tests.extent import run_isolated
from tests.test_layernorm_forms import BF, DT, F32, HF, case
from visiondk_amd import ops

PADS = {"x": 8, "dy": 24, "dres": 12, "dx": 20, "dxb": 40, "out8": 12}          # elements between the rows (fp32: x 4, 16-bit: x 4 keep the 8- and 16-byte row alignment)
p = lambda t: None if t is None else t.data_ptr()          # (padded views are not contiguous: be.ptr refuses them)


@pytest.mark.parametrize("form", ["colsum-bf16", "colsum-f32", "fp8-e4m3", "fp8-e5m2", "dres16", "dxb_rs"])
def test_layernorm_bwd_forms_extents(be, dev, form):
    T, Cc = (21, 128) if form == "dxb_rs" else (19, 772)
    dtype = {"colsum-f32": F32, "dres16": HF, "dxb_rs": HF}.get(form, BF)
    out16 = BF if dtype == F32 else dtype
    inp, ref, B, e32 = case(T, Cc, dtype, out16, True, **({"dres16": True} if form == "dres16" else {"dres": True, "rps": 7} if form == "dxb_rs" else {"dres": True}))
    fmt = {"fp8-e4m3": ops.FP8_E4M3, "fp8-e5m2": ops.FP8_E5M2}.get(form)
    need = C.c_size_t(0)
    be.check(be.lib.vdk_layernorm_bwd_workspace_bytes(T, Cc, C.byref(need)), "vdk_layernorm_bwd_workspace_bytes")

    def run(ar):
        x, dy, dres = ar.put(inp["x"], PADS["x"], "x"), ar.put(inp["dy"], PADS["dy"], "dy"), ar.put(inp["dres"], PADS["dres"], "dres")
        mean, rstd, gamma = ar.put(inp["mean"], 0, "mean"), ar.put(inp["rstd"], 0, "rstd"), ar.put(inp["gamma"], 0, "gamma")
        rs = ar.put(inp["rs"], 0, "dxb_rs") if inp["rs"] is not None else None
        dx, dxb = ar.out((T, Cc), F32, PADS["dx"], "dx"), ar.out((T, Cc), out16, PADS["dxb"], "dxb")
        gb, cs = ar.out(2 * Cc, F32, 0, "dgamma | dbeta"), ar.out(Cc, F32, 0, "column sums")
        ws = ar.out(need.value, torch.uint8, 0, "workspace")
        o8 = sc = am = None
        if fmt is not None:
            o8 = ar.out((T, Cc), torch.uint8, PADS["out8"], "fp8 copy")
            sc, am = ar.put(torch.full((1,), 2.0), 0, "scale"), ar.put(torch.zeros(1), 0, "amax")
        h16 = form == "dres16"
        be.check(be.lib.vdk_debug_layernorm_bwd_forms(p(dy), dy.stride(0), DT[dtype], p(x), x.stride(0), p(mean), p(rstd), p(gamma), None if h16 else p(dres), dres.stride(0), T, Cc,
                                                      p(dx), dx.stride(0), p(dxb), dxb.stride(0), p(gb), p(gb) + 4 * Cc, p(ws), need.value, be.stream(), p(cs), p(o8),
                                                      o8.stride(0) if o8 is not None else 0, fmt or 0, p(sc), p(am), 1 if out16 == HF else 0, None, p(rs), inp["rps"] or 1,
                                                      p(dres) if h16 else None, 1), "vdk_debug_layernorm_bwd_forms")
        return {"dx": dx, "dxb": dxb, "dgamma": gb[:Cc], "dbeta": gb[Cc:], "colsum": cs, "out8": o8, "amax": am}

    got, _ = run_isolated(run, dev, sync=torch.cuda.synchronize if be.device_only else None, what=f"layernorm bwd {form} extents {T} x {Cc}")
    L.check_backward({k: v.cpu() for k, v in got.items()}, inp, ref, B, e32, f"{be.name} extents {form}")


@pytest.mark.parametrize("form", ["bf16", "fp16", "bf16-e5m2"])
def test_colsum16_q8_extents(be, dev, form):
    T, N = 33, 264
    dtype = HF if form == "fp16" else BF
    fmt = ops.FP8_E5M2 if form == "bf16-e5m2" else None
    x0 = torch.randn(T, N, generator=torch.Generator().manual_seed(T + N)).to(dtype)
    need = C.c_size_t(0)
    be.check(be.lib.vdk_colsum_bf16_workspace_bytes(T, N, C.byref(need)), "vdk_colsum_bf16_workspace_bytes")

    def run(ar):
        x, out, ws = ar.put(x0, 16, "in"), ar.out(N, F32, 0, "column sums"), ar.out(need.value, torch.uint8, 0, "workspace")
        o8 = sc = am = None
        if fmt is not None:
            o8, sc, am = ar.out((T, N), torch.uint8, 24, "fp8 copy"), ar.put(torch.full((1,), 2.0), 0, "scale"), ar.put(torch.zeros(1), 0, "amax")
        be.check(be.lib.vdk_debug_colsum16_q8(p(x), x.stride(0), T, N, p(out), p(ws), need.value, p(o8), o8.stride(0) if o8 is not None else 0, fmt or 0, p(sc), p(am),
                                              1 if dtype == HF else 0, be.stream()), "vdk_debug_colsum16_q8")
        return {"colsum": out, "out8": o8, "amax": am}

    got, _ = run_isolated(run, dev, sync=torch.cuda.synchronize if be.device_only else None, what=f"colsum16 {form} extents {T} x {N}")
    L.check_colsum(got["colsum"].cpu(), x0, f"{be.name} extents colsum16 {form}")
