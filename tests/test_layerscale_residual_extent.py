"""The LayerScale residual kernels (csrc/layerscale_residual.hip) read and write nothing outside their operands' extents (tests/extent.py, as
tests/test_window_attention_cos_extent.py): both entries on guard-banded, column-padded operands filled with 0x00 / 0xFF / 0x7B -- I1 guards intact, I2 outputs bit-identical
across the fills, I3 the same bits as the contiguous call -- with a workspace of exactly the reported size (a guarded flat buffer: one byte past it is guard).
37 x 8 (one column group, a ragged row split), 52 x 384 (two column blocks, the second ragged), 302 x 1024 (three row splits, the last one ragged)."""
import ctypes as C

import pytest
import torch

from tests.extent import run_isolated
from tests.test_layerscale_residual import OPF, make_gamma

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
PADS = (8, 24, 64, 16, 40)          # elements between the rows of x, h, y, dy, dh


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("rows,Cc", [(37, 8), (52, 384), (302, 1024)])
def test_ls_residual_extents(be, dev, rows, Cc, dtype):
    g = torch.Generator().manual_seed(rows + Cc)
    x0, dy0 = torch.randn(rows, Cc, generator=g), torch.randn(rows, Cc, generator=g)
    h0 = torch.randn(rows, Cc, generator=g).to(dtype)
    gamma0 = make_gamma(Cc, g)
    p = lambda t: None if t is None else t.data_ptr()          # (padded views are not contiguous: be.ptr refuses them)
    need = C.c_size_t(0)
    be.check(be.lib.vdk_ls_residual_bwd_workspace_bytes(rows, Cc, C.byref(need)), "ls_residual bwd workspace")

    def run(ar):
        px, ph, py, pd, pdh = PADS
        x, h, dy, gm = ar.put(x0, px, "x"), ar.put(h0, ph, "h"), ar.put(dy0, pd, "dy"), ar.put(gamma0, 0, "gamma")
        y, dh, dg = ar.out((rows, Cc), F32, py, "y"), ar.out((rows, Cc), dtype, pdh, "dh"), ar.out(Cc, F32, 0, "dgamma")
        ws = ar.out(need.value, torch.uint8, 0, "bwd workspace")
        be.check(be.lib.vdk_ls_residual_fwd(p(x), x.stride(0), p(h), h.stride(0), p(gm), p(y), y.stride(0), rows, Cc, OPF[dtype], be.stream()), "ls_residual fwd")
        be.check(be.lib.vdk_ls_residual_bwd(p(dy), dy.stride(0), p(h), h.stride(0), p(gm), p(dh), dh.stride(0), p(dg), rows, Cc, OPF[dtype], p(ws), need.value, be.stream()),
                 "ls_residual bwd")
        return {"y": y, "dh": dh, "dgamma": dg}

    got, _ = run_isolated(run, dev, sync=torch.cuda.synchronize if be.device_only else None, what=f"ls_residual extents {dtype} {rows} x {Cc}")
    for name, t in got.items():
        assert bool(torch.isfinite(t.float()).all()), name
    assert torch.equal(got["y"].cpu(), x0 + gamma0 * h0.float())
