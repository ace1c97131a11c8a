"""The range-search and DBSCAN entries (csrc/cbir_range.hip) read and write nothing outside their operands' extents (tests/extent.py, as
tests/test_window_attention_cos_extent.py): the raw ABI on guard-banded operands filled with 0x00 / 0xFF / 0x7B -- I1 guards intact, I2 outputs bit-identical across the fills,
I3 the same bits as the plain call -- with a workspace of exactly the reported size (one byte less is VDK_EWORKSPACE) and D / I buffers longer than the result: nothing is
written past lims[nq] entries."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.extent import run_isolated
from tests.test_cbir_range import _case, _expect, _radii

EWORKSPACE = -2
SLACK = 300            # entries of D / I behind the result


@pytest.mark.parametrize("nq,n,d,storage", [(33, 333, 64, "float32"), (9, 100, 192, "float16"), (70, 2100, 128, "float32")])
def test_range_and_dbscan_extents(be, dev, nq, n, d, storage):
    q, g, S = _case(nq, n, d, storage)
    r = float(_radii(S)["5pct"])
    half = storage == "float16"
    g32 = torch.from_numpy(g).half().float() if half else torch.from_numpy(g)
    q32 = torch.from_numpy(q).half().float() if half else torch.from_numpy(q)
    dp = (d + 127) // 128 * 128
    p = lambda t: None if t is None else t.data_ptr()
    need = C.c_size_t(0)
    be.check(be.lib.vdk_cbir_range_workspace_bytes(nq, n, d, C.byref(need)), "range workspace")
    sync = torch.cuda.synchronize if be.device_only else (lambda: None)
    st = be.stream()

    def run(ar):
        Q, G32 = ar.put(q32, 0, "Q"), ar.put(g32, 0, "G f32")
        G = ar.put(g32.half(), 0, "G f16") if half else G32
        Gb, gn, gm = ar.out((n, dp), torch.bfloat16, 0, "Gb"), ar.out(3 * n, torch.float32, 0, "gallery norms"), ar.out(4, torch.int32, 0, "gmax")
        be.check(be.lib.vdk_cbir_prepare_gallery(p(G32), n, d, p(Gb), p(gn), p(gm), st), "prepare gallery")
        lims, ws = ar.out(nq + 1, torch.int64, 0, "lims"), ar.out(need.value, torch.uint8, 0, "workspace")
        gdt = 2 if half else 1
        args = (p(Q), nq, p(G), gdt, p(Gb), p(gm), n, d, r, 0, p(lims))
        assert be.lib.vdk_cbir_range_count(*args, p(ws), need.value - 1, st) == EWORKSPACE
        be.check(be.lib.vdk_cbir_range_count(*args, p(ws), need.value, st), "range count")
        sync()
        total = int(lims[nq].item())
        Ds, Is = ar.out(total + SLACK, torch.float32, 0, "D"), ar.out(total + SLACK, torch.int64, 0, "I")
        fargs = (p(Q), nq, p(G), gdt, n, d, 5000, p(lims), total, p(Ds), p(Is))
        assert be.lib.vdk_cbir_range_fill(*fargs, p(ws), need.value - 1, st) == EWORKSPACE
        be.check(be.lib.vdk_cbir_range_fill(*fargs, p(ws), need.value, st), "range fill")
        sync()
        if not ar.plain:                                # nothing past lims[nq] entries
            assert bool((Ds[total:].view(torch.uint8) == ar.fill).all()) and bool((Is[total:].view(torch.uint8) == ar.fill).all())
        # DBSCAN kernels on a CSR of the same kind: the first min(nq, n) queries against themselves would need a square problem, so the CSR is this one with its
        # neighbour ids folded into [0, nq)
        nbr = ar.put(torch.remainder(Is[:total] - 5000, nq).cpu(), 0, "nbr")
        core, l0, l1 = ar.out(nq, torch.uint8, 0, "core"), ar.out(nq, torch.int32, 0, "label a"), ar.out(nq, torch.int32, 0, "label b")
        flag, out = ar.put(torch.zeros(1, dtype=torch.int32), 0, "flag"), ar.out(nq, torch.int64, 0, "labels")
        be.check(be.lib.vdk_dbscan_core(p(lims), nq, 3, p(core), p(l0), st), "dbscan core")
        be.check(be.lib.vdk_dbscan_round(p(lims), p(nbr), nq, p(core), p(l0), p(l1), p(flag), st), "dbscan round")
        sync()
        root = (core != 0) & (l1 == torch.arange(nq, dtype=torch.int32, device=l1.device))
        rank = ar.put((torch.cumsum(root.int(), 0) - root.int()).int().cpu(), 0, "rank")
        be.check(be.lib.vdk_dbscan_assign(p(lims), p(nbr), nq, p(core), p(l1), p(rank), p(out), st), "dbscan assign")
        return {"lims": lims, "D": Ds[:total], "I": Is[:total], "core": core, "l0": l0, "l1": l1, "labels": out}

    got, _ = run_isolated(run, dev, sync=torch.cuda.synchronize if be.device_only else None, what=f"range extents {nq}x{n}x{d} {storage}")
    want = _expect(S, np.float32(r), idx_base=5000)
    np.testing.assert_array_equal(got["lims"].cpu().numpy(), want[0])
    np.testing.assert_array_equal(got["I"].cpu().numpy(), want[2])
    np.testing.assert_array_equal(got["D"].cpu().numpy().view(np.uint32), want[1].view(np.uint32))
