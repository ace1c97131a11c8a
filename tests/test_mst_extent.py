"""The raw row-scan entry of the spanning-tree kernels (csrc/cbir_mst.hip: vdk_mst_scan) reads and writes nothing outside its operands' extents (tests/extent.py, as
tests/test_cbir_range_extent.py): the raw ABI on guard-banded operands filled with 0x00 / 0xFF / 0x7B -- I1 guards intact, I2 outputs bit-identical across the fills, I3 the
same bits as the plain call -- with a workspace of exactly the reported size (one byte less is VDK_EWORKSPACE).  The scanned block is a strict part of the rows, so best_w /
best_j hold the fill outside it; what the scan leaves is held against a numpy statement of it on the oracle's scores.  The refusals of the entry are checked on the way."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import cbir as ocbir
from tests.extent import run_isolated

F32 = np.float32
EINVAL, EWORKSPACE = -1, -2


def _case(n, d, ncomp, seed=0):
    rng = np.random.default_rng(seed)
    x = ocbir.l2norm_rows(rng.standard_normal((n, d), dtype=F32))
    core = (0.3 * rng.random(n)).astype(F32)                     # any non-negative values: the entry takes them as given
    comp = rng.integers(0, ncomp, n).astype(np.int32)
    so, io = ocbir.flat_ip_search(x, x, n)
    S = np.empty((n, n), F32)
    np.put_along_axis(S, io, so, axis=1)
    return x, core, comp, S


def _expect(S, core, comp, q0, nq):
    w = np.maximum(np.maximum(core[:, None], core[None, :]), np.maximum(F32(0), F32(1) - S)).astype(F32)
    w[comp[:, None] == comp[None, :]] = np.inf
    j = np.argmin(w, axis=1)                                     # the first minimum: the smallest j among equal w
    return w[np.arange(len(j)), j][q0:q0 + nq], j[q0:q0 + nq].astype(np.int32)


@pytest.mark.parametrize("n,d,q0,nq,ncomp", [(333, 64, 32, 270, 7), (100, 192, 0, 100, 2), (2100, 128, 1500, 600, 40), (70, 512, 3, 9, 70)])
def test_scan_extents(be, dev, n, d, q0, nq, ncomp):
    x, core, comp, S = _case(n, d, ncomp)
    dp = (d + 127) // 128 * 128
    p = lambda t: None if t is None else t.data_ptr()
    need = C.c_size_t(0)
    be.check(be.lib.vdk_mst_scan_workspace_bytes(nq, n, d, C.byref(need)), "mst workspace")
    sync = torch.cuda.synchronize if be.device_only else (lambda: None)
    st = be.stream()

    def run(ar):
        X = ar.put(torch.from_numpy(x), 0, "X")
        Gb, gn, gm = ar.out((n, dp), torch.bfloat16, 0, "Gb"), ar.out(3 * n, torch.float32, 0, "row norms"), ar.out(4, torch.int32, 0, "gmax")
        be.check(be.lib.vdk_cbir_prepare_gallery(p(X), n, d, p(Gb), p(gn), p(gm), st), "prepare gallery")
        co, cm = ar.put(torch.from_numpy(core), 0, "core"), ar.put(torch.from_numpy(comp), 0, "comp")
        bw, bj = ar.out(n, torch.float32, 0, "best_w"), ar.out(n, torch.int32, 0, "best_j")
        ws = ar.out(need.value, torch.uint8, 0, "workspace")
        args = (p(X), p(Gb), p(gn), p(gm), p(co), p(cm), n, d, q0, nq, p(bw), p(bj))
        assert be.lib.vdk_mst_scan(*args, p(ws), need.value - 1, st) == EWORKSPACE
        be.check(be.lib.vdk_mst_scan(*args, p(ws), need.value, st), "mst scan")
        sync()
        if not ar.plain:                                # nothing outside the block
            for t in (bw, bj):
                b = t.view(torch.uint8).reshape(n, 4)
                assert bool((b[:q0] == ar.fill).all()) and bool((b[q0 + nq:] == ar.fill).all())
        return {"best_w": bw[q0:q0 + nq], "best_j": bj[q0:q0 + nq]}

    got, _ = run_isolated(run, dev, sync=torch.cuda.synchronize if be.device_only else None, what=f"mst scan extents {n}x{d} rows {q0}+{nq}")
    want_w, want_j = _expect(S, core, comp, q0, nq)
    np.testing.assert_array_equal(got["best_j"].cpu().numpy(), want_j)
    np.testing.assert_array_equal(got["best_w"].cpu().numpy().view(np.uint32), want_w.view(np.uint32))


def test_refusals(be, dev):
    n, d = 100, 64
    x, core, comp, _ = _case(n, d, 5)
    p, lib, st = be.ptr, be.lib, be.stream()
    X, co, cm = torch.from_numpy(x).to(dev), torch.from_numpy(core).to(dev), torch.from_numpy(comp).to(dev)
    Gb, gn, gm = torch.empty((n, 128), dtype=torch.bfloat16, device=dev), torch.empty(3 * n, dtype=torch.float32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
    be.check(lib.vdk_cbir_prepare_gallery(p(X), n, d, p(Gb), p(gn), p(gm), st), "prepare gallery")
    need = C.c_size_t(0)
    be.check(lib.vdk_mst_scan_workspace_bytes(n, n, d, C.byref(need)), "workspace")
    ws = torch.empty(need.value + 16, dtype=torch.uint8, device=dev)
    bw, bj = torch.empty(n + 4, dtype=torch.float32, device=dev), torch.empty(n + 4, dtype=torch.int32, device=dev)

    def scan(N=n, D=d, q0=0, nq=n, X_=X.data_ptr(), Gb_=Gb.data_ptr(), co_=co.data_ptr(), cm_=cm.data_ptr(), bw_=bw.data_ptr(), bj_=bj.data_ptr(), ws_=ws.data_ptr(),
             nbytes=need.value):
        return lib.vdk_mst_scan(X_, Gb_, p(gn), p(gm), co_, cm_, N, D, q0, nq, bw_, bj_, ws_, nbytes, st)
    bad = (dict(D=62), dict(D=516), dict(N=1 << 31), dict(N=1, nq=1), dict(q0=1), dict(q0=-1), dict(nq=0), dict(nq=n + 1), dict(X_=None), dict(co_=None), dict(bj_=None),
           dict(X_=X.data_ptr() + 4), dict(Gb_=Gb.data_ptr() + 8), dict(ws_=ws.data_ptr() + 4), dict(co_=co.data_ptr() + 2), dict(cm_=cm.data_ptr() + 1),
           dict(bw_=bw.data_ptr() + 2), dict(bj_=bj.data_ptr() + 3))
    for kw in bad:
        assert scan(**kw) == EINVAL and b"vdk_mst" in lib.vdk_last_error(), kw
    assert scan(nbytes=need.value - 1) == EWORKSPACE and scan(ws_=None) == EWORKSPACE
    for args in ((n, n, 62), (n, n, 516), (n, 1 << 31, d), (0, n, d), (n + 1, n, d), (1, 1, d)):
        assert lib.vdk_mst_scan_workspace_bytes(*args, C.byref(need)) == EINVAL, args
    assert lib.vdk_mst_scan_workspace_bytes(n, n, d, None) == EINVAL
    assert scan(bw_=bw.data_ptr() + 4, bj_=bj.data_ptr() + 4, ws_=ws.data_ptr() + 16) == 0              # 4-byte outputs and a 16-byte workspace are aligned enough
    if be.device_only:
        torch.cuda.synchronize()
