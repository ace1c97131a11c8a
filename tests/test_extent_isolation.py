"""No kernel reads or writes outside its operands' extents.

Every entry of include/visiondk.h that takes a pointer to tensor data runs through the raw ABI on guard-banded operands (tests/extent.py): pitches larger than the rows, the
allocation around every operand filled with 0x00 / 0xFF (NaN) / 0x7B (large finite), once per pattern, plus once on plain contiguous tensors.
  I1  no stray write:  the guards of EVERY buffer (inputs included) are intact;
  I2  no stray read:   every output and by-product is bit-identical across the three patterns (the output windows start out as pattern, so an element that the kernel
                       leaves unwritten fails here as well);
  I3  not vacuous:     the 0x00 run is bit-identical to the contiguous call (where a pitch changes the GEMM routing: it meets the existing test's tolerance instead).
Padding whose content the header DEFINES (zeroed columns of dlogits / dcos / patchify / transposes / softmax rows) is part of the logical window here and asserted to be zero.
COVERED / EXCLUDED at the end tie the list of entries to the header.
"""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

from tests.extent import run_isolated
from visiondk_amd import _abi

BF, HF, F32, I64, I32, U8 = torch.bfloat16, torch.float16, torch.float32, torch.int64, torch.int32, torch.uint8
DT = {BF: 0, F32: 1, HF: 2}


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def p(t):
    return None if t is None else t.data_ptr()


def _sync(be):
    return torch.cuda.synchronize if be.device_only else None


def _run(be, dev, case, **kw):
    return run_isolated(case, dev, sync=_sync(be), **kw)


def _need(be, fn, *args):
    n = C.c_size_t(0)
    be.check(fn(*args, C.byref(n)), fn.__name__)
    return max(int(n.value), 16)


def ck(be, rc, what):
    be.check(rc, what)


# ------------------------------------------------------------------------------------------------------------------ 16-bit GEMM
def _desc(a, b, c, M, N, K, **kw):
    d = _abi.GemmDesc()
    d.A, d.lda, d.B, d.ldb, d.C, d.ldc = a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(), c.stride(0)
    d.M, d.N, d.K = M, N, K
    d.c_dtype, d.ab_dtype, d.alpha, d.splitk = DT[c.dtype], DT[a.dtype] if a.dtype in DT else 0, 1.0, 1
    for k, v in kw.items():
        if isinstance(v, torch.Tensor):
            setattr(d, k, v.data_ptr())
            if k == "residual":
                d.ldr = v.stride(0)
            if k == "aux":
                d.ldaux = v.stride(0)
        else:
            setattr(d, k, v)
    return d


class _forced:
    def __init__(self, be, kern):
        self.be, self.kern = be, kern

    def __enter__(self):
        self.be.lib.vdk_gemm_force_kernel(self.kern)

    def __exit__(self, *a):
        self.be.lib.vdk_gemm_force_kernel(0)


def _g(be, served, d, what, ws=None, nbytes=0):
    """one vdk_gemm_bf16_nt launch; `served` collects which kernel the library says it ran (vdk_gemm_last_kernel)"""
    ck(be, be.lib.vdk_gemm_bf16_nt(C.byref(d), p(ws), nbytes, be.stream()), what)
    served.append(be.lib.vdk_gemm_last_kernel())


def _all_served_by(served, kern):
    """a forced kernel is only forced where it can serve: every launch of every run must report the kernel the case is named after"""
    assert served and set(served) == {kern}, (kern, served)


# K % 128 == 0 wherever the persistent four-wave kernel (5) is meant: it multiplies k-tiles in pairs and hands K % 128 != 0 to the eight-wave kernel; kernels 1, 2 and 6 also get
# an odd number of 64-wide k-tiles (K = 192).  fp16 operands: the four-wave and the 128x128 kernels only.
_NT = [(300, 264, 256, k, BF) for k in (1, 2, 5, 6)] + [(300, 264, 192, k, BF) for k in (2, 6)] + [(130, 520, 128, k, BF) for k in (2, 5, 6)] + [(34, 192, 128, k, BF) for k in (1, 5)] + \
      [(300, 264, 256, k, HF) for k in (1, 5, 6)] + [(34, 192, 192, 6, HF)]


@pytest.mark.parametrize("M,N,K,kern,dtype", _NT, ids=[f"{m}x{n}x{k}-k{kn}-{'bf16' if dt == BF else 'fp16'}" for m, n, k, kn, dt in _NT])
def test_gemm_nt_epilogues(be, dev, M, N, K, kern, dtype):
    """vdk_gemm_bf16_nt, NT: fp32 C with bias + padded residual (ldr), 16-bit C with GELU writing a padded aux (ldaux), DGELU reading it back; lda = K + 8 (row starts shift by
    16 bytes from row to row), ldb = K + 16, ldc = N + 8"""
    torch.manual_seed(5)
    a0 = torch.randn(M, K).to(dtype); b0 = torch.randn(N, K).to(dtype); b0[:, 3] += 2.0
    bias0 = torch.randn(N); res0 = torch.randn(M, N)
    ref = a0.float() @ b0.float().T
    kernels = []

    def case(ar):
        a = ar.put(a0, 8, "A"); b = ar.put(b0, 16, "B"); bias = ar.put(bias0, 0, "bias"); res = ar.put(res0, 4, "residual")
        c = ar.out((M, N), F32, 8, "C f32"); g = ar.out((M, N), dtype, 8, "C 16-bit"); aux = ar.out((M, N), dtype, 16, "aux"); dg = ar.out((M, N), dtype, 8, "C dgelu")
        with _forced(be, kern):
            _g(be, kernels, _desc(a, b, c, M, N, K, bias=bias, residual=res), "gemm f32")
            _g(be, kernels, _desc(a, b, g, M, N, K, bias=bias, act=_abi.ACT_GELU, aux=aux), "gemm gelu")
            _g(be, kernels, _desc(a, b, dg, M, N, K, act=_abi.ACT_DGELU, aux=aux), "gemm dgelu")
        return {"c": c, "gelu": g, "aux": aux, "dgelu": dg}

    got, _ = _run(be, dev, case, same_as_plain=False, what=f"gemm nt kern {kern}")
    _all_served_by(kernels, kern)
    assert _rel(got["c"].cpu(), ref + bias0 + res0) < 1e-5                                                     # tolerances of tests/test_gemm.py
    assert _rel(got["aux"].float().cpu(), (ref + bias0).to(dtype).float()) < 3e-3
    assert _rel(got["gelu"].float().cpu(), torch.nn.functional.gelu(ref + bias0).to(dtype).float()) < 4e-3


@pytest.mark.parametrize("M,N,K,kern", [(300, 264, 256, 0), (300, 264, 256, 2), (300, 264, 256, 5), (300, 264, 256, 6), (300, 264, 192, 2), (257, 264, 200, 1), (257, 264, 200, 0)])
def test_gemm_nt_same_kernel_bits(be, dev, M, N, K, kern):
    """I3 for the GEMM: with the same kernel serving the padded and the contiguous call (vdk_gemm_last_kernel), the results are the same bits.  Forced kernels must be the ones
    that ran (K = 200 has no whole 64-wide k-tiles: the 128x128 kernel); kern = 0 is the automatic routing, the only one that may look at a pitch."""
    torch.manual_seed(6)
    a0 = torch.randn(M, K).bfloat16(); b0 = torch.randn(N, K).bfloat16()
    kernels = []

    def case(ar):
        a = ar.put(a0, 8, "A"); b = ar.put(b0, 16, "B"); c = ar.out((M, N), F32, 8, "C"); cb = ar.out((M, N), BF, 24, "C bf16")
        with _forced(be, kern):
            _g(be, kernels, _desc(a, b, c, M, N, K, alpha=0.5), "gemm")
            _g(be, kernels, _desc(a, b, cb, M, N, K), "gemm")
        return {"c": c, "cb": cb}

    got, pl = _run(be, dev, case, same_as_plain=False)
    ref = a0.float() @ b0.float().T
    assert _rel(got["c"].cpu(), 0.5 * ref) < 1e-5 and _rel(got["cb"].float().cpu(), ref.bfloat16().float()) < 3e-3
    if kern:
        _all_served_by(kernels, kern)
    if kernels[0] == kernels[6] and kernels[1] == kernels[7]:          # (runs: three patterns, then the contiguous call)
        assert torch.equal(got["c"].cpu(), pl["c"].cpu()) and torch.equal(got["cb"].cpu().view(torch.int16), pl["cb"].cpu().view(torch.int16))


@pytest.mark.parametrize("kern", [2, 5, 6])
@pytest.mark.parametrize("K,M,N,splitk,rg", [(256, 264, 136, 1, 0), (256, 72, 520, 2, 0), (128, 128, 192, 1, 16), (768, 264, 136, 3, 0)])
def test_gemm_tn_and_splitk(be, dev, K, M, N, splitk, rg, kern):
    """trans = 1 (A [K, M], B [K, N] as they lie), with and without a_row_group (the token-row remap is served by the eight-wave kernel whichever is forced), split-K 1 / 2 / 3 with
    the slab workspace guarded and sized exactly"""
    torch.manual_seed(7)
    kernels = []
    phys = K + K // rg + 1 if rg else K
    a0 = torch.randn(phys, M).bfloat16(); b0 = torch.randn(K, N).bfloat16()
    a_log = a0[torch.tensor([t + t // rg + 1 for t in range(K)])] if rg else a0
    ref = a_log.float().T @ b0.float()
    need = _need(be, be.lib.vdk_gemm_splitk_workspace_bytes, M, N, splitk) if splitk > 1 else 0

    def case(ar):
        a = ar.put(a0, 8, "A"); b = ar.put(b0, 24, "B")
        c = ar.out((M, N), F32, 0 if splitk > 1 else 8, "C")              # split-K needs ldc == N
        ws = ar.out(need, U8, 0, "split-K slabs") if need else None
        with _forced(be, kern):
            _g(be, kernels, _desc(a, b, c, M, N, K, trans=1, a_row_group=rg, splitk=splitk), "gemm tn", ws, need)
        return {"c": c}

    got, _ = _run(be, dev, case, same_as_plain=False)
    _all_served_by(kernels, 2 if rg else kern)
    assert _rel(got["c"].cpu(), ref) < 1e-5


@pytest.mark.parametrize("kern", [2, 5])
@pytest.mark.parametrize("M,N,K,splitk", [(256, 256, 512, 2), (264, 256, 768, 3)])
def test_gemm_nt_splitk(be, dev, M, N, K, splitk, kern):
    torch.manual_seed(8)
    a0 = torch.randn(M, K).bfloat16(); b0 = torch.randn(N, K).bfloat16()
    need = _need(be, be.lib.vdk_gemm_splitk_workspace_bytes, M, N, splitk)
    kernels = []

    def case(ar):
        a = ar.put(a0, 8, "A"); b = ar.put(b0, 8, "B"); c = ar.out((M, N), F32, 0, "C"); ws = ar.out(need, U8, 0, "split-K slabs")
        with _forced(be, kern):
            _g(be, kernels, _desc(a, b, c, M, N, K, splitk=splitk), "gemm split-K", ws, need)
        return {"c": c}

    got, _ = _run(be, dev, case, same_as_plain=False)
    _all_served_by(kernels, kern)
    assert _rel(got["c"].cpu(), a0.float() @ b0.float().T) < 1e-5


@pytest.mark.parametrize("M,N,K,grid", [(300, 264, 192, 8)])
def test_gemm_stream_k(be, dev, M, N, K, grid):
    """stream-K (forced): the persistent workspace -- tile counters zeroed by the caller, accumulator slabs pattern -- guarded; every launch leaves the counters zero"""
    torch.manual_seed(9)
    a0 = torch.randn(M, K).bfloat16(); b0 = torch.randn(N, K).bfloat16(); bias0 = torch.randn(N); res0 = torch.randn(M, N)
    be.lib.vdk_gemm_streamk_grid(grid)              # the workspace holds one pair of slabs per persistent workgroup: sized for THIS grid, not for every CU of the chip
    try:
        need = _need(be, be.lib.vdk_gemm_streamk_workspace_bytes)
    finally:
        be.lib.vdk_gemm_streamk_grid(0)
    kernels = []

    def case(ar):
        a = ar.put(a0, 8, "A"); b = ar.put(b0, 16, "B"); bias = ar.put(bias0); res = ar.put(res0, 4, "residual"); c = ar.out((M, N), F32, 8, "C")
        ws = ar.out(need, U8, 0, "stream-K workspace")
        ws[:65536] = 0
        be.lib.vdk_gemm_streamk_grid(grid); be.lib.vdk_gemm_force_kernel(3)
        try:
            for _ in range(2):                                      # the second launch finds the counters as the first left them
                _g(be, kernels, _desc(a, b, c, M, N, K, bias=bias, residual=res, splitk=-1), "gemm stream-K", ws, need)
        finally:
            be.lib.vdk_gemm_force_kernel(0); be.lib.vdk_gemm_streamk_grid(0)
        return {"c": c, "counters": ws[:65536].clone()}

    got, _ = _run(be, dev, case, same_as_plain=False)
    _all_served_by(kernels, 3)
    assert int(got["counters"].count_nonzero()) == 0
    assert _rel(got["c"].cpu(), a0.float() @ b0.float().T + bias0 + res0) < 1e-5


@pytest.mark.parametrize("kern", [2, 5])
def test_gemm_row_group_into_token_buffer(be, dev, kern):
    """row_group > 0: output row m lands at row m + m / rg + 1 of a [B, 1 + np, D] token buffer and takes residual row m % rg + 1 (pos_embed); the class-token rows that the
    GEMM skips are guards too: they keep the pattern.  row_group < 0: rows stay, residual row m % |rg|."""
    torch.manual_seed(10)
    Bt, np_, N, K = 5, 16, 264, 256                 # (K % 128 == 0: the four-wave kernel that serves the ViT patch embedding takes it)
    M = Bt * np_
    a0 = torch.randn(M, K).bfloat16(); b0 = torch.randn(N, K).bfloat16(); bias0 = torch.randn(N); pos0 = torch.randn(1 + np_, N)
    ref = a0.float() @ b0.float().T + bias0
    skipped, kernels = [], []

    def case(ar):
        a = ar.put(a0, 8, "A"); b = ar.put(b0, 8, "B"); bias = ar.put(bias0); pos = ar.put(pos0, 4, "pos_embed")
        tok = ar.out((Bt * (1 + np_), N), F32, 8, "token buffer"); tok2 = ar.out((M, N), F32, 8, "token buffer without cls")
        with _forced(be, kern):
            _g(be, kernels, _desc(a, b, tok, M, N, K, bias=bias, residual=pos, row_group=np_), "gemm row_group")
            _g(be, kernels, _desc(a, b, tok2, M, N, K, bias=bias, residual=pos, row_group=-np_), "gemm row_group < 0")
        cls = tok.reshape(Bt, 1 + np_, N)[:, 0]
        if not ar.plain:
            skipped.append(bool((cls.contiguous().view(U8) == ar.fill).all()))
        return {"patch rows": tok.reshape(Bt, 1 + np_, N)[:, 1:], "tok2": tok2}

    got, _ = _run(be, dev, case)
    assert skipped == [True, True, True]
    _all_served_by(kernels, kern)
    assert _rel(got["patch rows"].cpu().reshape(M, N), ref + pos0[1:].repeat(Bt, 1)) < 1e-5
    assert _rel(got["tok2"].cpu(), ref + pos0[:np_].repeat(Bt, 1)) < 1e-5


@pytest.mark.parametrize("kern", [5, 6])
@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_gemm_col_scale_row_scale(be, dev, kern, dtype):
    torch.manual_seed(11)
    M, N, K, rps = 300, 264, 128, 49
    a0 = torch.randn(M, K).to(dtype); b0 = torch.randn(N, K).to(dtype); bias0 = torch.randn(N); res0 = torch.randn(M, N); cs0 = torch.rand(N) + 0.5
    rs0 = torch.rand((M + rps - 1) // rps) + 0.5
    ref = a0.float() @ b0.float().T
    kernels = []

    def case(ar):
        a = ar.put(a0, 8, "A"); b = ar.put(b0, 8, "B"); bias = ar.put(bias0); res = ar.put(res0, 12, "residual"); cs = ar.put(cs0, 0, "col_scale"); rs = ar.put(rs0, 0, "row_scale")
        c = ar.out((M, N), F32, 8, "C col_scale"); c2 = ar.out((M, N), F32, 8, "C row_scale")
        with _forced(be, kern):
            _g(be, kernels, _desc(a, b, c, M, N, K, bias=bias, residual=res, col_scale=cs), "gemm col_scale")
            _g(be, kernels, _desc(a, b, c2, M, N, K, bias=bias, residual=res, row_scale=rs, rows_per_scale=rps), "gemm row_scale")
        return {"c": c, "c2": c2}

    got, _ = _run(be, dev, case)
    _all_served_by(kernels, kern)
    assert _rel(got["c"].cpu() - res0, ref * cs0 + bias0) < 2e-5
    assert _rel(got["c2"].cpu() - res0, (ref + bias0) * rs0.repeat_interleave(rps)[:M, None]) < 2e-5


def test_gemm_colsum_byproducts(be, dev):
    """a_colsum (eight-wave 256x256 NT kernel) and c_colsum (plain bf16 epilogue) partial-sum rows, guarded"""
    torch.manual_seed(12)
    M, N, K = 512, 264, 192
    a0 = torch.randn(M, K).bfloat16(); b0 = torch.randn(N, K).bfloat16()
    with _forced(be, 2):
        ra = be.lib.vdk_gemm_a_colsum_rows(M, N, K); rc = be.lib.vdk_gemm_c_colsum_rows(M, N, K)
    assert ra > 0 and rc > 0
    kernels = []

    def case(ar):
        a = ar.put(a0, 8, "A"); b = ar.put(b0, 8, "B"); c = ar.out((M, N), F32, 8, "C"); cb = ar.out((M, N), BF, 8, "C bf16")
        acs = ar.out((ra, K), F32, 0, "a_colsum"); ccs = ar.out((rc, N), F32, 0, "c_colsum")
        with _forced(be, 2):
            ck(be, be.lib.vdk_gemm_bf16_nt(C.byref(_desc(a, b, c, M, N, K, a_colsum=acs)), None, 0, be.stream()), "gemm a_colsum")      # (an error if the 256x256 NT kernel cannot serve: VdkGemmDesc.a_colsum)
            _g(be, kernels, _desc(a, b, cb, M, N, K, c_colsum=ccs), "gemm c_colsum")
        return {"c": c, "cb": cb, "a_colsum": acs, "c_colsum": ccs}

    got, _ = _run(be, dev, case)
    _all_served_by(kernels, 2)
    assert _rel(got["a_colsum"].sum(0).cpu(), a0.float().sum(0)) < 1e-5
    assert _rel(got["c_colsum"].sum(0).cpu(), got["cb"].float().sum(0).cpu()) < 1e-5


@pytest.mark.parametrize("Cin,H,Co,k,s,pd", [(8, 15, 72, 3, 2, 1), (16, 14, 264, 3, 1, 1), (8, 7, 64, 1, 1, 0)])
def test_gemm_implicit_conv(be, dev, Cin, H, Co, k, s, pd):
    """VdkConvGeom: forward, transposed (input gradient) and the `rows`-form weight gradient with the NHWC tensor guarded (pixels beyond the image read as zeros, never as
    the neighbouring memory)"""
    torch.manual_seed(13)
    Bt = 3
    OH = (H + 2 * pd - k) // s + 1
    x0 = torch.randn(Bt, H, H, Cin).bfloat16(); w0 = torch.randn(Co, Cin, k, k)
    wf0 = w0.permute(0, 2, 3, 1).reshape(Co, k * k * Cin).bfloat16()
    wd0 = w0.permute(1, 2, 3, 0).reshape(Cin, k * k * Co).bfloat16()
    dy0 = torch.randn(Bt * OH * OH, Co).bfloat16()
    M, K = Bt * OH * OH, k * k * Cin
    rows = M; Kw = (rows + 127) // 128 * 128
    want = torch.nn.functional.conv2d(x0.float().permute(0, 3, 1, 2), wf0.float().reshape(Co, k, k, Cin).permute(0, 3, 1, 2), stride=s, padding=pd).permute(0, 2, 3, 1).reshape(M, Co)

    def case(ar):
        x = ar.put(x0.reshape(-1), 0, "NHWC input"); wf = ar.put(wf0, 8, "weight"); wd = ar.put(wd0, 8, "weight (dgrad)"); dy = ar.put(dy0, 0, "dY")
        y = ar.out((M, Co), F32, 8, "conv out"); dx = ar.out((Bt * H * H, Cin), F32, 8, "conv dgrad"); dw = ar.out((Co, K), F32, 8, "conv wgrad")
        g = _abi.ConvGeom(Cin, H, H, OH, OH, k, k, s, pd, 0)
        d = _desc(x, wf, y, M, Co, K); d.lda = 0; d.conv = C.cast(C.pointer(g), C.c_void_p)
        ck(be, be.lib.vdk_gemm_bf16_nt(C.byref(d), None, 0, be.stream()), "conv fwd")
        gt = _abi.ConvGeom(Co, OH, OH, H, H, k, k, s, pd, 1)
        d2 = _desc(dy, wd, dx, Bt * H * H, Cin, k * k * Co); d2.lda = 0; d2.conv = C.cast(C.pointer(gt), C.c_void_p)
        ck(be, be.lib.vdk_gemm_bf16_nt(C.byref(d2), None, 0, be.stream()), "conv dgrad")
        gw = _abi.ConvGeom(Cin, H, H, OH, OH, k, k, s, pd, 0, rows)
        d3 = _desc(dy, x, dw, Co, K, Kw, trans=1); d3.lda = Co; d3.ldb = K; d3.conv = C.cast(C.pointer(gw), C.c_void_p)
        ck(be, be.lib.vdk_gemm_bf16_nt(C.byref(d3), None, 0, be.stream()), "conv wgrad")
        return {"y": y, "dx": dx, "dw": dw}

    got, _ = _run(be, dev, case)
    assert _rel(got["y"].cpu(), want) < 1e-5
    # both gradients against autograd on the same bf16-rounded operands (tolerance of tests/test_resnet_ops.py)
    xr = x0.float().permute(0, 3, 1, 2).clone().requires_grad_(True); wr = wf0.float().reshape(Co, k, k, Cin).permute(0, 3, 1, 2).clone().requires_grad_(True)
    torch.nn.functional.conv2d(xr, wr, stride=s, padding=pd).backward(dy0.float().reshape(Bt, OH, OH, Co).permute(0, 3, 1, 2))
    assert _rel(got["dx"].cpu().reshape(Bt, H, H, Cin), xr.grad.permute(0, 2, 3, 1)) < 1e-5
    assert _rel(got["dw"].cpu(), wr.grad.permute(0, 2, 3, 1).reshape(Co, K)) < 1e-5


# ------------------------------------------------------------------------------------------------------------------ other GEMMs
def _f32desc(a, b, c, M, N, K, **kw):
    d = _abi.GemmF32Desc()
    d.A, d.lda, d.B, d.ldb, d.C, d.ldc = a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(), c.stride(0)
    d.M, d.N, d.K, d.alpha = M, N, K, 1.0
    for k, v in kw.items():
        if isinstance(v, torch.Tensor):
            setattr(d, k, v.data_ptr())
            if k == "residual":
                d.ldr = v.stride(0)
        else:
            setattr(d, k, v)
    return d


@pytest.mark.parametrize("M,N,K", [(1, 8, 4), (37, 52, 36), (130, 264, 100)])
def test_gemm_f32(be, dev, M, N, K):
    """vdk_gemm_f32_nt: NT with bias + GELU + col_scale + padded residual, b_kmajor, a_kmajor + b_kmajor (weight-gradient form)"""
    torch.manual_seed(20)
    Ma = (M + 3) // 4 * 4                                                   # a_kmajor needs M % 4 == 0
    a0 = torch.randn(M, K); b0 = torch.randn(N, K); bias0 = torch.randn(N); res0 = torch.randn(M, N); cs0 = torch.rand(N) + 0.5
    at0 = torch.randn(K, Ma); bt0 = torch.randn(K, N)

    def case(ar):
        a = ar.put(a0, 4, "A"); b = ar.put(b0, 12, "B"); bias = ar.put(bias0); res = ar.put(res0, 4, "residual"); cs = ar.put(cs0)
        at = ar.put(at0, 4, "A k-major"); bt = ar.put(bt0, 4, "B k-major")
        c = ar.out((M, N), F32, 4, "C"); c2 = ar.out((M, N), F32, 4, "C b_kmajor"); c3 = ar.out((Ma, N), F32, 12, "C a_kmajor")
        ck(be, be.lib.vdk_gemm_f32_nt(C.byref(_f32desc(a, b, c, M, N, K, bias=bias, residual=res, act=_abi.ACT_GELU, col_scale=cs)), be.stream()), "gemm f32")
        ck(be, be.lib.vdk_gemm_f32_nt(C.byref(_f32desc(a, bt, c2, M, N, K, b_kmajor=1, alpha=0.5)), be.stream()), "gemm f32 b_kmajor")
        ck(be, be.lib.vdk_gemm_f32_nt(C.byref(_f32desc(at, bt, c3, Ma, N, K, a_kmajor=1, b_kmajor=1)), be.stream()), "gemm f32 a_kmajor")
        return {"c": c, "c2": c2, "c3": c3}

    got, _ = _run(be, dev, case)
    ref = (torch.nn.functional.gelu(a0.double() @ b0.double().T + bias0) * cs0 + res0)
    assert _rel(got["c"].cpu(), ref) < 2e-6 and _rel(got["c2"].cpu(), 0.5 * (a0.double() @ bt0.double())) < 2e-6 and _rel(got["c3"].cpu(), at0.double().T @ bt0.double()) < 2e-6


def test_gemm_f32_batched_and_k_split(be, dev):
    """batched strides (z1, z2) and the k_total split: slab z multiplies rows [z K, min((z + 1) K, k_total)) of k-major operands -- the last slab is ragged, and what follows the
    operands' k_total rows is guard"""
    torch.manual_seed(21)
    B1, B2, M, N, K = 2, 3, 37, 20, 36
    a0 = torch.randn(B1 * B2 * M, K); b0 = torch.randn(B1 * B2 * N, K)
    kt, kc = 150, 64                                                         # 3 slabs: 64 + 64 + 22 rows
    S = (kt + kc - 1) // kc
    at0 = torch.randn(kt, 40); bt0 = torch.randn(kt, 24)

    def case(ar):
        a = ar.put(a0, 4, "A"); b = ar.put(b0, 4, "B"); c = ar.out((B1 * B2 * M, N), F32, 4, "C")
        d = _f32desc(a, b, c, M, N, K, batch1=B1, batch2=B2)
        d.sa2, d.sa1, d.sb2, d.sb1, d.sc2, d.sc1 = M * a.stride(0), B2 * M * a.stride(0), N * b.stride(0), B2 * N * b.stride(0), M * c.stride(0), B2 * M * c.stride(0)
        ck(be, be.lib.vdk_gemm_f32_nt(C.byref(d), be.stream()), "gemm f32 batched")
        at = ar.put(at0, 4, "A k-major"); bt = ar.put(bt0, 8, "B k-major"); slabs = ar.out((S * 40, 24), F32, 0, "slabs")
        d2 = _f32desc(at, bt, slabs, 40, 24, kc, a_kmajor=1, b_kmajor=1, batch1=S, batch2=1, k_total=kt)
        d2.sa1, d2.sb1, d2.sc1 = kc * at.stride(0), kc * bt.stride(0), 40 * 24
        ck(be, be.lib.vdk_gemm_f32_nt(C.byref(d2), be.stream()), "gemm f32 k split")
        return {"c": c, "slabs": slabs}

    got, _ = _run(be, dev, case)
    ref = torch.bmm(a0.double().reshape(-1, M, K), b0.double().reshape(-1, N, K).transpose(1, 2)).reshape(-1, N)
    assert _rel(got["c"].cpu(), ref) < 2e-6
    assert _rel(got["slabs"].cpu().reshape(S, 40, 24).sum(0), at0.double().T @ bt0.double()) < 2e-6


@pytest.mark.parametrize("M,N,K", [(300, 320, 256)])
def test_gemm_fp8(be, dev, M, N, K):
    """vdk_quant_fp8 (flat, amax / scale device scalars guarded), vdk_fp8_scale_update, vdk_gemm_fp8_nt with padded lda / ldb (% 16) / ldc, vdk_gemm_fp8_nt_q8 with a padded
    ldo8 (% 8) and aux"""
    torch.manual_seed(22)
    x0 = torch.randn(M, K) * 2; w0 = torch.randn(N, K); bias0 = torch.randn(N); res0 = torch.randn(M, N)

    def case(ar):
        x = ar.put(x0.reshape(-1), 0, "x"); w = ar.put(w0.bfloat16().reshape(-1), 0, "w")
        amax = ar.put(torch.zeros(2), 0, "amax"); scale = ar.put(torch.ones(2), 0, "scale"); inv = ar.put(torch.ones(2), 0, "scale_inv")
        x8f = ar.out(M * K, U8, 0, "x8"); w8f = ar.out(N * K, U8, 0, "w8")
        ck(be, be.lib.vdk_quant_fp8(p(x), 1, M * K, None, p(x8f), 0, p(amax), be.stream()), "quant (amax pass)")
        ck(be, be.lib.vdk_quant_fp8(p(w), 0, N * K, None, p(w8f), 0, p(amax[1:]), be.stream()), "quant (amax pass)")
        ck(be, be.lib.vdk_fp8_scale_update(p(amax), p(scale), p(inv), 2, 0, 1.0, be.stream()), "scale update")
        ck(be, be.lib.vdk_quant_fp8(p(x), 1, M * K, p(scale), p(x8f), 0, p(amax), be.stream()), "quant")
        ck(be, be.lib.vdk_quant_fp8(p(w), 0, N * K, p(scale[1:]), p(w8f), 0, None, be.stream()), "quant")
        a8 = ar.put(x8f.reshape(M, K), 16, "A fp8"); b8 = ar.put(w8f.reshape(N, K), 32, "B fp8"); bias = ar.put(bias0, 0, "bias"); res = ar.put(res0, 4, "residual")
        c = ar.out((M, N), F32, 8, "C"); g = ar.out((M, N), BF, 8, "C gelu"); aux = ar.out((M, N), BF, 8, "aux"); o8 = ar.out((M, N), U8, 8, "out8"); oamax = ar.put(torch.zeros(1), 0, "out amax")
        ck(be, be.lib.vdk_gemm_fp8_nt(C.byref(_desc(a8, b8, c, M, N, K, bias=bias, residual=res)), 0, 0, p(inv), p(inv[1:]), be.stream()), "gemm fp8")
        ck(be, be.lib.vdk_gemm_fp8_nt_q8(C.byref(_desc(a8, b8, g, M, N, K, bias=bias, act=_abi.ACT_GELU, aux=aux)), 0, 0, p(inv), p(inv[1:]), p(o8), o8.stride(0), 0, None, p(oamax),
                                         be.stream()), "gemm fp8 q8")
        return {"x8": x8f, "w8": w8f, "amax": amax, "scale": scale, "inv": inv, "c": c, "g": g, "aux": aux, "o8": o8, "oamax": oamax}

    got, _ = _run(be, dev, case)
    assert _rel(got["c"].cpu(), x0 @ w0.bfloat16().float().T + bias0 + res0) < 5e-2           # the fp8 Linear tolerance of tests/test_gemm_fp8.py


# ------------------------------------------------------------------------------------------------------------------ attention
def _attention_case(be, B, N, H, dtype, legacy_api=False):
    D = H * 64
    torch.manual_seed(30)
    qkv0 = (torch.randn(B * N, 3 * D) * 1.5).to(dtype); qkv0[N // 2, :D] *= 4.0
    dout0 = torch.randn(B * N, D).to(dtype)

    def case(ar):
        # ld = 3 D + 8 and ldo = D + 24 shift the 16-byte row starts from row to row (the header asks for ld % 8 only); lddqkv = 3 D + 64 keeps them aligned
        qkv = ar.put(qkv0, 8, "qkv"); dout = ar.put(dout0, 24, "dout")
        o = ar.out((B * N, D), dtype, 24, "o"); lse = ar.out(B * H * N, F32, 0, "lse"); dqkv = ar.out((B * N, 3 * D), dtype, 64, "dqkv"); dvec = ar.out(B * H * N, F32, 0, "dvec")
        ldo = o.stride(0)
        # (o and dout share ldo in the ABI: both are padded by 24)
        if legacy_api:
            ck(be, be.lib.vdk_attention_fwd(p(qkv), qkv.stride(0), p(o), ldo, p(lse), B, N, H, 64, 0.125, be.stream()), "attention fwd")
            ck(be, be.lib.vdk_attention_bwd(p(qkv), qkv.stride(0), p(o), p(dout), ldo, p(lse), p(dqkv), dqkv.stride(0), p(dvec), B, N, H, 64, 0.125, be.stream()), "attention bwd")
        else:
            ck(be, be.lib.vdk_attention_fwd_dt(p(qkv), qkv.stride(0), p(o), ldo, p(lse), B, N, H, 64, 0.125, DT[dtype], be.stream()), "attention fwd")
            ck(be, be.lib.vdk_attention_bwd_dt(p(qkv), qkv.stride(0), p(o), p(dout), ldo, p(lse), p(dqkv), dqkv.stride(0), p(dvec), B, N, H, 64, 0.125, DT[dtype], be.stream()),
               "attention bwd")
        return {"o": o, "lse": lse, "dqkv": dqkv}

    return case


def _attention_run(be, dev, B, N, H, dtype, legacy_api=False):
    """I1 - I3, and (so that a result that is wrong in the same way in every run cannot pass) forward and backward against torch fp32 at the tolerances of tests/test_attention.py"""
    got, _ = _run(be, dev, _attention_case(be, B, N, H, dtype, legacy_api))
    D = H * 64
    torch.manual_seed(30)
    qkv = (torch.randn(B * N, 3 * D) * 1.5).to(dtype); qkv[N // 2, :D] *= 4.0
    x = qkv.float().reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    att = (x[0] * 0.125) @ x[1].transpose(-2, -1)
    oref = (att.softmax(-1) @ x[2]).transpose(1, 2).reshape(B * N, D)
    assert _rel(got["lse"].cpu().reshape(B, H, N), torch.logsumexp(att, -1)) < 1e-5
    assert _rel(got["o"].float().cpu(), oref) < 6e-3
    dout = torch.randn(B * N, D).to(dtype)                                    # (the second draw of _attention_case's generator sequence)
    qr = qkv.float().requires_grad_(True)
    xr = qr.reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    (((xr[0] * 0.125) @ xr[1].transpose(-2, -1)).softmax(-1) @ xr[2]).transpose(1, 2).reshape(B * N, D).backward(dout.float())
    for i, name in enumerate("qkv"):
        assert _rel(got["dqkv"][:, i * D:(i + 1) * D].float().cpu(), qr.grad[:, i * D:(i + 1) * D]) < 1.5e-2, name


_ATTN_N = [17, 50, 197, 224, 256, 257, 290, 577]


# B = H = 1: what lies beyond N is the guard; B * H > 1: it is another item's live data.  Every N in both forms on bf16 operands; fp16 operands (slow on the emulation) at one N
# of each kernel family
_ATTN = [(n, 1, 1, BF) for n in _ATTN_N] + [(n, 2, 2, BF) for n in _ATTN_N if n != 577] + [(577, 1, 2, BF)] + [(50, 2, 2, HF), (224, 1, 1, HF), (257, 1, 2, HF), (290, 1, 1, HF)]


@pytest.mark.parametrize("N,B,H,dtype", _ATTN, ids=[f"N{n}-B{b}H{h}-{'bf16' if dt == BF else 'fp16'}" for n, b, h, dt in _ATTN])
def test_attention_default_routing(be, dev, N, B, H, dtype):
    """vdk_attention_fwd_dt / _bwd_dt, default routing (LDS-resident kernels up to N = 256 / 224, streaming kernels beyond), all four pitches padded (+8, +24, +64)"""
    _attention_run(be, dev, B, N, H, dtype)


@pytest.mark.parametrize("B,N,H,dtype", [(1, 17, 1, BF), (2, 50, 2, BF), (1, 197, 1, BF), (2, 224, 1, BF), (2, 50, 1, HF)])
def test_attention_streaming_kernels_forced(be, dev, B, N, H, dtype, monkeypatch):
    """VDK_ATTN_LONG_MIN=1: the streaming kernels at short N -- single ragged chunks, whole tiles beyond N"""
    monkeypatch.setenv("VDK_ATTN_LONG_MIN", "1")
    _attention_run(be, dev, B, N, H, dtype)


@pytest.mark.parametrize("B,N,H", [(1, 17, 1), (2, 50, 2), (1, 197, 1), (1, 257, 1), (2, 290, 1)])
def test_attention_legacy_kernels(be, dev, B, N, H):
    """the flash-style kernels of round 1, forced, through the bf16-only entry points vdk_attention_fwd / vdk_attention_bwd"""
    be.lib.vdk_attention_force_legacy(1)
    try:
        _attention_run(be, dev, B, N, H, BF, legacy_api=True)
    finally:
        be.lib.vdk_attention_force_legacy(-1)


@pytest.mark.parametrize("grid", [1, 2])
@pytest.mark.parametrize("N", [45, 197, 290])
def test_attention_persistent_grid(be, dev, N, grid, monkeypatch):
    """VDK_ATTN_GRID: a workgroup walks over several (batch, head) items, prefetching the next item's tiles under the current one's -- the prefetch beyond the LAST item must not
    reach an output or leave a mark"""
    monkeypatch.setenv("VDK_ATTN_GRID", str(grid))
    _attention_run(be, dev, 3, N, 2, BF)


# ------------------------------------------------------------------------------------------------------------------ window attention
@pytest.mark.parametrize("windows,nW,H,use_idx", [(5, 0, 3, False), (8, 4, 2, True), (12, 4, 3, False), (3, 0, 1, True)])
def test_window_attention(be, dev, windows, nW, H, use_idx):
    """vdk_window_attention_fwd / _fwd_f32 / _bwd: 49-token windows, head dim 32, with and without the shifted-window mask, with and without rowidx, window counts that are no
    multiple of the per-workgroup count; both workspaces sized exactly, guarded and pattern-filled"""
    torch.manual_seed(40)
    N, hd = 49, 32
    Cc = H * hd
    T = windows * N
    qkv0 = torch.randn(T, 3 * Cc); dout0 = torch.randn(T, Cc).bfloat16()
    bias0 = torch.randn(H * N * N) * 0.5
    mask0 = torch.where(torch.rand(nW, N, N) < 0.2, -100.0, 0.0).reshape(-1) if nW else None
    idx0 = torch.randperm(T).to(I32) if use_idx else None
    nf = _need(be, be.lib.vdk_window_attention_fwd_workspace_bytes, nW, H); nb = _need(be, be.lib.vdk_window_attention_bwd_workspace_bytes, windows, nW, H)

    def case(ar):
        qkv = ar.put(qkv0.bfloat16(), 8, "qkv"); q32 = ar.put(qkv0, 4, "qkv f32"); dout = ar.put(dout0, 8, "dout"); bias = ar.put(bias0, 0, "bias")
        mask = ar.put(mask0, 0, "mask") if nW else None; idx = ar.put(idx0, 0, "rowidx") if use_idx else None
        o = ar.out((T, Cc), BF, 8, "o"); o32 = ar.out((T, Cc), F32, 4, "o f32"); lse = ar.out(windows * H * N, F32, 0, "lse")
        dqkv = ar.out((T, 3 * Cc), BF, 8, "dqkv"); dbias = ar.out(H * N * N, F32, 0, "dbias")
        wf = ar.out(nf, U8, 0, "fwd workspace"); wf2 = ar.out(nf, U8, 0, "fwd workspace (f32)"); wb = ar.out(nb, U8, 0, "bwd workspace")
        s = hd ** -0.5
        ck(be, be.lib.vdk_window_attention_fwd(p(qkv), qkv.stride(0), p(o), o.stride(0), p(lse), p(bias), p(mask), nW, windows, H, N, hd, s, p(idx), p(wf), nf, be.stream()), "wa fwd")
        ck(be, be.lib.vdk_window_attention_fwd_f32(p(q32), q32.stride(0), p(o32), o32.stride(0), p(bias), p(mask), nW, windows, H, N, hd, s, p(idx), p(wf2), nf, be.stream()), "wa fwd f32")
        ck(be, be.lib.vdk_window_attention_bwd(p(qkv), qkv.stride(0), p(o), p(dout), o.stride(0), p(lse), p(bias), p(mask), nW, windows, H, N, hd, s, p(idx), p(dqkv), dqkv.stride(0),
                                               p(dbias), p(wb), nb, be.stream()), "wa bwd")
        return {"o": o, "o32": o32, "lse": lse, "dqkv": dqkv, "dbias": dbias}

    _run(be, dev, case)


def test_relpos_bias_table_grad(be, dev):
    torch.manual_seed(41)
    H, N, R = 3, 49, 169
    dbias0 = torch.randn(H * N * N)
    rel = torch.randint(0, R, (N * N,))
    U = int(torch.bincount(rel, minlength=R).max())
    uses0 = torch.full((R, U), -1, dtype=I32)
    for r in range(R):
        w = torch.nonzero(rel == r).flatten()
        uses0[r, :w.numel()] = w.to(I32)

    def case(ar):
        dbias = ar.put(dbias0, 0, "dbias"); uses = ar.put(uses0.reshape(-1), 0, "uses"); dt = ar.out(R * H, F32, 0, "dtable")
        ck(be, be.lib.vdk_relpos_bias_table_grad(p(dbias), p(uses), R, U, H, N * N, p(dt), be.stream()), "relpos grad")
        return {"dtable": dt}

    got, _ = _run(be, dev, case)
    want = torch.zeros(R, H, dtype=torch.float64).index_add_(0, rel, dbias0.double().reshape(H, N * N).T)
    assert _rel(got["dtable"].cpu().reshape(R, H), want) < 1e-6


# ------------------------------------------------------------------------------------------------------------------ attention pool, norms of the margin head
@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,N,H", [(3, 37, 2), (1, 196, 1), (2, 577, 2)])
def test_attn_pool(be, dev, B, N, H, dtype):
    torch.manual_seed(50)
    D = H * 64
    q0 = torch.randn(D); kv0 = torch.randn(B * N, 2 * D).to(dtype); dout0 = torch.randn(B, D)

    def case(ar):
        q = ar.put(q0, 0, "q"); kv = ar.put(kv0, 8, "kv"); dout = ar.put(dout0, 4, "dout")
        out = ar.out((B, D), F32, 4, "out"); probs = ar.out(B * H * N, F32, 0, "probs"); dkv = ar.out((B * N, 2 * D), dtype, 24, "dkv"); dq = ar.out(B * D, F32, 0, "dq_part")
        if dtype == BF:         # the entries without a format parameter are the bf16 form
            ck(be, be.lib.vdk_attn_pool_fwd(p(q), p(kv), kv.stride(0), B, N, H, 0.125, p(out), out.stride(0), p(probs), be.stream()), "attn pool fwd")
            ck(be, be.lib.vdk_attn_pool_bwd(p(q), p(kv), kv.stride(0), p(probs), p(dout), dout.stride(0), B, N, H, 0.125, p(dkv), dkv.stride(0), p(dq), be.stream()), "attn pool bwd")
            out2 = ar.out((B, D), F32, 4, "out (dt entry)")
            ck(be, be.lib.vdk_attn_pool_fwd_dt(p(q), p(kv), kv.stride(0), B, N, H, 0.125, p(out2), out2.stride(0), None, 0, be.stream()), "attn pool fwd dt")
            return {"out": out, "probs": probs, "dkv": dkv, "dq": dq, "out2": out2}
        ck(be, be.lib.vdk_attn_pool_fwd_dt(p(q), p(kv), kv.stride(0), B, N, H, 0.125, p(out), out.stride(0), p(probs), DT[dtype], be.stream()), "attn pool fwd")
        ck(be, be.lib.vdk_attn_pool_bwd_dt(p(q), p(kv), kv.stride(0), p(probs), p(dout), dout.stride(0), B, N, H, 0.125, p(dkv), dkv.stride(0), p(dq), DT[dtype], be.stream()), "attn pool bwd")
        return {"out": out, "probs": probs, "dkv": dkv, "dq": dq}

    got, _ = _run(be, dev, case)
    k = kv0.float().reshape(B, N, 2, H, 64)
    pr = torch.softmax(torch.einsum("hd,bnhd->bhn", q0.reshape(H, 64), k[:, :, 0]) * 0.125, -1)
    assert _rel(got["out"].cpu(), torch.einsum("bhn,bnhd->bhd", pr, k[:, :, 1]).reshape(B, D)) < 1e-5


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,D,Cn,planes", [(5, 64, 37, 3), (70, 128, 1001, 3), (1, 64, 8, 1)])
def test_colnorm_rownorm(be, dev, B, D, Cn, planes, dtype):
    """vdk_colnorm_fwd(_dt) / _bwd and vdk_rownorm_fwd(_dt) / _bwd: the header defines zeros in columns C..Cp-1 of Wb and in rows / columns B..Bp-1 of fb / fbt: those belong to
    the windows (asserted zero); ldw, ldb, ldg, ldo, lddfh padded beyond"""
    torch.manual_seed(51)
    Cp, Bp = (Cn + 7) // 8 * 8, (B + 63) // 64 * 64
    w0 = torch.randn(D, Cn); f0 = torch.randn(B, D); dwh0 = torch.randn(D, Cp); dfh0 = torch.randn(B, D)

    def case(ar):
        w = ar.put(w0, 4, "W"); f = ar.put(f0.reshape(-1), 0, "feats"); dwh = ar.put(dwh0, 4, "dWh"); dfh = ar.put(dfh0, 4, "dfh")
        inv = ar.out(Cn, F32, 0, "inv"); wb = ar.out((planes * D, Cp), dtype, 8, "Wb"); dW = ar.out((D, Cn), F32, 4, "dW")
        fh = ar.out(B * D, F32, 0, "fh"); fb = ar.out(Bp * D, dtype, 0, "fb"); fbt = ar.out(planes * D * Bp, dtype, 0, "fbt"); finv = ar.out(B, F32, 0, "finv"); df = ar.out(B * D, F32, 0, "df")
        if dtype == BF:
            ck(be, be.lib.vdk_colnorm_fwd(p(w), w.stride(0), D, Cn, Cp, 1e-12, p(inv), p(wb), wb.stride(0), planes, be.stream()), "colnorm fwd")
            ck(be, be.lib.vdk_rownorm_fwd(p(f), B, Bp, D, 1e-12, p(fh), p(fb), p(fbt), p(finv), planes, be.stream()), "rownorm fwd")
        else:
            ck(be, be.lib.vdk_colnorm_fwd_dt(p(w), w.stride(0), D, Cn, Cp, 1e-12, p(inv), p(wb), wb.stride(0), planes, DT[dtype], be.stream()), "colnorm fwd")
            ck(be, be.lib.vdk_rownorm_fwd_dt(p(f), B, Bp, D, 1e-12, p(fh), p(fb), p(fbt), p(finv), planes, DT[dtype], be.stream()), "rownorm fwd")
        ck(be, be.lib.vdk_colnorm_bwd(p(w), w.stride(0), p(inv), p(dwh), dwh.stride(0), D, Cn, p(dW), dW.stride(0), be.stream()), "colnorm bwd")
        ck(be, be.lib.vdk_rownorm_bwd(p(fh), p(finv), p(dfh), dfh.stride(0), B, D, p(df), be.stream()), "rownorm bwd")
        return {"inv": inv, "wb": wb, "dW": dW, "fh": fh, "fb": fb, "fbt": fbt, "finv": finv, "df": df}

    got, _ = _run(be, dev, case)
    assert int(got["wb"][:, Cn:].count_nonzero()) == 0 and int(got["fb"].reshape(Bp, D)[B:].count_nonzero()) == 0 and int(got["fbt"].reshape(planes * D, Bp)[:, B:].count_nonzero()) == 0
    assert _rel(got["fh"].cpu().reshape(B, D), torch.nn.functional.normalize(f0)) < 1e-6
    assert _rel(got["wb"][:D, :Cn].float().cpu(), torch.nn.functional.normalize(w0, dim=0).to(dtype).float()) < 1e-3


# ------------------------------------------------------------------------------------------------------------------ row ops
_LN_SHAPES = [(10, 768), (7, 64), (33, 1024), (5, 1536), (21, 128), (9, 96), (17, 256), (150, 128), (77, 512), (300, 384), (1, 100)]


@pytest.mark.parametrize("T,Cc", _LN_SHAPES)
def test_layernorm(be, dev, T, Cc):
    """vdk_layernorm_fwd (f32 and both 16-bit outputs, strided x / y) and vdk_layernorm_bwd (dy 16-bit and f32, dres, dx f32 + 16-bit) with every pitch padded and the
    workspace sized exactly: all the C classes of test_layernorm_fwd_bwd, a one-row and a 300-row case"""
    torch.manual_seed(60)
    x0 = torch.randn(T, Cc) * 2 + 0.5; g0 = torch.randn(Cc); b0 = torch.randn(Cc); dy0 = torch.randn(T, Cc); dres0 = torch.randn(T, Cc)
    need = _need(be, be.lib.vdk_layernorm_bwd_workspace_bytes, T, Cc)

    def case(ar):
        x = ar.put(x0, 4, "x"); g = ar.put(g0, 0, "gamma"); b = ar.put(b0, 0, "beta"); dyb = ar.put(dy0.bfloat16(), 8, "dy bf16"); dyf = ar.put(dy0, 12, "dy f32"); dres = ar.put(dres0, 4, "dres")
        y = ar.out((T, Cc), F32, 4, "y f32"); yb = ar.out((T, Cc), BF, 8, "y bf16"); yh = ar.out((T, Cc), HF, 4, "y fp16")
        mean = ar.out(T, F32, 0, "mean"); rstd = ar.out(T, F32, 0, "rstd")
        dx = ar.out((T, Cc), F32, 4, "dx"); dxb = ar.out((T, Cc), BF, 8, "dxb"); dg = ar.out(Cc, F32, 0, "dgamma"); db = ar.out(Cc, F32, 0, "dbeta")
        dx2 = ar.out((T, Cc), F32, 8, "dx (f32 dy)"); dg2 = ar.out(Cc, F32, 0, "dgamma 2"); db2 = ar.out(Cc, F32, 0, "dbeta 2")
        ws = ar.out(need, U8, 0, "workspace"); ws2 = ar.out(need, U8, 0, "workspace 2")
        st = be.stream()
        ck(be, be.lib.vdk_layernorm_fwd(p(x), x.stride(0), T, Cc, p(g), p(b), 1e-6, p(y), y.stride(0), 1, p(mean), p(rstd), st), "ln fwd")
        ck(be, be.lib.vdk_layernorm_fwd(p(x), x.stride(0), T, Cc, p(g), p(b), 1e-6, p(yb), yb.stride(0), 0, None, None, st), "ln fwd bf16")
        ck(be, be.lib.vdk_layernorm_fwd(p(x), x.stride(0), T, Cc, p(g), p(b), 1e-6, p(yh), yh.stride(0), 2, None, None, st), "ln fwd fp16")
        ck(be, be.lib.vdk_layernorm_bwd(p(dyb), dyb.stride(0), 0, p(x), x.stride(0), p(mean), p(rstd), p(g), p(dres), dres.stride(0), T, Cc, p(dx), dx.stride(0), p(dxb), dxb.stride(0),
                                        p(dg), p(db), p(ws), need, st), "ln bwd")
        ck(be, be.lib.vdk_layernorm_bwd(p(dyf), dyf.stride(0), 1, p(x), x.stride(0), p(mean), p(rstd), p(g), None, 0, T, Cc, p(dx2), dx2.stride(0), None, 0, p(dg2), p(db2), p(ws2), need, st),
           "ln bwd f32")
        return {"y": y, "yb": yb, "yh": yh, "mean": mean, "rstd": rstd, "dx": dx, "dxb": dxb, "dg": dg, "db": db, "dx2": dx2, "dg2": dg2, "db2": db2}

    got, _ = _run(be, dev, case)
    assert _rel(got["y"].cpu(), torch.nn.functional.layer_norm(x0, (Cc,), g0, b0, 1e-6)) < 1e-6


@pytest.mark.parametrize("T,Cc", [(37, 256), (300, 768), (1, 132)])
def test_layernorm_q8(be, dev, T, Cc):
    torch.manual_seed(61)
    x0 = torch.randn(T, Cc); g0 = torch.randn(Cc); b0 = torch.randn(Cc)

    def case(ar):
        x = ar.put(x0, 4, "x"); g = ar.put(g0); b = ar.put(b0); scale = ar.put(torch.tensor([3.0]), 0, "scale"); amax = ar.put(torch.zeros(1), 0, "amax")
        y = ar.out((T, Cc), BF, 8, "y"); y8 = ar.out((T, Cc), U8, 4, "y8"); mean = ar.out(T, F32, 0, "mean"); rstd = ar.out(T, F32, 0, "rstd")
        ck(be, be.lib.vdk_layernorm_fwd_q8(p(x), x.stride(0), T, Cc, p(g), p(b), 1e-6, p(y), y.stride(0), p(mean), p(rstd), p(y8), y8.stride(0), 0, p(scale), p(amax), be.stream()), "ln q8")
        return {"y": y, "y8": y8, "mean": mean, "rstd": rstd, "amax": amax}

    got, _ = _run(be, dev, case)
    assert torch.equal(got["y"].cpu(), torch.nn.functional.layer_norm(x0, (Cc,), g0, b0, 1e-6).bfloat16()) or _rel(got["y"].float().cpu(), torch.nn.functional.layer_norm(x0, (Cc,), g0, b0, 1e-6)) < 4e-3


@pytest.mark.parametrize("B,F", [(40, 72), (300, 100), (1, 33)])
def test_batchnorm1d(be, dev, B, F):
    torch.manual_seed(62)
    x0 = torch.randn(B, F) * 2 + 0.5; g0 = torch.rand(F) + 0.5; b0 = torch.randn(F); dy0 = torch.randn(B, F)

    def case(ar):
        x = ar.put(x0, 4, "x"); g = ar.put(g0); b = ar.put(b0); dy = ar.put(dy0, 8, "dy"); rm = ar.put(torch.zeros(F), 0, "running_mean"); rv = ar.put(torch.ones(F), 0, "running_var")
        y = ar.out((B, F), F32, 4, "y"); sm = ar.out(F, F32, 0, "save_mean"); si = ar.out(F, F32, 0, "save_invstd"); ye = ar.out((B, F), F32, 1, "y eval")
        dx = ar.out((B, F), F32, 4, "dx"); dg = ar.out(F, F32, 0, "dgamma"); db = ar.out(F, F32, 0, "dbeta")
        st = be.stream()
        ck(be, be.lib.vdk_batchnorm1d_fwd(p(x), x.stride(0), B, F, p(g), p(b), 1e-5, 0.1, 1 if B > 1 else 0, p(rm), p(rv), p(y), y.stride(0), p(sm), p(si), st), "bn1d fwd")
        ck(be, be.lib.vdk_batchnorm1d_fwd(p(x), x.stride(0), B, F, p(g), p(b), 1e-5, 0.1, 0, p(rm), p(rv), p(ye), ye.stride(0), None, None, st), "bn1d eval")
        if B > 1:
            ck(be, be.lib.vdk_batchnorm1d_bwd(p(dy), dy.stride(0), p(x), x.stride(0), B, F, p(g), p(sm), p(si), p(dx), dx.stride(0), p(dg), p(db), st), "bn1d bwd")
            return {"y": y, "ye": ye, "rm": rm, "rv": rv, "sm": sm, "si": si, "dx": dx, "dg": dg, "db": db}
        return {"y": y, "ye": ye}

    _run(be, dev, case)


@pytest.mark.parametrize("S,n", [(9, 60), (2, 1003), (300, 72)])
def test_reductions(be, dev, S, n):
    """vdk_reduce_rows_f32 (ld > n), vdk_colsum_bf16, vdk_colsum_f32 (ld > N, exact workspaces)"""
    torch.manual_seed(63)
    x0 = torch.randn(S, n)
    nb = _need(be, be.lib.vdk_colsum_bf16_workspace_bytes, S, n - n % 8 or 8); nf = _need(be, be.lib.vdk_colsum_f32_workspace_bytes, S, n)
    nbf = n - n % 8 or 8

    def case(ar):
        x = ar.put(x0, 6, "x"); xb = ar.put(x0[:, :nbf].bfloat16(), 8, "x bf16")
        out = ar.out(n, F32, 0, "out"); cb = ar.out(nbf, F32, 0, "colsum bf16"); cf = ar.out(n, F32, 0, "colsum f32"); wb = ar.out(nb, U8, 0, "ws bf16"); wf = ar.out(nf, U8, 0, "ws f32")
        ck(be, be.lib.vdk_reduce_rows_f32(p(x), x.stride(0), S, n, p(out), 0.5, be.stream()), "reduce rows")
        ck(be, be.lib.vdk_colsum_bf16(p(xb), xb.stride(0), S, nbf, p(cb), p(wb), nb, be.stream()), "colsum bf16")
        ck(be, be.lib.vdk_colsum_f32(p(x), x.stride(0), S, n, p(cf), p(wf), nf, be.stream()), "colsum f32")
        return {"out": out, "cb": cb, "cf": cf}

    got, _ = _run(be, dev, case)
    assert _rel(got["out"].cpu(), x0.double().sum(0) * 0.5) < 1e-6 and _rel(got["cf"].cpu(), x0.double().sum(0)) < 1e-5


@pytest.mark.parametrize("dl", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,Cn", [(6, 1000), (1, 5), (300, 257)])
def test_losses(be, dev, B, Cn, dl):
    """vdk_softmax_ce(_amp) / vdk_bce_logits(_amp): the header DEFINES zeros in columns C..lddl-1 of the 16-bit gradient (they pad the contraction dim of the head GEMMs): that
    region (lddl = C rounded up to 8, plus 8) belongs to the window and is asserted to be zero; the guards lie beyond lddl"""
    torch.manual_seed(64)
    Cp = (Cn + 7) // 8 * 8 + 8
    lg0 = torch.randn(B, Cn) * 3; ya0 = torch.randint(0, Cn, (B,)); yb0 = torch.randint(0, Cn, (B,)); t0 = (torch.rand(B, Cn) > 0.5).float()

    def case(ar):
        lg = ar.put(lg0, 3, "logits"); ya = ar.put(ya0, 0, "ya"); yb = ar.put(yb0, 0, "yb"); t = ar.put(t0, 5, "targets"); ls = ar.put(torch.tensor([128.0]), 0, "loss_scale")
        loss = ar.out(B, F32, 0, "loss_rows"); dlb = ar.out((B, Cp), dl, 0, "dlogits16"); dlf = ar.out((B, Cn), F32, 3, "dlogits f32")
        loss2 = ar.out(B, F32, 0, "bce loss_rows"); dlb2 = ar.out((B, Cp), dl, 0, "bce dlogits16"); dlf2 = ar.out((B, Cn), F32, 1, "bce dlogits f32")
        st = be.stream()
        ck(be, be.lib.vdk_softmax_ce_amp(p(lg), lg.stride(0), B, Cn, p(ya), p(yb), 0.3, 0.05, 1.0 / B, p(ls), p(loss), p(dlb), dlb.stride(0), DT[dl], p(dlf), dlf.stride(0), st), "ce amp")
        ck(be, be.lib.vdk_bce_logits_amp(p(lg), lg.stride(0), p(t), t.stride(0), B, Cn, 1.0 / B, p(ls), 2.0, 0.25, p(loss2), p(dlb2), dlb2.stride(0), DT[dl], p(dlf2), dlf2.stride(0), st),
           "bce amp")
        outs = {"loss": loss, "dlb": dlb, "dlf": dlf, "loss2": loss2, "dlb2": dlb2, "dlf2": dlf2}
        if dl == BF:         # the entries without a loss scale write bf16
            l3 = ar.out(B, F32, 0, "loss_rows (plain)"); d3 = ar.out((B, Cp), BF, 0, "dlogits (plain)"); l4 = ar.out(B, F32, 0, "bce loss_rows (plain)"); d4 = ar.out((B, Cp), BF, 0, "bce dlogits (plain)")
            ck(be, be.lib.vdk_softmax_ce(p(lg), lg.stride(0), B, Cn, p(ya), None, 1.0, 0.0, 1.0 / B, p(l3), p(d3), d3.stride(0), None, 0, st), "ce")
            ck(be, be.lib.vdk_bce_logits(p(lg), lg.stride(0), p(t), t.stride(0), B, Cn, 1.0 / B, 0.0, 0.25, p(l4), p(d4), d4.stride(0), None, 0, st), "bce")
            outs.update({"l3": l3, "d3": d3, "l4": l4, "d4": d4})
        return outs

    got, _ = _run(be, dev, case)
    for k in ("dlb", "dlb2") + (("d3", "d4") if dl == BF else ()):
        assert int(got[k][:, Cn:].count_nonzero()) == 0, k                    # header: columns C..lddl-1 zeroed
    crit = torch.nn.CrossEntropyLoss(label_smoothing=0.05, reduction="none")
    assert _rel(got["loss"].cpu(), 0.3 * crit(lg0, ya0) + 0.7 * crit(lg0, yb0)) < 1e-6


@pytest.mark.parametrize("B,Cn", [(9, 1000), (1, 37), (300, 70)])
def test_topk_ohem_l2norm(be, dev, B, Cn):
    torch.manual_seed(65)
    x0 = torch.randn(B, Cn) * 2; lab0 = torch.randint(0, Cn, (B,))
    k = 5
    D4 = Cn - Cn % 4

    def case(ar):
        x = ar.put(x0, 3, "logits"); lab = ar.put(lab0, 0, "labels"); xf = ar.put(x0[:, :D4].reshape(-1), 0, "x")
        idx = ar.out(B * k, I64, 0, "topk idx"); val = ar.out(B * k, F32, 0, "topk values"); prob = ar.out(B, F32, 0, "prob_ws"); mask = ar.out(B, U8, 0, "mask"); nrm = ar.out(B * D4, F32, 0, "l2norm out")
        ck(be, be.lib.vdk_topk_rows(p(x), x.stride(0), B, Cn, k, p(idx), p(val), be.stream()), "topk")
        ck(be, be.lib.vdk_ohem_mask(p(x), x.stride(0), B, Cn, p(lab), max(B // 4, 1), 0.2, 255, p(prob), p(mask), be.stream()), "ohem")
        ck(be, be.lib.vdk_l2norm_rows(p(xf), p(nrm), B, D4, 1e-12, be.stream()), "l2norm")
        return {"idx": idx, "val": val, "mask": mask, "nrm": nrm}

    got, _ = _run(be, dev, case)
    rv, ri = torch.topk(x0, k, dim=1)
    assert torch.equal(got["val"].cpu().reshape(B, k), rv) and torch.equal(got["idx"].cpu().reshape(B, k), ri)


def test_softmax_rows_f32(be, dev):
    """in place; the header defines zeros in [cols, ld): the window is the whole [rows, ld] here, a further pitch cannot be expressed (ld IS the pitch), the guards lie around"""
    torch.manual_seed(66)
    rows, cols, ld = 37, 49, 56
    x0 = torch.randn(rows, ld)

    def case(ar):
        x = ar.put(x0.reshape(-1), 0, "x")
        ck(be, be.lib.vdk_softmax_rows_f32(p(x), ld, rows, cols, 0.5, be.stream()), "softmax rows")
        return {"x": x}

    got, _ = _run(be, dev, case)
    g = got["x"].cpu().reshape(rows, ld)
    assert int(g[:, cols:].count_nonzero()) == 0 and _rel(g[:, :cols], torch.softmax(0.5 * x0[:, :cols].double(), 1)) < 1e-6


# ------------------------------------------------------------------------------------------------------------------ flat passes
_FLAT_N = [1, 1003, 1023, 1024, 1025, 4097]


@pytest.mark.parametrize("n", _FLAT_N)
def test_optimizer_passes(be, dev, n):
    """vdk_sumsq_f32, vdk_sgd_step / _graph / _amp (all five buffers guarded), vdk_loss_scale_update, vdk_sam_first_step"""
    torch.manual_seed(70)
    p0 = torch.randn(n); g0 = torch.randn(n) * 0.1; m0 = torch.randn(n) * 0.01
    nws = _need(be, be.lib.vdk_sumsq_workspace_bytes)

    def case(ar):
        st = be.stream()
        g = ar.put(g0, 0, "grads"); nsq = ar.out(1, F32, 0, "normsq"); ws = ar.out(nws, U8, 0, "sumsq workspace")
        ck(be, be.lib.vdk_sumsq_f32(p(g), n, p(nsq), p(ws), nws, st), "sumsq")
        outs = {"nsq": nsq}
        for tag in ("plain", "graph", "amp16", "ampbf"):
            pp = ar.put(p0, 0, "params"); m = ar.put(m0, 0, "momentum"); e = ar.put(p0, 0, "ema"); p16 = ar.out(n, HF if tag == "amp16" else BF, 0, "params16")
            if tag == "plain":
                ck(be, be.lib.vdk_sgd_step(p(pp), p(g), p(m), p(e), p(p16), n, 0.01, 0.9, 5e-4, 1.0, p(nsq), 10.0, 0.99, 0, st), "sgd")
            elif tag == "graph":
                hyper = ar.put(torch.tensor([0.01, 0.9, 5e-4, 0.99, 0.0]), 0, "hyper")
                ck(be, be.lib.vdk_sgd_step_graph(p(pp), p(g), p(m), p(e), p(p16), n, p(hyper), 1.0, p(nsq), 10.0, st), "sgd graph")
            else:
                lst = ar.put(torch.tensor([1.0, 0.0, 0.0]), 0, "loss_state")
                ck(be, be.lib.vdk_sgd_step_amp(p(pp), p(g), p(m), p(e), p(p16), 2 if tag == "amp16" else 0, n, 0.01, 0.9, 5e-4, 1.0, p(lst), p(nsq), 10.0, 0.99, 0, st), "sgd amp")
                ck(be, be.lib.vdk_loss_scale_update(p(lst), p(nsq), 2.0, 0.5, 1, st), "loss scale update")
                outs["lst " + tag] = lst
            outs.update({"p " + tag: pp, "m " + tag: m, "e " + tag: e, "p16 " + tag: p16})
        ps = ar.put(p0, 0, "params (sam)"); old = ar.out(n, F32, 0, "old_params"); nsq2 = ar.out(1, F32, 0, "sam normsq"); ws2 = ar.out(nws, U8, 0, "sam workspace")
        ck(be, be.lib.vdk_sam_first_step(p(ps), p(g), p(old), n, 0.05, 1, p(nsq2), p(ws2), nws, st), "sam")
        outs.update({"ps": ps, "old": old, "nsq2": nsq2})
        return outs

    got, _ = _run(be, dev, case)
    assert abs(got["nsq"].item() - (g0.double() ** 2).sum().item()) < 1e-6 * (g0.double() ** 2).sum().item()
    assert torch.equal(got["p plain"].cpu(), got["p graph"].cpu()) and torch.equal(got["old"].cpu(), p0)


@pytest.mark.parametrize("n", _FLAT_N)
def test_elementwise_passes(be, dev, n):
    """vdk_cast_f32_bf16 / _f16, vdk_gelu_f32, vdk_dgelu_f32, vdk_mixup (these take n % 4 == 0: n rounded up), vdk_scale_dev_f32 (any n), vdk_rowscale_f32; vdk_quant_fp8 is in test_gemm_fp8"""
    torch.manual_seed(71)
    n4 = (n + 3) // 4 * 4                                                     # the casts take n % 4 == 0
    x0 = torch.randn(n); d0 = torch.randn(n4); x40 = torch.randn(n4)
    Bm = 4
    xm0 = torch.randn(Bm * n4); perm0 = torch.tensor([2, 0, 3, 1])
    sc0 = torch.rand(Bm) + 0.5

    def case(ar):
        st = be.stream()
        x = ar.put(x0, 0, "x"); x4 = ar.put(x40, 0, "x (n % 4 == 0)"); ob = ar.out(n4, BF, 0, "bf16"); oh = ar.out(n4, HF, 0, "fp16"); g = ar.out(n4, F32, 0, "gelu"); d = ar.put(d0, 0, "d (in place)")
        xs = ar.put(x0, 0, "x scaled in place"); s = ar.put(torch.tensor([0.25]), 0, "scale"); xr = ar.put(x0, 0, "x divided in place")
        xm = ar.put(xm0, 0, "mixup x"); perm = ar.put(perm0, 0, "perm"); om = ar.out(Bm * n4, F32, 0, "mixup out"); sc = ar.put(sc0, 0, "row scale"); ors = ar.out(Bm * n4, F32, 0, "rowscale out")
        ck(be, be.lib.vdk_cast_f32_bf16(p(x4), p(ob), n4, st), "cast bf16"); ck(be, be.lib.vdk_cast_f32_f16(p(x4), p(oh), n4, st), "cast f16")
        ck(be, be.lib.vdk_gelu_f32(p(x4), p(g), n4, st), "gelu"); ck(be, be.lib.vdk_dgelu_f32(p(d), p(x4), n4, st), "dgelu")
        ck(be, be.lib.vdk_scale_dev_f32(p(xs), n, p(s), 0, st), "scale"); ck(be, be.lib.vdk_scale_dev_f32(p(xr), n, p(s), 1, st), "scale reciprocal")
        ck(be, be.lib.vdk_mixup(p(xm), p(perm), 0.3, Bm, n4, p(om), st), "mixup")
        ck(be, be.lib.vdk_rowscale_f32(p(xm), p(sc), p(ors), Bm, n4, st), "rowscale")
        return {"ob": ob, "oh": oh, "g": g, "d": d, "xs": xs, "xr": xr, "om": om, "ors": ors}

    got, _ = _run(be, dev, case)
    assert torch.equal(got["ob"].cpu(), x40.bfloat16()) and torch.equal(got["oh"].cpu(), x40.half()) and torch.equal(got["xs"].cpu(), x0 * 0.25)
    assert _rel(got["om"].cpu().reshape(Bm, n4), 0.3 * xm0.reshape(Bm, n4) + 0.7 * xm0.reshape(Bm, n4)[perm0]) < 1e-6


@pytest.mark.parametrize("R,Cc", [(20, 12), (197, 72), (1, 8), (300, 264)])
def test_transposes_patchify_cls(be, dev, R, Cc):
    """vdk_transpose_bf16 (with and without in_row_group, with the column-sum by-product), vdk_transpose_cast_f32_bf16: rows R..Rpad-1 of the output are DEFINED zero (inside the
    window, asserted), ldo > Rpad beyond; vdk_patchify_bf16 / _f32 (zero-padded to Kp), vdk_cls_rows"""
    torch.manual_seed(72)
    Rp = (R + 63) // 64 * 64
    rg = 4 if R % 4 == 0 else 0
    x0 = torch.randn(R, Cc); phys = R + R // rg + 1 if rg else R
    xg0 = torch.randn(phys, Cc).bfloat16()
    img0 = torch.randn(2, 3, 28, 28); ps = 14; K = 3 * ps * ps; Kp = (K + 7) // 8 * 8
    Bt, D = 3, Cc
    tok0 = torch.randn(Bt * 5 * D); cls0 = torch.randn(D); pos00 = torch.randn(D)

    def case(ar):
        st = be.stream()
        xb = ar.put(x0.bfloat16(), 8, "in bf16"); xf = ar.put(x0, 4, "in f32"); xg = ar.put(xg0, 8, "in (row groups)")
        o = ar.out((Cc, Rp), BF, 8, "out"); cs = ar.out(((Rp + 63) // 64) * Cc, F32, 0, "colsum_partial"); o2 = ar.out((Cc, Rp), BF, 24, "out (cast)"); o3 = ar.out((Cc, Rp), BF, 8, "out (row groups)")
        ck(be, be.lib.vdk_transpose_bf16(p(xb), xb.stride(0), R, Cc, p(o), o.stride(0), Rp, 0, p(cs), st), "transpose")
        ck(be, be.lib.vdk_transpose_cast_f32_bf16(p(xf), xf.stride(0), R, Cc, p(o2), o2.stride(0), Rp, st), "transpose cast")
        outs = {"o": o, "cs": cs, "o2": o2}
        if rg:
            ck(be, be.lib.vdk_transpose_bf16(p(xg), xg.stride(0), R, Cc, p(o3), o3.stride(0), Rp, rg, None, st), "transpose row groups")
            outs["o3"] = o3
        img = ar.put(img0.reshape(-1), 0, "image"); pb = ar.out(2 * 4 * Kp, BF, 0, "patches bf16"); pf = ar.out(2 * 4 * K, F32, 0, "patches f32")
        ck(be, be.lib.vdk_patchify_bf16(p(img), 2, 3, 28, 28, ps, p(pb), Kp, st), "patchify")
        ck(be, be.lib.vdk_patchify_f32(p(img), 2, 3, 28, 28, ps, p(pf), st), "patchify f32")
        tok = ar.put(tok0, 0, "token buffer"); cls = ar.put(cls0, 0, "cls"); pos = ar.put(pos00, 0, "pos0")
        before = tok.clone()
        ck(be, be.lib.vdk_cls_rows(p(tok), 5 * D, Bt, D, p(cls), p(pos), st), "cls rows")
        outs.update({"pb": pb, "pf": pf, "cls rows": tok.reshape(Bt, 5, D)[:, 0], "other rows untouched": (tok.reshape(Bt, 5, D)[:, 1:] == before.reshape(Bt, 5, D)[:, 1:]).all().reshape(1)})
        return outs

    got, _ = _run(be, dev, case)
    assert torch.equal(got["o"][:, :R].cpu(), x0.bfloat16().T) and int(got["o"][:, R:].count_nonzero()) == 0
    assert torch.equal(got["o2"][:, :R].cpu(), x0.bfloat16().T) and int(got["o2"][:, R:].count_nonzero()) == 0
    assert bool(got["other rows untouched"].all())
    ref = torch.nn.functional.unfold(img0, ps, stride=ps).transpose(1, 2).reshape(-1, K)
    pbv = got["pb"].cpu().reshape(-1, Kp)
    assert torch.equal(pbv[:, :K], ref.bfloat16()) and int(pbv[:, K:].count_nonzero()) == 0 and torch.equal(got["pf"].cpu().reshape(-1, K), ref)


# ------------------------------------------------------------------------------------------------------------------ CNN pieces
@pytest.mark.parametrize("Bt,H,W,Cc", [(2, 7, 7, 40), (1, 15, 14, 72), (2, 14, 14, 96)])
def test_convnext_pieces(be, dev, Bt, H, W, Cc):
    """vdk_dwconv7_weight_prep / _fwd (both directions, with bias, shortcut and the 16-bit copy) / _wgrad, the space-to-depth pairs, the 2x2 and layer-scale weight forms,
    the f32 pooling pair: NHWC tensors are flat buffers, H, W odd and small, C no multiple of 64"""
    torch.manual_seed(80)
    x0 = torch.randn(Bt * H * W * Cc); w0 = torch.randn(Cc * 49); b0 = torch.randn(Cc); r0 = torch.randn(Bt * H * W * Cc); dy0 = torch.randn(Bt * H * W * Cc)
    He, We = H - H % 2, W - W % 2                                            # the stride-2 forms take even sides
    xe0 = torch.randn(Bt * He * We * Cc)
    Co, Ci, Mh = 24, 16, 4 * Cc
    w22 = torch.randn(Co * Ci * 4); dwp0 = torch.randn(Co * 4 * Ci); w2_0 = torch.randn(Cc * Mh); b2_0 = torch.randn(Cc); gm0 = torch.randn(Cc); dw2p0 = torch.randn(Cc * Mh)
    nws = _need(be, be.lib.vdk_dwconv7_wgrad_workspace_bytes, Bt, H, W, Cc)

    def case(ar):
        st = be.stream()
        x = ar.put(x0, 0, "in"); w = ar.put(w0, 0, "w"); b = ar.put(b0, 0, "bias"); r = ar.put(r0, 0, "res"); dy = ar.put(dy0, 0, "dy")
        wt = ar.out(49 * Cc, F32, 0, "wt"); y = ar.out(x0.numel(), F32, 0, "out"); yb = ar.out(x0.numel(), BF, 0, "out_bf16"); dx = ar.out(x0.numel(), F32, 0, "din")
        dw = ar.out(Cc * 49, F32, 0, "dw"); db = ar.out(Cc, F32, 0, "db"); ws = ar.out(nws, U8, 0, "wgrad workspace")
        ck(be, be.lib.vdk_dwconv7_weight_prep(p(w), p(wt), Cc, st), "dw weight prep")
        ck(be, be.lib.vdk_dwconv7_fwd(p(x), p(wt), p(b), p(r), p(y), p(yb), Bt, H, W, Cc, 0, st), "dwconv fwd")
        ck(be, be.lib.vdk_dwconv7_fwd(p(dy), p(wt), None, None, p(dx), None, Bt, H, W, Cc, 1, st), "dwconv dgrad")
        ck(be, be.lib.vdk_dwconv7_wgrad(p(x), p(dy), p(dw), p(db), Bt, H, W, Cc, p(ws), nws, st), "dwconv wgrad")
        xe = ar.put(xe0, 0, "in (even)"); xeb = ar.put(xe0.bfloat16(), 0, "in bf16 (even)")
        s2d = ar.out(xe0.numel(), BF, 0, "space to depth"); d2s = ar.out(xe0.numel(), BF, 0, "depth to space"); s2f = ar.out(xe0.numel(), F32, 0, "space to depth f32"); d2f = ar.out(xe0.numel(), F32, 0, "depth to space f32")
        ck(be, be.lib.vdk_space_to_depth2_bf16(p(xeb), p(s2d), Bt, He, We, Cc, 0, st), "s2d"); ck(be, be.lib.vdk_space_to_depth2_bf16(p(s2d), p(d2s), Bt, He, We, Cc, 1, st), "d2s")
        ck(be, be.lib.vdk_space_to_depth2_f32(p(xe), p(s2f), Bt, He, We, Cc, st), "s2d f32"); ck(be, be.lib.vdk_depth_to_space2_f32(p(s2f), p(d2f), Bt, He, We, Cc, st), "d2s f32")
        wq = ar.put(w22, 0, "conv2x2 w"); wb = ar.out(Co * 4 * Ci, BF, 0, "wb"); wtb = ar.out(4 * Ci * Co, BF, 0, "wtb"); dwp = ar.put(dwp0, 0, "dwp"); dwu = ar.out(Co * Ci * 4, F32, 0, "dw unpermuted")
        ck(be, be.lib.vdk_conv2x2_weight_prep(p(wq), p(wb), p(wtb), Co, Ci, st), "conv2x2 prep"); ck(be, be.lib.vdk_conv2x2_wgrad_unpermute(p(dwp), p(dwu), Co, Ci, st), "conv2x2 unpermute")
        w2 = ar.put(w2_0, 0, "w2"); b2 = ar.put(b2_0, 0, "b2"); gm = ar.put(gm0, 0, "gamma"); dw2p = ar.put(dw2p0, 0, "dw2p")
        w2p = ar.out(Cc * Mh, BF, 0, "w2p"); w2pt = ar.out(Mh * Cc, BF, 0, "w2pt"); b2p = ar.out(Cc, F32, 0, "b2p"); dw2 = ar.out(Cc * Mh, F32, 0, "dw2"); db2 = ar.out(Cc, F32, 0, "db2"); dgm = ar.out(Cc, F32, 0, "dgamma")
        ck(be, be.lib.vdk_layerscale_weight_prep(p(w2), p(b2), p(gm), p(w2p), p(w2pt), p(b2p), Cc, Mh, st), "layerscale prep")
        ck(be, be.lib.vdk_layerscale_grad(p(dw2p), p(b), p(w2), p(b2), p(gm), p(dw2), p(db2), p(dgm), Cc, Mh, st), "layerscale grad")
        pool = ar.out(Bt * Cc, F32, 0, "pooled"); dmap = ar.out(x0.numel(), F32, 0, "dmap"); dmapb = ar.out(x0.numel(), BF, 0, "dmap bf16")
        ck(be, be.lib.vdk_avgpool_rows_f32_fwd(p(x), p(pool), Bt, H * W, Cc, st), "avgpool rows fwd"); ck(be, be.lib.vdk_avgpool_rows_f32_bwd(p(pool), p(dmap), p(dmapb), Bt, H * W, Cc, st), "avgpool rows bwd")
        return {"wt": wt, "y": y, "yb": yb, "dx": dx, "dw": dw, "db": db, "s2d": s2d, "d2s": d2s, "s2f": s2f, "d2f": d2f, "wb": wb, "wtb": wtb, "dwu": dwu, "w2p": w2p, "w2pt": w2pt, "b2p": b2p,
                "dw2": dw2, "db2": db2, "dgm": dgm, "pool": pool, "dmap": dmap, "dmapb": dmapb}

    got, _ = _run(be, dev, case)
    xi = x0.reshape(Bt, H, W, Cc).permute(0, 3, 1, 2)
    want = torch.nn.functional.conv2d(xi, w0.reshape(Cc, 1, 7, 7), b0, padding=3, groups=Cc).permute(0, 2, 3, 1).reshape(-1) + r0
    assert _rel(got["y"].cpu(), want) < 1e-5 and torch.equal(got["d2s"].cpu(), xe0.bfloat16()) and torch.equal(got["d2f"].cpu(), xe0)


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("Bt,H,W,Cc", [(2, 7, 7, 40), (1, 15, 14, 72)])
def test_resnet_pieces(be, dev, Bt, H, W, Cc, dtype):
    """vdk_nchw_to_nhwc_bf16, vdk_im2col_bf16, vdk_conv_weight_prep / _wgrad_unpermute, vdk_bn_act_fwd / _bwd, vdk_bn_rows_bwd, vdk_maxpool3s2_fwd / _bwd (with and without the
    argmax map), vdk_avgpool_fwd / _bwd; both 16-bit formats through vdk_resnet_ops_format"""
    torch.manual_seed(81)
    R = Bt * H * W
    img0 = torch.randn(Bt * 3 * H * W); x0 = torch.randn(R * Cc); xr0 = torch.randn(R, Cc) * 2 + 0.3; res0 = torch.randn(R * Cc); g0 = torch.rand(Cc) + 0.5; b0 = torch.randn(Cc); dout0 = torch.randn(R * Cc)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dpo0 = torch.randn(Bt * OH * OW * Cc); Co, Ci = 24, 3
    w0 = torch.randn(Co * Ci * 9); dwp0 = torch.randn(Co * 9 * 8); dfeat0 = torch.randn(Bt, Cc)
    nws = _need(be, be.lib.vdk_bn_rows_workspace_bytes, R, Cc)
    Bp = 64

    def case(ar):
        st = be.stream()
        ck(be, be.lib.vdk_resnet_ops_format(DT[dtype]), "ops format")
        try:
            img = ar.put(img0, 0, "image"); nhwc = ar.out(R * 8, dtype, 0, "nhwc")
            ck(be, be.lib.vdk_nchw_to_nhwc_bf16(p(img), p(nhwc), Bt, 3, H, W, 8, st), "nchw to nhwc")
            xb = ar.put(x0.to(dtype), 0, "x16"); col = ar.out(Bt * OH * OW * 9 * Cc, dtype, 0, "col")
            ck(be, be.lib.vdk_im2col_bf16(p(xb), p(col), Bt, H, W, Cc, OH, OW, 3, 3, 2, 1, st), "im2col")
            w = ar.put(w0, 0, "w"); wf = ar.out(Co * 9 * 8, dtype, 0, "wf"); wd = ar.out(8 * 9 * Co, dtype, 0, "wd"); dwp = ar.put(dwp0, 0, "dwp"); dw = ar.out(Co * Ci * 9, F32, 0, "dw")
            ck(be, be.lib.vdk_conv_weight_prep(p(w), p(wf), p(wd), Co, Ci, 8, 3, 3, st), "conv weight prep"); ck(be, be.lib.vdk_conv_wgrad_unpermute(p(dwp), p(dw), Co, Ci, 8, 3, 3, st), "wgrad unpermute")
            x = ar.put(xr0.reshape(-1), 0, "x"); g = ar.put(g0, 0, "gamma"); b = ar.put(b0, 0, "beta"); rm = ar.put(torch.zeros(Cc), 0, "running_mean"); rv = ar.put(torch.ones(Cc), 0, "running_var")
            res = ar.put(res0, 0, "res"); dout = ar.put(dout0, 0, "dout")
            ob = ar.out(R * Cc, dtype, 0, "out16"); of = ar.out(R * Cc, F32, 0, "out f32"); sm = ar.out(Cc, F32, 0, "save_mean"); si = ar.out(Cc, F32, 0, "save_invstd"); ws = ar.out(nws, U8, 0, "bn workspace")
            ck(be, be.lib.vdk_bn_act_fwd(p(x), R, Cc, p(g), p(b), 1e-5, 0.1, 1, p(rm), p(rv), p(res), None, 1, p(ob), p(of), p(sm), p(si), p(ws), nws, None, None, st), "bn act fwd")
            dyb = ar.out(R * Cc, dtype, 0, "dy16"); dres = ar.out(R * Cc, F32, 0, "dres"); dg = ar.out(Cc, F32, 0, "dgamma"); db = ar.out(Cc, F32, 0, "dbeta"); ws2 = ar.out(nws, U8, 0, "bn workspace (bwd)")
            ck(be, be.lib.vdk_bn_act_bwd(p(x), p(dout), p(ob), R, Cc, p(g), p(sm), p(si), p(dyb), p(dres), p(dg), p(db), p(ws2), nws, None, None, st), "bn act bwd")
            outs = {"nhwc": nhwc, "col": col, "wf": wf, "wd": wd, "dw": dw, "ob": ob, "of": of, "sm": sm, "si": si, "rm": rm, "rv": rv, "dyb": dyb, "dres": dres, "dg": dg, "db": db}
            if Cc % 4 == 0:
                dxr = ar.out(R * Cc, F32, 0, "dx (rows)"); dg2 = ar.out(Cc, F32, 0, "dgamma (rows)"); db2 = ar.out(Cc, F32, 0, "dbeta (rows)"); ws3 = ar.out(nws, U8, 0, "bn workspace (rows)")
                ck(be, be.lib.vdk_bn_rows_bwd(p(x), p(dout), R, Cc, p(g), p(sm), p(si), p(dxr), p(dg2), p(db2), p(ws3), nws, None, None, st), "bn rows bwd")
                outs.update({"dxr": dxr, "dg2": dg2, "db2": db2})
            po = ar.out(Bt * OH * OW * Cc, dtype, 0, "pool out"); am = ar.out(Bt * OH * OW * Cc, U8, 0, "argmax"); dpo = ar.put(dpo0, 0, "dpool"); din = ar.out(R * Cc, F32, 0, "din"); din2 = ar.out(R * Cc, F32, 0, "din (argmax)")
            ck(be, be.lib.vdk_maxpool3s2_fwd(p(xb), p(po), p(am), Bt, H, W, Cc, st), "maxpool fwd")
            ck(be, be.lib.vdk_maxpool3s2_bwd(p(xb), None, p(dpo), p(din), Bt, H, W, Cc, st), "maxpool bwd"); ck(be, be.lib.vdk_maxpool3s2_bwd(None, p(am), p(dpo), p(din2), Bt, H, W, Cc, st), "maxpool bwd argmax")
            feat = ar.out(Bp * Cc, dtype, 0, "pooled features"); dfeat = ar.put(dfeat0.to(dtype), 8, "dfeat"); dmap = ar.out(R * Cc, F32, 0, "dmap")
            ck(be, be.lib.vdk_avgpool_fwd(p(xb), p(feat), Bt, Bp, H * W, Cc, st), "avgpool fwd"); ck(be, be.lib.vdk_avgpool_bwd(p(dfeat), dfeat.stride(0), p(dmap), Bt, H * W, Cc, st), "avgpool bwd")
            outs.update({"po": po, "am": am, "din": din, "din2": din2, "feat": feat, "dmap": dmap})
        finally:
            be.lib.vdk_resnet_ops_format(0)
        return outs

    got, _ = _run(be, dev, case)
    assert torch.equal(got["din"].cpu(), got["din2"].cpu())
    bn = torch.nn.functional.batch_norm(xr0, None, None, g0, b0, True, 0.1, 1e-5)
    assert _rel(got["of"].cpu().reshape(R, Cc), torch.relu(bn + res0.reshape(R, Cc))) < 1e-5


# ------------------------------------------------------------------------------------------------------------------ margin head
def _head(mode):
    return {0: _abi.MarginHead(0, 32.0, 0.35, 0.0, 0.0, None), 1: _abi.MarginHead(1, 64.0, 0.25, 0.0, 0.0, None), 2: _abi.MarginHead(2, 32.0, 0.35, 0.0, 1.12, None),
            3: _abi.MarginHead(3, 32.0, 0.35, 0.0, 1.12, None)}[mode]


@pytest.mark.parametrize("mode", [0, 1, 3])
@pytest.mark.parametrize("B,Cn", [(5, 37), (70, 1001)])
def test_margin_ce_family(be, dev, B, Cn, mode):
    """vdk_margin_ce / _amp / _f32 / _bwd on a padded cos (ldc), padded logits (ldl); the padding columns C..lddc-1 of dcos are DEFINED zero: inside the window, asserted"""
    torch.manual_seed(90)
    Cp = (Cn + 7) // 8 * 8 + 8
    cos0 = torch.rand(B, Cn) * 1.8 - 0.9; lab0 = torch.randint(0, Cn, (B,)); dlog0 = torch.randn(B, Cn)

    def case(ar):
        st = be.stream()
        h = _head(mode)
        cos = ar.put(cos0, 12, "cos"); lab = ar.put(lab0, 0, "labels"); dlog = ar.put(dlog0, 4, "dlogits"); ls = ar.put(torch.tensor([64.0]), 0, "loss_scale")
        lg = ar.out((B, Cn), F32, 5, "logits"); loss = ar.out(B, F32, 0, "loss_rows"); dc = ar.out((B, Cp), BF, 0, "dcos"); dch = ar.out((B, Cp), HF, 0, "dcos fp16"); loss2 = ar.out(B, F32, 0, "loss_rows amp")
        dcf = ar.out((B, Cp), F32, 0, "dcos f32"); loss3 = ar.out(B, F32, 0, "loss_rows f32"); dcb = ar.out((B, Cp), BF, 0, "dcos (bwd)")
        ck(be, be.lib.vdk_margin_ce(C.byref(h), p(cos), cos.stride(0), B, Cn, p(lab), 0.1, 1.0 / B, p(lg), lg.stride(0), p(loss), p(dc), dc.stride(0), st), "margin ce")
        ck(be, be.lib.vdk_margin_ce_amp(C.byref(h), p(cos), cos.stride(0), B, Cn, p(lab), 0.1, 1.0 / B, p(ls), None, 0, p(loss2), p(dch), dch.stride(0), 2, st), "margin ce amp")
        ck(be, be.lib.vdk_margin_ce_f32(C.byref(h), p(cos), cos.stride(0), B, Cn, p(lab), 0.1, 1.0 / B, p(loss3), p(dcf), dcf.stride(0), st), "margin ce f32")
        ck(be, be.lib.vdk_margin_bwd(C.byref(h), p(cos), cos.stride(0), B, Cn, p(lab), p(dlog), dlog.stride(0), p(dcb), dcb.stride(0), st), "margin bwd")
        return {"lg": lg, "loss": loss, "dc": dc, "dch": dch, "loss2": loss2, "dcf": dcf, "loss3": loss3, "dcb": dcb}

    got, _ = _run(be, dev, case)
    for k in ("dc", "dch", "dcf", "dcb"):
        assert int(got[k][:, Cn:].count_nonzero()) == 0, k
    assert torch.equal(got["loss"].cpu(), got["loss2"].cpu())
    assert _rel(got["loss"].cpu(), torch.nn.functional.cross_entropy(got["lg"].cpu(), lab0, label_smoothing=0.1, reduction="none")) < 1e-5


@pytest.mark.parametrize("mode,amp", [(0, False), (3, False), (0, True)], ids=["arcface", "mv_arc", "arcface-amp"])      # (the amp pair evaluates plain ArcFace)
def test_margin_sharded(be, dev, mode, amp):
    """the class-sharded head: vdk_margin_target_cos, vdk_margin_stats(_amp), vdk_margin_grad(_amp) over two column shards, the last one ragged (C = 1001 = 504 + 497)"""
    torch.manual_seed(91)
    B, Ct = 37, 1001
    shards = [(0, 504), (504, 497)]
    cosf = torch.rand(B, Ct) * 1.8 - 0.9; lab0 = torch.randint(0, Ct, (B,))
    gmax0 = torch.randn(B).abs() + 30; gsum0 = torch.rand(B) + 1

    def case(ar):
        st = be.stream()
        h = _head(mode)
        outs = {}
        lab = ar.put(lab0, 0, "labels"); ls = ar.put(torch.tensor([64.0]), 0, "loss_scale"); gmax = ar.put(gmax0, 0, "gmax"); gsum = ar.put(gsum0, 0, "gsum")
        gts = []
        for i, (c0, cl) in enumerate(shards):
            cos = ar.put(cosf[:, c0:c0 + cl].contiguous(), 4, f"cos shard {i}"); gt = ar.out(B, F32, 0, f"gt {i}")
            ck(be, be.lib.vdk_margin_target_cos(p(cos), cos.stride(0), B, cl, c0, p(lab), p(gt), st), "target cos")
            gts.append((cos, gt)); outs[f"gt{i}"] = gt
        gtsum = ar.put((gts[0][1] + gts[1][1]).cpu() if not ar.plain else gts[0][1] + gts[1][1], 0, "gt (summed)")
        for i, (c0, cl) in enumerate(shards):
            cos = gts[i][0]
            clp = (cl + 7) // 8 * 8 + 8
            stats = ar.out(B * 4, F32, 0, f"stats {i}"); dc = ar.out((B, clp), HF if amp else BF, 0, f"dcos {i}")
            if amp:
                ck(be, be.lib.vdk_margin_stats_amp(C.byref(h), p(cos), cos.stride(0), B, cl, c0, p(lab), p(gtsum), p(stats), st), "stats amp")
                ck(be, be.lib.vdk_margin_grad_amp(C.byref(h), p(cos), cos.stride(0), B, cl, c0, Ct, p(lab), p(gtsum), p(gmax), p(gsum), 0.1, 1.0 / B, p(ls), p(dc), dc.stride(0), 2, st), "grad amp")
            else:
                ck(be, be.lib.vdk_margin_stats(C.byref(h), p(cos), cos.stride(0), B, cl, c0, p(lab), p(gtsum), p(stats), st), "stats")
                ck(be, be.lib.vdk_margin_grad(C.byref(h), p(cos), cos.stride(0), B, cl, c0, Ct, p(lab), p(gtsum), p(gmax), p(gsum), 0.1, 1.0 / B, p(dc), dc.stride(0), st), "grad")
            outs[f"stats{i}"] = stats; outs[f"dc{i}"] = dc
        return outs

    got, _ = _run(be, dev, case)
    assert torch.equal((got["gt0"] + got["gt1"]).cpu(), cosf[torch.arange(B), lab0])
    assert int(got["dc1"][:, 497:].count_nonzero()) == 0 and int(got["dc0"][:, 504:].count_nonzero()) == 0


@pytest.mark.parametrize("mode", [0, 2])
def test_margin_fused_cos_passes(be, dev, mode):
    """vdk_margin_cos_pass (1: statistics, 2: gradient) + vdk_margin_rowstat + vdk_margin_target_cos_direct on padded fbt / wb planes; rows >= B and columns >= C of dcos are
    DEFINED zero (inside the window, asserted)"""
    torch.manual_seed(92)
    B, Bp, D, Cn = 70, 128, 64, 1001
    Cp = (Cn + 7) // 8 * 8
    K = D
    f = torch.nn.functional.normalize(torch.randn(B, D)); w = torch.nn.functional.normalize(torch.randn(D, Cn), dim=0)
    fbt0 = torch.zeros(K, Bp); fbt0[:, :B] = f.T; wb0 = torch.zeros(K, Cp); wb0[:, :Cn] = w
    lab0 = torch.randint(0, Cn, (B,))
    nsl = (Cp + 63) // 64
    rcs = []

    def case(ar):
        st = be.stream()
        h = _head(mode)
        fbt = ar.put(fbt0.bfloat16(), 8, "fbt"); wb = ar.put(wb0.bfloat16(), 8, "wb"); lab = ar.put(lab0, 0, "labels")
        gt = ar.out(B, F32, 0, "gt"); stats = ar.out(B * nsl * 4, F32, 0, "stats"); tl = ar.put(torch.zeros(B), 0, "tlogit"); rowstat = ar.out(B * 2, F32, 0, "rowstat"); loss = ar.out(B, F32, 0, "loss_rows")
        dc = ar.out((Bp, Cp), BF, 8, "dcos")
        ck(be, be.lib.vdk_margin_target_cos_direct(p(fbt), fbt.stride(0), p(wb), wb.stride(0), K, B, p(lab), p(gt), st), "target cos direct")
        gtp = p(gt) if mode >= 2 else None
        rc = be.lib.vdk_margin_cos_pass(C.byref(h), 1, p(fbt), fbt.stride(0), p(wb), wb.stride(0), B, Bp, Cn, Cp, K, p(lab), gtp, p(stats), p(tl), None, 0.1, 1.0 / B, None, 0, st)
        rcs.append(rc)
        ck(be, rc, "cos pass 1")
        ck(be, be.lib.vdk_margin_rowstat(p(stats), nsl, p(tl), B, Cn, 0.1, p(rowstat), p(loss), st), "rowstat")
        ck(be, be.lib.vdk_margin_cos_pass(C.byref(h), 2, p(fbt), fbt.stride(0), p(wb), wb.stride(0), B, Bp, Cn, Cp, K, p(lab), gtp, None, None, p(rowstat), 0.1, 1.0 / B, p(dc), dc.stride(0), st), "cos pass 2")
        return {"gt": gt, "stats": stats, "tl": tl, "rowstat": rowstat, "loss": loss, "dc": dc}

    got, _ = _run(be, dev, case)
    assert int(got["dc"][B:].count_nonzero()) == 0 and int(got["dc"][:, Cn:].count_nonzero()) == 0


# ------------------------------------------------------------------------------------------------------------------ retrieval, preprocess
@pytest.mark.parametrize("nq,N,D,k", [(5, 333, 64, 10), (33, 77, 128, 40)])
def test_cbir(be, dev, nq, N, D, k):
    """vdk_cbir_prepare_gallery, vdk_cbir_search, _search_fast (D <= 128), _search_fast2 (guaranteed and staged schedules), vdk_cbir_merge_topk: workspaces sized exactly, guarded
    and pattern-filled, Gb / gnorm_ws / gmax_bits guarded; N and nq no multiples of 32 (ragged tails of every kernel).  Complements tests/test_cbir_tails.py, which plants
    values in the tail positions; here the surroundings are poison."""
    import numpy as np
    from oracle import cbir as ocbir
    rng = np.random.default_rng(7)
    g0 = torch.from_numpy(ocbir.l2norm_rows(rng.standard_normal((N, D), dtype=np.float32))); q0 = torch.from_numpy(ocbir.l2norm_rows(rng.standard_normal((nq, D), dtype=np.float32)))
    DP = (D + 127) // 128 * 128
    cap = max(2048, 2 * k)
    n1 = _need(be, be.lib.vdk_cbir_workspace_bytes, nq, k, cap); n2 = _need(be, be.lib.vdk_cbir_fast_workspace_bytes, nq, k, cap); n3 = _need(be, be.lib.vdk_cbir_fast2_workspace_bytes, nq, D, k, cap)
    S = 3
    nm = _need(be, be.lib.vdk_cbir_workspace_bytes, nq, k, max(S * k, 2 * k))

    def case(ar):
        st = be.stream()
        G = ar.put(g0.reshape(-1), 0, "G"); Q = ar.put(q0.reshape(-1), 0, "Q")
        Gb = ar.out(N * DP, BF, 0, "Gb"); gn = ar.out(3 * N, F32, 0, "gnorm_ws"); gm = ar.put(torch.zeros(4, dtype=I32), 0, "gmax_bits")
        ck(be, be.lib.vdk_cbir_prepare_gallery(p(G), N, D, p(Gb), p(gn), p(gm), st), "prepare gallery")
        outs = {"Gb": Gb, "gmax": gm[:3]}
        s1 = ar.out(nq * k, F32, 0, "scores"); i1 = ar.out(nq * k, I64, 0, "idx"); w1 = ar.out(n1, U8, 0, "search workspace")
        ck(be, be.lib.vdk_cbir_search(p(Q), nq, p(G), N, D, k, 100, p(s1), p(i1), cap, p(w1), n1, st), "search")
        s2 = ar.out(nq * k, F32, 0, "scores fast"); i2 = ar.out(nq * k, I64, 0, "idx fast"); w2 = ar.out(n2, U8, 0, "fast workspace")
        ck(be, be.lib.vdk_cbir_search_fast(p(Q), nq, p(G), p(Gb), p(gm), N, D, k, 100, p(s2), p(i2), cap, p(w2), n2, st), "search fast")
        outs.update({"s1": s1, "i1": i1, "s2": s2, "i2": i2})
        for sched in (0, 1024):
            s3 = ar.out(nq * k, F32, 0, "scores fast2"); i3 = ar.out(nq * k, I64, 0, "idx fast2"); w3 = ar.out(n3, U8, 0, "fast2 workspace"); ov = ar.put(torch.zeros(1, dtype=I32), 0, "overflow_out")
            ck(be, be.lib.vdk_cbir_search_fast2(p(Q), nq, p(G), 1, p(Gb), p(gm), N, D, k, 100, p(s3), p(i3), cap, sched, p(ov), p(w3), n3, st), "search fast2")
            outs.update({f"s3 {sched}": s3, f"i3 {sched}": i3, f"ov {sched}": ov})
        sh_s = torch.stack([s1.reshape(nq, k).cpu()] * S).reshape(-1).clone(); sh_i = torch.stack([i1.reshape(nq, k).cpu() + 10000 * s for s in range(S)]).reshape(-1)
        ss = ar.put(sh_s, 0, "shard scores"); si = ar.put(sh_i, 0, "shard idx"); ms = ar.out(nq * k, F32, 0, "merged scores"); mi = ar.out(nq * k, I64, 0, "merged idx"); wm = ar.out(nm, U8, 0, "merge workspace")
        ck(be, be.lib.vdk_cbir_merge_topk(p(ss), p(si), S, nq, k, p(ms), p(mi), p(wm), nm, st), "merge")
        outs.update({"ms": ms, "mi": mi})
        return outs

    got, _ = _run(be, dev, case)
    so, io = ocbir.flat_ip_search(q0.numpy(), g0.numpy(), k)
    io = np.where(io >= 0, io + 100, io)
    for s_, i_ in (("s1", "i1"), ("s2", "i2"), ("s3 0", "i3 0"), ("s3 1024", "i3 1024")):
        assert int(got["ov 0"].item()) == 0 and int(got["ov 1024"].item()) == 0
        assert (got[i_].cpu().numpy().reshape(nq, k) == io).all() and (got[s_].cpu().numpy().reshape(nq, k).view(np.uint32) == so.view(np.uint32)).all(), s_


def test_preprocess(be, dev):
    """vdk_preprocess_resize_pad_normalize: ragged image sizes of tests/test_preprocess.py, the packed pixel buffer extended to a multiple of 16 bytes as the header asks (the
    extension is part of the operand, the guards lie beyond), workspace sized exactly"""
    torch.manual_seed(95)
    sizes = [(37, 53), (64, 64), (5, 120), (130, 31)]
    S = 32
    px, offs = [], []
    o = 0
    for (w, h) in sizes:
        offs.append(o); t = torch.randint(0, 256, (h * w * 3,), dtype=U8); px.append(t); o += t.numel()
        padn = (-o) % 16
        if padn:
            px.append(torch.zeros(padn, dtype=U8)); o += padn
    pix0 = torch.cat(px); B = len(sizes); ms = max(max(s) for s in sizes)
    nws = _need(be, be.lib.vdk_preprocess_workspace_bytes, B, S, ms)

    def case(ar):
        pix = ar.put(pix0, 0, "pixels"); off = ar.put(torch.tensor(offs, dtype=I64), 0, "offsets"); wh = ar.put(torch.tensor(sizes, dtype=I32).reshape(-1), 0, "wh")
        out = ar.out(B * 3 * S * S, F32, 0, "out"); status = ar.out(B, I32, 0, "status"); ws = ar.out(nws, U8, 0, "workspace")
        ck(be, be.lib.vdk_preprocess_resize_pad_normalize(p(pix), p(off), p(wh), B, S, ms, 0.485, 0.456, 0.406, 0.229, 0.224, 0.225, p(out), p(status), p(ws), nws, be.stream()), "preprocess")
        return {"out": out, "status": status}

    got, _ = _run(be, dev, case)
    assert int(got["status"].count_nonzero()) == 0


# ------------------------------------------------------------------------------------------------------------------ the list of entries is tied to the header
# ABI name -> the test that runs the entry on guarded operands (a *_workspace_bytes query counts as covered by sizing a guarded workspace exactly; the engine entries by the
# wrapper calls of tests/test_workspace_isolation.py)
COVERED = {
    "vdk_l2norm_rows": "tests.test_extent_isolation::test_topk_ohem_l2norm",
    "vdk_cbir_workspace_bytes": "tests.test_extent_isolation::test_cbir",
    "vdk_cbir_search": "tests.test_extent_isolation::test_cbir",
    "vdk_cbir_prepare_gallery": "tests.test_extent_isolation::test_cbir",
    "vdk_cbir_fast_workspace_bytes": "tests.test_extent_isolation::test_cbir",
    "vdk_cbir_search_fast": "tests.test_extent_isolation::test_cbir",
    "vdk_cbir_fast2_workspace_bytes": "tests.test_extent_isolation::test_cbir",
    "vdk_cbir_search_fast2": "tests.test_extent_isolation::test_cbir",
    "vdk_cbir_merge_topk": "tests.test_extent_isolation::test_cbir",
    "vdk_gemm_splitk_workspace_bytes": "tests.test_extent_isolation::test_gemm_tn_and_splitk",
    "vdk_gemm_streamk_workspace_bytes": "tests.test_extent_isolation::test_gemm_stream_k",
    "vdk_gemm_bf16_nt": "tests.test_extent_isolation::test_gemm_nt_epilogues",
    "vdk_quant_fp8": "tests.test_extent_isolation::test_gemm_fp8",
    "vdk_fp8_scale_update": "tests.test_extent_isolation::test_gemm_fp8",
    "vdk_gemm_fp8_nt": "tests.test_extent_isolation::test_gemm_fp8",
    "vdk_gemm_fp8_nt_q8": "tests.test_extent_isolation::test_gemm_fp8",
    "vdk_transpose_bf16": "tests.test_extent_isolation::test_transposes_patchify_cls",
    "vdk_attention_fwd": "tests.test_extent_isolation::test_attention_legacy_kernels",
    "vdk_attention_bwd": "tests.test_extent_isolation::test_attention_legacy_kernels",
    "vdk_attention_fwd_dt": "tests.test_extent_isolation::test_attention_default_routing",
    "vdk_attention_bwd_dt": "tests.test_extent_isolation::test_attention_default_routing",
    "vdk_layernorm_fwd": "tests.test_extent_isolation::test_layernorm",
    "vdk_layernorm_fwd_q8": "tests.test_extent_isolation::test_layernorm_q8",
    "vdk_layernorm_bwd_workspace_bytes": "tests.test_extent_isolation::test_layernorm",
    "vdk_layernorm_bwd": "tests.test_extent_isolation::test_layernorm",
    "vdk_batchnorm1d_fwd": "tests.test_extent_isolation::test_batchnorm1d",
    "vdk_batchnorm1d_bwd": "tests.test_extent_isolation::test_batchnorm1d",
    "vdk_reduce_rows_f32": "tests.test_extent_isolation::test_reductions",
    "vdk_colsum_bf16_workspace_bytes": "tests.test_extent_isolation::test_reductions",
    "vdk_colsum_bf16": "tests.test_extent_isolation::test_reductions",
    "vdk_softmax_ce": "tests.test_extent_isolation::test_losses",
    "vdk_bce_logits": "tests.test_extent_isolation::test_losses",
    "vdk_softmax_ce_amp": "tests.test_extent_isolation::test_losses",
    "vdk_bce_logits_amp": "tests.test_extent_isolation::test_losses",
    "vdk_patchify_bf16": "tests.test_extent_isolation::test_transposes_patchify_cls",
    "vdk_cls_rows": "tests.test_extent_isolation::test_transposes_patchify_cls",
    "vdk_cast_f32_bf16": "tests.test_extent_isolation::test_elementwise_passes",
    "vdk_cast_f32_f16": "tests.test_extent_isolation::test_elementwise_passes",
    "vdk_transpose_cast_f32_bf16": "tests.test_extent_isolation::test_transposes_patchify_cls",
    "vdk_sumsq_workspace_bytes": "tests.test_extent_isolation::test_optimizer_passes",
    "vdk_sumsq_f32": "tests.test_extent_isolation::test_optimizer_passes",
    "vdk_sgd_step": "tests.test_extent_isolation::test_optimizer_passes",
    "vdk_sgd_step_graph": "tests.test_extent_isolation::test_optimizer_passes",
    "vdk_sgd_step_amp": "tests.test_extent_isolation::test_optimizer_passes",
    "vdk_loss_scale_update": "tests.test_extent_isolation::test_optimizer_passes",
    "vdk_sam_first_step": "tests.test_extent_isolation::test_optimizer_passes",
    "vdk_ohem_mask": "tests.test_extent_isolation::test_topk_ohem_l2norm",
    "vdk_topk_rows": "tests.test_extent_isolation::test_topk_ohem_l2norm",
    "vdk_mixup": "tests.test_extent_isolation::test_elementwise_passes",
    "vdk_gemm_f32_nt": "tests.test_extent_isolation::test_gemm_f32",
    "vdk_window_attention_fwd": "tests.test_extent_isolation::test_window_attention",
    "vdk_window_attention_fwd_workspace_bytes": "tests.test_extent_isolation::test_window_attention",
    "vdk_window_attention_fwd_f32": "tests.test_extent_isolation::test_window_attention",
    "vdk_window_attention_bwd_workspace_bytes": "tests.test_extent_isolation::test_window_attention",
    "vdk_window_attention_bwd": "tests.test_extent_isolation::test_window_attention",
    "vdk_relpos_bias_table_grad": "tests.test_extent_isolation::test_relpos_bias_table_grad",
    "vdk_gelu_f32": "tests.test_extent_isolation::test_elementwise_passes",
    "vdk_dgelu_f32": "tests.test_extent_isolation::test_elementwise_passes",
    "vdk_rowscale_f32": "tests.test_extent_isolation::test_elementwise_passes",
    "vdk_colsum_f32_workspace_bytes": "tests.test_extent_isolation::test_reductions",
    "vdk_colsum_f32": "tests.test_extent_isolation::test_reductions",
    "vdk_depth_to_space2_f32": "tests.test_extent_isolation::test_convnext_pieces",
    "vdk_softmax_rows_f32": "tests.test_extent_isolation::test_softmax_rows_f32",
    "vdk_patchify_f32": "tests.test_extent_isolation::test_transposes_patchify_cls",
    "vdk_space_to_depth2_f32": "tests.test_extent_isolation::test_convnext_pieces",
    "vdk_dwconv7_fwd": "tests.test_extent_isolation::test_convnext_pieces",
    "vdk_dwconv7_wgrad_workspace_bytes": "tests.test_extent_isolation::test_convnext_pieces",
    "vdk_dwconv7_wgrad": "tests.test_extent_isolation::test_convnext_pieces",
    "vdk_dwconv7_weight_prep": "tests.test_extent_isolation::test_convnext_pieces",
    "vdk_space_to_depth2_bf16": "tests.test_extent_isolation::test_convnext_pieces",
    "vdk_conv2x2_weight_prep": "tests.test_extent_isolation::test_convnext_pieces",
    "vdk_conv2x2_wgrad_unpermute": "tests.test_extent_isolation::test_convnext_pieces",
    "vdk_layerscale_weight_prep": "tests.test_extent_isolation::test_convnext_pieces",
    "vdk_layerscale_grad": "tests.test_extent_isolation::test_convnext_pieces",
    "vdk_vit_workspace_bytes": "tests.test_workspace_isolation::test_vit_engine_workspace",
    "vdk_vit_fp8_update": "tests.test_workspace_isolation::test_vit_engine_workspace",
    "vdk_vit_refresh_weights": "tests.test_workspace_isolation::test_vit_engine_workspace",
    "vdk_vit_forward": "tests.test_workspace_isolation::test_vit_engine_workspace",
    "vdk_vit_backward": "tests.test_workspace_isolation::test_vit_engine_workspace",
    "vdk_vit_workspace_f32_bytes": "tests.test_workspace_isolation::test_vit_engine_precise_workspace",
    "vdk_vit_forward_f32": "tests.test_workspace_isolation::test_vit_engine_precise_workspace",
    "vdk_conv_weight_prep": "tests.test_extent_isolation::test_resnet_pieces",
    "vdk_conv_wgrad_unpermute": "tests.test_extent_isolation::test_resnet_pieces",
    "vdk_nchw_to_nhwc_bf16": "tests.test_extent_isolation::test_resnet_pieces",
    "vdk_im2col_bf16": "tests.test_extent_isolation::test_resnet_pieces",
    "vdk_bn_rows_workspace_bytes": "tests.test_extent_isolation::test_resnet_pieces",
    "vdk_bn_act_fwd": "tests.test_extent_isolation::test_resnet_pieces",
    "vdk_bn_act_bwd": "tests.test_extent_isolation::test_resnet_pieces",
    "vdk_bn_rows_bwd": "tests.test_extent_isolation::test_resnet_pieces",
    "vdk_maxpool3s2_fwd": "tests.test_extent_isolation::test_resnet_pieces",
    "vdk_maxpool3s2_bwd": "tests.test_extent_isolation::test_resnet_pieces",
    "vdk_avgpool_fwd": "tests.test_extent_isolation::test_resnet_pieces",
    "vdk_avgpool_bwd": "tests.test_extent_isolation::test_resnet_pieces",
    "vdk_avgpool_rows_f32_fwd": "tests.test_extent_isolation::test_convnext_pieces",
    "vdk_avgpool_rows_f32_bwd": "tests.test_extent_isolation::test_convnext_pieces",
    "vdk_scale_dev_f32": "tests.test_extent_isolation::test_elementwise_passes",
    "vdk_preprocess_workspace_bytes": "tests.test_extent_isolation::test_preprocess",
    "vdk_preprocess_resize_pad_normalize": "tests.test_extent_isolation::test_preprocess",
    "vdk_convnext_workspace_bytes": "tests.test_workspace_isolation::test_convnext_engine_workspace",
    "vdk_convnext_refresh_weights": "tests.test_workspace_isolation::test_convnext_engine_workspace",
    "vdk_convnext_forward": "tests.test_workspace_isolation::test_convnext_engine_workspace",
    "vdk_convnext_workspace_f32_bytes": "tests.test_workspace_isolation::test_convnext_engine_f32_workspaces",
    "vdk_convnext_forward_f32": "tests.test_workspace_isolation::test_convnext_engine_f32_workspaces",
    "vdk_convnext_train_f32_workspace_bytes": "tests.test_workspace_isolation::test_convnext_engine_f32_workspaces",
    "vdk_convnext_forward_train_f32": "tests.test_workspace_isolation::test_convnext_engine_f32_workspaces",
    "vdk_convnext_backward_train_f32": "tests.test_workspace_isolation::test_convnext_engine_f32_workspaces",
    "vdk_convnext_backward": "tests.test_workspace_isolation::test_convnext_engine_workspace",
    "vdk_swin_workspace_bytes": "tests.test_workspace_isolation::test_swin_engine_workspace",
    "vdk_swin_refresh_weights": "tests.test_workspace_isolation::test_swin_engine_workspace",
    "vdk_swin_forward": "tests.test_workspace_isolation::test_swin_engine_workspace",
    "vdk_swin_workspace_f32_bytes": "tests.test_workspace_isolation::test_swin_engine_precise_workspace",
    "vdk_swin_forward_f32": "tests.test_workspace_isolation::test_swin_engine_precise_workspace",
    "vdk_swin_backward": "tests.test_workspace_isolation::test_swin_engine_workspace",
    "vdk_resnet_workspace_bytes": "tests.test_workspace_isolation::test_resnet_engine_workspace",
    "vdk_resnet_refresh_weights": "tests.test_workspace_isolation::test_resnet_engine_workspace",
    "vdk_resnet_forward": "tests.test_workspace_isolation::test_resnet_engine_workspace",
    "vdk_resnet_backward": "tests.test_workspace_isolation::test_resnet_engine_workspace",
    "vdk_attn_pool_fwd": "tests.test_extent_isolation::test_attn_pool",
    "vdk_attn_pool_bwd": "tests.test_extent_isolation::test_attn_pool",
    "vdk_attn_pool_fwd_dt": "tests.test_extent_isolation::test_attn_pool",
    "vdk_attn_pool_bwd_dt": "tests.test_extent_isolation::test_attn_pool",
    "vdk_colnorm_fwd": "tests.test_extent_isolation::test_colnorm_rownorm",
    "vdk_colnorm_bwd": "tests.test_extent_isolation::test_colnorm_rownorm",
    "vdk_colnorm_fwd_dt": "tests.test_extent_isolation::test_colnorm_rownorm",
    "vdk_rownorm_fwd_dt": "tests.test_extent_isolation::test_colnorm_rownorm",
    "vdk_rownorm_fwd": "tests.test_extent_isolation::test_colnorm_rownorm",
    "vdk_rownorm_bwd": "tests.test_extent_isolation::test_colnorm_rownorm",
    "vdk_margin_cos_pass": "tests.test_extent_isolation::test_margin_fused_cos_passes",
    "vdk_margin_rowstat": "tests.test_extent_isolation::test_margin_fused_cos_passes",
    "vdk_margin_target_cos_direct": "tests.test_extent_isolation::test_margin_fused_cos_passes",
    "vdk_margin_ce": "tests.test_extent_isolation::test_margin_ce_family",
    "vdk_margin_ce_amp": "tests.test_extent_isolation::test_margin_ce_family",
    "vdk_margin_ce_f32": "tests.test_extent_isolation::test_margin_ce_family",
    "vdk_margin_target_cos": "tests.test_extent_isolation::test_margin_sharded",
    "vdk_margin_stats": "tests.test_extent_isolation::test_margin_sharded",
    "vdk_margin_grad": "tests.test_extent_isolation::test_margin_sharded",
    "vdk_margin_stats_amp": "tests.test_extent_isolation::test_margin_sharded",
    "vdk_margin_grad_amp": "tests.test_extent_isolation::test_margin_sharded",
    "vdk_margin_bwd": "tests.test_extent_isolation::test_margin_ce_family",
}

# ABI name -> why the entry is left out: it takes no pointer to tensor data, or needs more than one process
EXCLUDED = {
    "vdk_last_error": "returns the thread-local message: no tensor operand",
    "vdk_is_device_build": "build query: no operand",
    "vdk_abi_version": "build query: no operand",
    "vdk_gemm_reserve_cus": "sets a grid-size knob: no operand",
    "vdk_gemm_reserved_cus": "reads that knob: no operand",
    "vdk_gemm_a_colsum_rows": "size query of the a_colsum by-product (called to size the guarded buffer): no operand",
    "vdk_gemm_c_colsum_rows": "size query of the c_colsum by-product (called to size the guarded buffer): no operand",
    "vdk_prof_begin": "profiling events: no tensor operand",
    "vdk_prof_pause": "profiling events: no tensor operand",
    "vdk_prof_end": "profiling totals into host scalars: no tensor operand",
    "vdk_prof_bytes": "profiling totals into a host scalar: no tensor operand",
    "vdk_vit_param_count": "layout query into host scalars",
    "vdk_vit_param_info": "layout query into host scalars",
    "vdk_swin_param_count": "layout query into host scalars",
    "vdk_swin_param_info": "layout query into host scalars",
    "vdk_convnext_param_count": "layout query into host scalars",
    "vdk_convnext_param_info": "layout query into host scalars",
    "vdk_resnet_param_count": "layout query into host scalars",
    "vdk_resnet_param_info": "layout query into host scalars",
    "vdk_resnet_ops_format": "sets the calling thread's 16-bit format (test_resnet_pieces runs under both): no operand",
    "vdk_comm_unique_id": "communicator handle (host bytes)",
    "vdk_comm_init": "communicator handle: collective over all ranks",
    "vdk_comm_destroy": "communicator handle",
    "vdk_comm_rank": "communicator handle",
    "vdk_comm_world": "communicator handle",
    "vdk_comm_trace": "communicator timing trace",
    "vdk_comm_trace_close_last": "communicator timing trace",
    "vdk_comm_mark": "communicator timing trace",
    "vdk_comm_trace_read": "communicator timing trace into host arrays",
    "vdk_comm_stream": "communicator handle",
    "vdk_comm_finish": "stream ordering on a communicator handle: no tensor operand",
    "vdk_allreduce_bucket": "needs more than one process",
    "vdk_allgather": "needs more than one process",
}


def _function_bodies(src):
    """top-level function name -> its source text"""
    out = {}
    for part in re.split(r"^(?=def |class |@|[A-Za-z_]\w* = |# ---)", src, flags=re.M):
        m = re.match(r"def (\w+)\(", part)
        if m:
            out[m.group(1)] = part
    return out


def _entries_called(fn, bodies, seen=None):
    """the ABI names `lib.vdk_*` in the body of `fn` and of the module-level helpers (`_name(`) it calls"""
    seen = set() if seen is None else seen
    if fn in seen or fn not in bodies:
        return set()
    seen.add(fn)
    names = set(re.findall(r"lib\.(vdk_\w+)", bodies[fn]))
    for helper in re.findall(r"\b(_\w+)\(", bodies[fn]):
        names |= _entries_called(helper, bodies, seen)
    return names


def test_every_abi_entry_is_covered_or_excluded_with_a_reason():
    """a new entry of include/visiondk.h cannot arrive without a guard-band test, or a written reason for having none; and a COVERED id whose test does not call the entry fails"""
    root = Path(__file__).resolve().parent
    header = (root.parent / "include" / "visiondk.h").read_text()
    names = re.findall(r"^(?:int|const char\*|void\*)\s+(vdk_\w+)\(", header, flags=re.M)
    assert len(names) == len(set(names)) and len(names) >= 171
    assert not set(COVERED) & set(EXCLUDED)
    assert set(COVERED) | set(EXCLUDED) == set(names), (sorted(set(names) - set(COVERED) - set(EXCLUDED)), sorted((set(COVERED) | set(EXCLUDED)) - set(names)))
    assert len(EXCLUDED) <= 40 and all(EXCLUDED.values())
    bodies = {f"tests.{mod}": _function_bodies((root / f"{mod}.py").read_text()) for mod in ("test_extent_isolation", "test_workspace_isolation")}
    for name, tid in COVERED.items():
        mod, fn = tid.split("::")
        assert mod in bodies and fn.startswith("test_") and fn in bodies[mod], (name, tid)
        if mod == "tests.test_extent_isolation" or name.endswith("_bytes"):
            # the kernel-level entries and the size queries are named literally in the test that calls them (or in a helper of this module that the test calls)
            assert name in _entries_called(fn, bodies[mod]), (name, tid)
        else:
            # the engine entries are reached through the wrapper the test drives: vdk_<family>_... belongs to a test of that family's engine
            assert name.split("_")[1] in fn, (name, tid)
