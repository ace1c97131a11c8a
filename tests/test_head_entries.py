"""Every margin-head ABI entry, element by element, on planted cosines (tests/headbound.py), on the CPU SIMT emulation and on the device.

The whole-tensor norms of tests/test_heads.py and tests/test_sharded_head_fp16.py accept a dropped, shifted or duplicated class column (1 / C of a row's probability), and
most of their cases compare one form of csrc/margin_head.hip with another, which cancels an error of the shared margin functions.  Here the input is a float32 cosine
matrix in which every edge column (the ends of a 4096-column pass, of its 1024-column loads, of the scalar tail C & ~3, of a 64-column epilogue slice, of a shard) is the
target of one row and an O(1) hard negative of another, with cosines outside [-1, 1], on both sides of MV-Softmax's threshold, below CircleLoss's -m and an ArcFace target in
the fallback branch; the reference is the float64 restatement of the reference's modules; every entry of dcos is bounded in units of gscale (p + eps / C + (1 - eps) [t]) |jac|
by 4 x the worst entry of a float32 torch evaluation rounded to the case's format, every fp32 output (logits, loss rows, statistics, the fp32 dcos) in units of its
|terms| by 8 x max(the float32 evaluation's worst error, eps32); padding is exactly zero in buffers filled with 7.

Sizes: B = 24; C = 1003 (the narrow kernel), 5003 (one full 4096-column pass, a partial one, a 3-column tail), 6150 (a last pass with two full 1024-column loads, a third
that only thread 0 issues, a 2-column tail)."""
import ctypes as C

import pytest
import torch

from tests import headbound as hb
from visiondk_amd import _abi, heads, ops

B, EPS, GS, LS = 24, 0.1, 0.2, 1024.0
SIZES = (1003, 5003, 6150)
BF, HF = torch.bfloat16, torch.float16
MODE_ID = {"arcface": _abi.HEAD_ARCFACE, "circle": _abi.HEAD_CIRCLE, "mv_am": _abi.HEAD_MV_AM, "mv_arc": _abi.HEAD_MV_ARC}
_CASE = {}


def case(Cn, mode, extra=(), magface=False):
    """planted cosines, the float64 reference and the float32 evaluation: computed once, shared by the entries, formats and backends, never written to"""
    key = (Cn, mode, extra, magface)
    if key not in _CASE:
        h = hb.head(mode, row_margin=torch.linspace(0.45, 0.8, B)) if magface else hb.head(mode)
        pc = hb.planted_cos(B, Cn, mode, 3, extra=extra, h=h)
        ldc = (Cn + 7) // 8 * 8
        buf = torch.full((B, ldc), 3.0)                  # (padding cosines no kernel may read: as cosines they would outweigh every row)
        buf[:, :Cn] = pc.cos
        ref = hb.head_rows(h, pc.cos, pc.labels, EPS, GS)
        o32 = hb.head_rows(h, pc.cos, pc.labels, EPS, GS, dtype=torch.float32)
        _CASE[key] = (pc, buf, ldc, ref, o32)
    return _CASE[key]


def cfg_of(h, be, dev):
    rm = None if h.row_margin is None else h.row_margin.float().to(dev)
    return _abi.MarginHead(MODE_ID[h.mode], h.s, h.m, h.m_am, h.t, be.ptr(rm)), rm


def check_dcos16(got, Cn, ref, o32, dtype, lscale, what):
    """the 16-bit dcos [B, ldd] under the loss scale `lscale`: padding zero, every entry within FACTOR x the rounded float32 evaluation's worst"""
    got = got.cpu()
    assert float(got[:, Cn:].float().abs().sum()) == 0.0, (what, "padding columns")
    orc = (o32.dcos * lscale).to(dtype).double() / lscale
    bnd = hb.bound16(hb.entry_errors(orc, ref.dcos, ref.s_dcos))
    return hb.check("dcos", hb.entry_errors(got[:, :Cn].double() / lscale, ref.dcos, ref.s_dcos), bnd, what=what)


def check32(name, got, want, scale, got32, what):
    """an fp32 output in units of `scale` against LSE_FACTOR x max(the float32 evaluation's worst, eps32)"""
    bnd = hb.bound32(hb.entry_errors(got32, want, scale))
    return hb.check(name, hb.entry_errors(got.cpu(), want, scale), bnd, hb.LSE_FACTOR, what)


def lse_scale(r):
    return r.mx.abs() + torch.log(r.se).abs()


@pytest.mark.parametrize("Cn", SIZES)
@pytest.mark.parametrize("mode", hb.MODES)
def test_margin_ce_with_logits_and_margin_bwd(be, dev, mode, Cn):
    """vdk_margin_ce writing logits, loss rows and dcos (the narrow kernel at every C), and vdk_margin_bwd on a dlogits of mixed sign and magnitude"""
    pc, buf, ldc, ref, o32 = case(Cn, mode)
    cfg, _ = cfg_of(pc.h, be, dev)
    cos, lab = buf.to(dev), pc.labels.to(dev)
    logits = torch.full((B, ldc), 7.0, device=dev)
    loss = torch.full((B,), 7.0, device=dev)
    dcos = torch.full((B, ldc), 7.0, dtype=BF, device=dev)
    be.check(be.lib.vdk_margin_ce(C.byref(cfg), be.ptr(cos), ldc, B, Cn, be.ptr(lab), EPS, GS, be.ptr(logits), ldc, be.ptr(loss), be.ptr(dcos), ldc, be.stream()), "vdk_margin_ce")
    what = f"margin_ce {mode} C{Cn}"
    assert bool((logits[:, Cn:] == 7.0).all())                       # the logits have no padding to zero: nothing beyond C is written
    check32("logits", logits[:, :Cn], ref.logit, ref.labs, o32.logit, what)
    check32("loss", loss, ref.loss, ref.s_loss, o32.loss, what)
    check_dcos16(dcos, Cn, ref, o32, BF, 1.0, what)
    g = torch.Generator().manual_seed(4)
    dl = torch.randn(B, Cn, generator=g) * torch.exp(3.0 * torch.randn(B, Cn, generator=g))
    dcos = torch.full((B, ldc), 7.0, dtype=BF, device=dev)
    dld = dl.to(dev)
    be.check(be.lib.vdk_margin_bwd(C.byref(cfg), be.ptr(cos), ldc, B, Cn, be.ptr(lab), be.ptr(dld), Cn, be.ptr(dcos), ldc, be.stream()), "vdk_margin_bwd")
    got = dcos.cpu()
    assert float(got[:, Cn:].float().abs().sum()) == 0.0
    want, scale = dl.double() * ref.jac, dl.double().abs() * ref.jac.abs()
    bnd = hb.bound16(hb.entry_errors((dl * o32.jac).to(BF), want, scale))
    hb.check("dcos", hb.entry_errors(got[:, :Cn], want, scale), bnd, what=f"margin_bwd {mode} C{Cn}")


def _ce_amp(be, dev, pc, buf, ldc, Cn, dtype, lscale, cfg):
    cos, lab = buf.to(dev), pc.labels.to(dev)
    loss = torch.full((B,), 7.0, device=dev)
    dcos = torch.full((B, ldc), 7.0, dtype=dtype, device=dev)
    ls = None if lscale is None else torch.tensor([lscale, 0.0, 0.0], device=dev)
    be.check(be.lib.vdk_margin_ce_amp(C.byref(cfg), be.ptr(cos), ldc, B, Cn, be.ptr(lab), EPS, GS, be.ptr(ls), None, 0, be.ptr(loss), be.ptr(dcos), ldc,
                                      _abi.F16_ if dtype == HF else _abi.BF16, be.stream()), "vdk_margin_ce_amp")
    return loss, dcos


@pytest.mark.parametrize("dtype", [BF, HF])
@pytest.mark.parametrize("Cn", SIZES)
@pytest.mark.parametrize("mode", hb.MODES + ("arcface_generic",))
def test_margin_ce_amp(be, dev, mode, Cn, dtype, monkeypatch):
    """vdk_margin_ce_amp without logits -- the vector kernel from C = 4096 on, ArcFace in its once-per-row form and (VDK_MARGIN_GENERIC=1) in the generic one -- with
    bf16 and fp16 dcos, without and with a device loss scale (1024: dcos comes back scaled, the loss rows do not)"""
    monkeypatch.setenv("VDK_MARGIN_GENERIC", "1" if mode == "arcface_generic" else "0")
    pc, buf, ldc, ref, o32 = case(Cn, mode.split("_generic")[0])
    cfg, _ = cfg_of(pc.h, be, dev)
    for lscale in (None, LS):
        what = f"margin_ce_amp {mode} C{Cn} {dtype} scale {lscale}"
        loss, dcos = _ce_amp(be, dev, pc, buf, ldc, Cn, dtype, lscale, cfg)
        check32("loss", loss, ref.loss, ref.s_loss, o32.loss, what)
        check_dcos16(dcos, Cn, ref, o32, dtype, lscale or 1.0, what)


@pytest.mark.parametrize("dtype", [BF, HF])
@pytest.mark.parametrize("Cn", SIZES)
def test_margin_ce_amp_with_per_row_margins(be, dev, Cn, dtype):
    """the MagFace path: ArcFace with a margin per row (0.45 .. 0.8), which takes the generic instantiation; one target below every row's cos(pi - m)"""
    pc, buf, ldc, ref, o32 = case(Cn, "arcface", magface=True)
    cfg, keep = cfg_of(pc.h, be, dev)
    what = f"margin_ce_amp row margins C{Cn} {dtype}"
    loss, dcos = _ce_amp(be, dev, pc, buf, ldc, Cn, dtype, LS, cfg)
    check32("loss", loss, ref.loss, ref.s_loss, o32.loss, what)
    check_dcos16(dcos, Cn, ref, o32, dtype, LS, what)


@pytest.mark.parametrize("Cn", SIZES[:2])
@pytest.mark.parametrize("mode", hb.MODES)
def test_margin_ce_f32(be, dev, mode, Cn):
    """vdk_margin_ce_f32: the fp32 dcos of the fp32-class training mode, every entry against the float32 evaluation's own error"""
    pc, buf, ldc, ref, o32 = case(Cn, mode)
    cfg, _ = cfg_of(pc.h, be, dev)
    cos, lab = buf.to(dev), pc.labels.to(dev)
    loss = torch.full((B,), 7.0, device=dev)
    dcos = torch.full((B, ldc), 7.0, device=dev)
    be.check(be.lib.vdk_margin_ce_f32(C.byref(cfg), be.ptr(cos), ldc, B, Cn, be.ptr(lab), EPS, GS, be.ptr(loss), be.ptr(dcos), ldc, be.stream()), "vdk_margin_ce_f32")
    what = f"margin_ce_f32 {mode} C{Cn}"
    assert float(dcos[:, Cn:].abs().sum()) == 0.0
    check32("loss", loss, ref.loss, ref.s_loss, o32.loss, what)
    check32("dcos32", dcos[:, :Cn], ref.dcos, ref.s_dcos, o32.dcos, what)


@pytest.mark.parametrize("split", [2504, 2501])
@pytest.mark.parametrize("mode,form", [(m, f) for m in hb.MODES for f in ("old", "bf16", "fp16")] + [("arcface", "fp16_generic")])
def test_sharded_chain_against_the_whole_row(be, dev, mode, form, split, monkeypatch):
    """vdk_margin_target_cos -> vdk_margin_stats(_amp) -> the host merge of heads.sharded_margin_ce -> vdk_margin_grad(_amp) over the column blocks [0, split) and
    [split, 5003) of one planted matrix (2504: the second block 16-byte aligned, the vector path at c_base != 0; 2501: the scalar path); targets on both sides of the split,
    on the first block's last and the second's first column.  The merged statistics, the loss and the concatenated dcos against float64 of the WHOLE row (C_total = 5003 in
    the smoothing term); form: the old passes (bf16, no loss scale) | the _amp passes with bf16 / fp16 dcos under a loss scale (ArcFace once per row | generic)."""
    Cn = 5003
    monkeypatch.setenv("VDK_MARGIN_GENERIC", "1" if form == "fp16_generic" else "0")
    pc, buf, ldc, ref, o32 = case(Cn, mode, extra=(split,))
    assert {split - 1, split, split + 1} <= set(pc.labels.tolist())
    cfg, _ = cfg_of(pc.h, be, dev)
    cos, lab = buf.to(dev), pc.labels.to(dev)
    amp = form != "old"
    dtype = HF if form.startswith("fp16") else BF
    lscale = LS if amp else 1.0
    ls = torch.tensor([LS, 0.0, 0.0], device=dev)
    blocks = [(0, split), (split, Cn - split)]
    gt = torch.zeros(B, device=dev)
    for c0, cl in blocks:
        g = torch.full((B,), 7.0, device=dev)
        be.check(be.lib.vdk_margin_target_cos(cos.data_ptr() + 4 * c0, ldc, B, cl, c0, be.ptr(lab), be.ptr(g), be.stream()), "vdk_margin_target_cos")
        gt += g
    assert torch.equal(gt.cpu(), pc.cos[torch.arange(B), pc.labels])              # one shard owns the column, the others add 0
    parts = []
    for c0, cl in blocks:
        st = torch.full((B, 4), 7.0, device=dev)
        fn = be.lib.vdk_margin_stats_amp if amp else be.lib.vdk_margin_stats
        be.check(fn(C.byref(cfg), cos.data_ptr() + 4 * c0, ldc, B, cl, c0, be.ptr(lab), be.ptr(gt), be.ptr(st), be.stream()), "vdk_margin_stats")
        parts.append(st)
    gmax = torch.stack([p[:, 0] for p in parts]).max(0).values.contiguous()
    sums = sum(torch.stack([p[:, 1] * torch.exp(p[:, 0] - gmax), p[:, 2], p[:, 3]], 1) for p in parts)
    gsum = sums[:, 0].contiguous()
    loss = gmax + torch.log(gsum) - (1.0 - EPS) * sums[:, 2] - EPS * sums[:, 1] / Cn
    what = f"sharded {mode} {form} split {split}"
    rows = torch.arange(B)
    at = ref.logit.argmax(1)
    check32("max", gmax, ref.mx, ref.labs[rows, at], o32.logit[rows, at], what)      # the max IS one logit: that logit's bound
    check32("lse", gmax + torch.log(gsum), ref.lse, lse_scale(ref), o32.lse, what)
    check32("sum logit", sums[:, 1], ref.sm, ref.labs.sum(1), o32.sm, what)
    check32("target logit", sums[:, 2], ref.lt, ref.labs[rows, pc.labels], o32.lt, what)
    check32("loss", loss, ref.loss, ref.s_loss, o32.loss, what)
    ds = []
    for c0, cl in blocks:
        ldd = (cl + 7) // 8 * 8
        d = torch.full((B, ldd), 7.0, dtype=dtype, device=dev)
        if amp:
            be.check(be.lib.vdk_margin_grad_amp(C.byref(cfg), cos.data_ptr() + 4 * c0, ldc, B, cl, c0, Cn, be.ptr(lab), be.ptr(gt), be.ptr(gmax), be.ptr(gsum), EPS, GS,
                                                be.ptr(ls), be.ptr(d), ldd, _abi.F16_ if dtype == HF else _abi.BF16, be.stream()), "vdk_margin_grad_amp")
        else:
            be.check(be.lib.vdk_margin_grad(C.byref(cfg), cos.data_ptr() + 4 * c0, ldc, B, cl, c0, Cn, be.ptr(lab), be.ptr(gt), be.ptr(gmax), be.ptr(gsum), EPS, GS,
                                            be.ptr(d), ldd, be.stream()), "vdk_margin_grad")
        assert float(d[:, cl:].float().abs().sum()) == 0.0, (what, "padding columns of block", c0)
        ds.append(d[:, :cl])
    check_dcos16(torch.cat(ds, 1), Cn, ref, o32, dtype, lscale, what)


@pytest.mark.parametrize("kern", [2, 5])
@pytest.mark.parametrize("mode", hb.MODES)
def test_epilogue_fused_passes(be, dev, mode, kern):
    """vdk_margin_cos_pass 1 -> vdk_margin_rowstat -> pass 2 on the eight-wave and on the four-wave 256x256 TN kernel: C = 1003, B = 70 (a ragged second row group, a
    ragged last 64-column slice), three bf16 planes of a planted head.  The cosines never leave the epilogue, so the reference is float64 of the head on the cosines the
    materialised GEMM gives over the same planes with the same kernel forced; the two GEMM routes' cosines (forced kernel | default routing) differ by fp32 summation
    order only -- asserted <= 2e-6 -- and no cosine lies within GUARD + that difference of a branch threshold, so the branch each entry takes does not depend on it."""
    D, Cn, Bn = 128, 1003, 70
    ph = hb.planted_head(D, Cn, mode, 6, B=Bn)
    cfg, _ = cfg_of(ph.h, be, dev)
    feats, w, lab = ph.feats.to(dev), ph.weight.to(dev), ph.labels.to(dev)
    st = heads._forward_cos(be, feats, w, 3)
    cos_default = st.cos[:Bn, :Cn].cpu()
    K = st.fbt.shape[0]
    nslice = (st.Cp + 63) // 64
    stats = torch.full((Bn, nslice, 4), 7.0, device=dev)
    tlogit = torch.zeros(Bn, device=dev)
    gt = None
    if mode in ("mv_am", "mv_arc"):
        gt = torch.full((Bn,), 7.0, device=dev)
        be.check(be.lib.vdk_margin_target_cos_direct(be.ptr(st.fbt), st.Bp, be.ptr(st.wb), st.Cp, K, Bn, be.ptr(lab), be.ptr(gt), be.stream()), "vdk_margin_target_cos_direct")
    rowstat = torch.full((Bn, 2), 7.0, device=dev)
    loss = torch.full((Bn,), 7.0, device=dev)
    dcos = torch.full((st.Bp, st.Cp), 7.0, dtype=BF, device=dev)
    be.lib.vdk_gemm_force_kernel(kern)
    try:
        cos_k = ops.gemm_nt(st.fbt, st.wb, out_dtype=torch.float32, trans=True, backend=be)[:Bn, :Cn].cpu()
        be.check(be.lib.vdk_margin_cos_pass(C.byref(cfg), 1, be.ptr(st.fbt), st.Bp, be.ptr(st.wb), st.Cp, Bn, st.Bp, Cn, st.Cp, K, be.ptr(lab), be.ptr(gt), be.ptr(stats),
                                            be.ptr(tlogit), None, EPS, GS, None, 0, be.stream()), "vdk_margin_cos_pass 1")
        be.check(be.lib.vdk_margin_rowstat(be.ptr(stats), nslice, be.ptr(tlogit), Bn, Cn, EPS, be.ptr(rowstat), be.ptr(loss), be.stream()), "vdk_margin_rowstat")
        be.check(be.lib.vdk_margin_cos_pass(C.byref(cfg), 2, be.ptr(st.fbt), st.Bp, be.ptr(st.wb), st.Cp, Bn, st.Bp, Cn, st.Cp, K, be.ptr(lab), be.ptr(gt), None, None,
                                            be.ptr(rowstat), EPS, GS, be.ptr(dcos), st.Cp, be.stream()), "vdk_margin_cos_pass 2")
    finally:
        be.lib.vdk_gemm_force_kernel(0)
    diff = float((cos_k.double() - cos_default.double()).abs().max())
    print(f"head fused {mode} kernel {kern}: the two GEMM routes' cosines differ by {diff:.2e}")
    assert diff <= 2e-6                                   # K = 384 products of |f^ w^| <= 1 summed in another order: a few ulps of 1
    if gt is not None:
        # MV-Softmax: the row's threshold and the target's logit come from gt, an INPUT of both passes (the target entry's own cosine is not looked at): the reference
        # takes the same number, which is the GEMM's own up to summation order
        assert float((gt.cpu() - cos_k[torch.arange(Bn), ph.labels]).abs().max()) <= 2e-6
        cos_k[torch.arange(Bn), ph.labels] = gt.cpu()
    hb.assert_guard(ph.h, cos_k, ph.labels, band=hb.GUARD + diff)
    ref = hb.head_rows(ph.h, cos_k, ph.labels, EPS, GS)
    o32 = hb.head_rows(ph.h, cos_k, ph.labels, EPS, GS, dtype=torch.float32)
    what = f"fused {mode} kernel {kern}"
    rows = torch.arange(Bn)
    at = ref.logit.argmax(1)
    rs = rowstat.cpu().double()
    check32("max", rs[:, 0], ref.mx, ref.labs[rows, at], o32.logit[rows, at], what)
    check32("lse", rs[:, 0] - torch.log(rs[:, 1]), ref.lse, lse_scale(ref), o32.lse, what)
    check32("loss", loss, ref.loss, ref.s_loss, o32.loss, what)
    got = dcos.cpu()
    assert float(got[Bn:].float().abs().sum()) == 0.0, (what, "padding rows")
    check_dcos16(got[:Bn], Cn, ref, o32, BF, 1.0, what)
