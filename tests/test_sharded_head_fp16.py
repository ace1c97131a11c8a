"""The class-sharded margin head on fp16 (and bf16) operands under a loss scale: `heads.sharded_margin_ce(..., cos_planes, operand, loss_scale)` and its two passes
vdk_margin_stats_amp / vdk_margin_grad_amp, on the CPU emulation and -- through the same C ABI -- on the gfx950 library.  Without a process group the function is one
shard holding every class; the in-process two-shard tests call the passes on column blocks of one cosine matrix.  The two-rank forms are in
tests/test_sharded_head_fp16_gloo.py (emulation) and tests/test_sharded_head_fp16_gpu.py (MI355X)."""
import ctypes as C

import pytest
import torch

from visiondk_amd import _abi, heads

D, CN, B = 64, 5003, 5
LABELS = [0, 5002, 77, 4096, 2500]


def _rel(a, b):
    a = torch.as_tensor(a).double().cpu(); b = torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _head(tag, be, dev, **kw):
    if tag == "arcface":
        return heads.ArcFace(D, CN, backend=be, device=dev, **kw)
    if tag == "circle":
        return heads.CircleLoss(D, CN, margin=0.25, gamma=64, backend=be, device=dev)
    return heads.MV_Softmax(D, CN, is_am=(tag == "mv_am"), backend=be, device=dev)


def _scale(v, dev):
    return torch.tensor([v, 0.0, 0.0], dtype=torch.float32, device=dev)


@pytest.mark.parametrize("planes", [1, 3])
@pytest.mark.parametrize("operand", ["bf16", "fp16"])
@pytest.mark.parametrize("tag", ["arcface", "circle", "mv_am"])
def test_one_shard_under_a_loss_scale_equals_the_fused_form(be, dev, tag, operand, planes):
    """one shard holding every class = the fused `margin_ce` on the same operands under the same loss scale (the shape and bounds of
    test_heads.py::test_sharded_form_with_one_shard_equals_fused_form: both sides round the same operands once).  The loss rows do not depend on the scale; with bf16 the
    gradients at scale 1024 divided by 1024 ARE the gradients at scale 1 (a power of two is exact in a format with fp32's exponent range)."""
    torch.manual_seed(5)
    h = _head(tag, be, dev)
    feats = torch.randn(B, D, device=dev)
    labels = torch.tensor(LABELS, device=dev)
    ls = _scale(1024.0, dev)
    l1, df1, dW1 = h.margin_ce(feats, labels, label_smoothing=0.1, operand=operand, loss_scale=ls, cos_planes=planes)
    l2, df2, dW2 = heads.sharded_margin_ce(h, feats, labels, h.weight.detach(), 0, CN, label_smoothing=0.1, operand=operand, loss_scale=ls, cos_planes=planes)
    res = (_rel(l2, l1), _rel(df2, df1), _rel(dW2, dW1))
    print(tag, operand, planes, res)
    assert res[0] < 1e-6 and res[1] < 1e-3 and res[2] < 1e-3, res
    l3, df3, dW3 = heads.sharded_margin_ce(h, feats, labels, h.weight.detach(), 0, CN, label_smoothing=0.1, operand=operand, loss_scale=_scale(1.0, dev),
                                           cos_planes=planes)
    assert torch.equal(l3, l2)                                   # the loss is never scaled
    assert torch.isfinite(df2).all() and torch.isfinite(dW2).all()
    if operand == "bf16":
        assert torch.equal(df2 / 1024.0, df3) and torch.equal(dW2 / 1024.0, dW3)
    else:                                                       # (fp16 rounds differently near its subnormals: the scale is there to lift the gradient out of them)
        assert _rel(df2 / 1024.0, df3) < 1e-3 and _rel(dW2 / 1024.0, dW3) < 1e-3


def _passes(be, h, cos, ldc, col0, cloc, c_base, labels, gt, ctot, dtype, ls, gmax=None, gsum=None, smoothing=0.1, gs=0.2):
    """vdk_margin_stats_amp (and, given the global max / sum, vdk_margin_grad_amp) on the column block [col0, col0 + cloc) of the fp32 cosine matrix `cos` [rows, ldc];
    the block's dcos gets a buffer of its own, padded to a multiple of 8 columns (the kernel zeroes the padding)"""
    nb = labels.shape[0]
    dev = cos.device
    cptr = cos.data_ptr() + 4 * col0
    stats = torch.empty((nb, 4), dtype=torch.float32, device=dev)
    be.check(be.lib.vdk_margin_stats_amp(C.byref(h.cfg), cptr, ldc, nb, cloc, c_base, be.ptr(labels), be.ptr(gt), be.ptr(stats), be.stream()), "vdk_margin_stats_amp")
    if gmax is None:
        return stats, None
    ldd = (cloc + 7) // 8 * 8
    dcos = torch.full((nb, ldd), 7.0, dtype=dtype, device=dev)      # (a non-zero fill: the padding columns must come back zeroed)
    be.check(be.lib.vdk_margin_grad_amp(C.byref(h.cfg), cptr, ldc, nb, cloc, c_base, ctot, be.ptr(labels), be.ptr(gt), be.ptr(gmax), be.ptr(gsum), smoothing, gs,
                                        be.ptr(ls), be.ptr(dcos), ldd, _abi.F16_ if dtype == torch.float16 else _abi.BF16, be.stream()), "vdk_margin_grad_amp")
    return stats, dcos


def _merge(parts):
    """the host-side merge of `sharded_margin_ce`: MAX of the maxima, the exp-sums rescaled to it, SUM of the logit sums and of the target logits"""
    gmax = torch.stack([p[:, 0] for p in parts]).max(0).values.contiguous()
    sums = sum(torch.stack([p[:, 1] * torch.exp(p[:, 0] - gmax), p[:, 2], p[:, 3]], 1) for p in parts)
    return gmax, sums


def _target_cos(be, cos, ldc, cloc, labels):
    gt = torch.empty(labels.shape[0], dtype=torch.float32, device=cos.device)
    be.check(be.lib.vdk_margin_target_cos(be.ptr(cos), ldc, labels.shape[0], cloc, 0, be.ptr(labels), be.ptr(gt), be.stream()), "vdk_margin_target_cos")
    return gt


@pytest.mark.parametrize("split", [2504, 2501])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("tag", ["arcface", "circle", "mv_am", "mv_arc"])
def test_two_column_blocks_in_one_process_equal_one_block(be, dev, tag, dtype, split):
    """the new passes on the column blocks [0, split) and [split, 5003) of ONE cosine matrix (c_base = split for the second: a target outside the shard on both sides, one
    row whose target is the second block's first column, the padded tail) against the whole matrix as one block.  Statistics merged as `sharded_margin_ce` merges them:
    max and target logit exactly, the two sums to the order of an fp32 sum.  Gradient from the SAME gt / max / sum: bit for bit, the same expressions on the same inputs.
    split = 2504 keeps the second block 16-byte aligned (the vector path at c_base != 0); 2501 starts it unaligned (the scalar path)."""
    torch.manual_seed(5)
    h = _head(tag, be, dev)
    feats = torch.randn(B + 1, D, device=dev)
    labels = torch.tensor(LABELS + [split], device=dev)
    nb = B + 1
    st = heads._forward_cos(be, feats, h.weight.detach(), 1, dtype=dtype)
    gt = _target_cos(be, st.cos, st.Cp, CN, labels)
    ls = _scale(1024.0, dev)
    one, _ = _passes(be, h, st.cos, st.Cp, 0, CN, 0, labels, gt, CN, dtype, ls)
    gmax1, sums1 = _merge([one])
    gsum1 = sums1[:, 0].contiguous()
    _, d_one = _passes(be, h, st.cos, st.Cp, 0, CN, 0, labels, gt, CN, dtype, ls, gmax1, gsum1)
    a, d_a = _passes(be, h, st.cos, st.Cp, 0, split, 0, labels, gt, CN, dtype, ls, gmax1, gsum1)
    b, d_b = _passes(be, h, st.cos, st.Cp, split, CN - split, split, labels, gt, CN, dtype, ls, gmax1, gsum1)
    gmax2, sums2 = _merge([a, b])
    assert torch.equal(gmax2, gmax1) and torch.equal(sums2[:, 2], sums1[:, 2])            # max and target logit: exact
    assert torch.equal(a[:, 3] != 0, labels < split) and torch.equal(b[:, 3] != 0, labels >= split)      # the target logit comes from the shard that owns the column
    r = (_rel(sums2[:, 0], sums1[:, 0]), _rel(sums2[:, 1], sums1[:, 1]))
    print(tag, dtype, split, r)
    assert r[0] < 1e-6 and r[1] < 1e-6, r
    assert torch.equal(torch.cat([d_a[:, :split], d_b[:, :CN - split]], 1).view(torch.int16), d_one[:, :CN].view(torch.int16))
    for d, n in ((d_one, CN), (d_a, split), (d_b, CN - split)):
        assert float(d[:, n:].float().abs().sum()) == 0.0 and torch.isfinite(d.float()).all()
    assert float(d_one[:nb, :CN].float().abs().max()) > 0.0


@pytest.mark.parametrize("operand", ["bf16", "fp16"])
def test_sharded_arcface_fast_path_equals_the_generic_evaluation(be, dev, operand, monkeypatch):
    """plain ArcFace through the new passes evaluates the margin once per row; VDK_MARGIN_GENERIC=1 runs the per-entry evaluation: the same expressions, so statistics,
    loss rows and both gradients are bit-identical.  The planted cases of test_heads.py::test_arcface_fast_path_equals_the_generic_evaluation (a target beyond
    cos(pi - m), cosines pushed outside [-1, 1], margin_am = 0.1), as one shard and with the shard boundary at column 2504 so that the planted target (column 5) lies
    outside the second shard."""
    torch.manual_seed(7)
    nb = 6
    h = heads.ArcFace(D, CN, margin_arc=0.35, margin_am=0.1, scale=32, backend=be, device=dev)
    feats = torch.randn(nb, D, device=dev)
    with torch.no_grad():
        h.weight[:, 5] = -feats[1] * 3.0            # target of row 1 nearly opposite: cos < cos(pi - m)
    labels = torch.tensor([0, 5, 1234, 4096, 17, 4999], device=dev)
    dtype = torch.float16 if operand == "fp16" else torch.bfloat16
    ls = _scale(1024.0, dev)
    st = heads._forward_cos(be, feats, h.weight.detach(), 3, dtype=dtype)
    with torch.no_grad():
        st.cos[2, 100] = 1.0 + 3e-7; st.cos[3, 3000] = -1.0 - 3e-7; st.cos[4, 2504] = 1.0 + 3e-7      # outside the clamp's range: zero jacobian, in both shards
    gt = _target_cos(be, st.cos, st.Cp, CN, labels)
    split = 2504
    outs = []
    for generic in ("0", "1"):
        monkeypatch.setenv("VDK_MARGIN_GENERIC", generic)
        full = heads.sharded_margin_ce(h, feats, labels, h.weight.detach(), 0, CN, label_smoothing=0.1, operand=operand, loss_scale=ls)
        one, _ = _passes(be, h, st.cos, st.Cp, 0, CN, 0, labels, gt, CN, dtype, ls)
        gmax, sums = _merge([one])
        gsum = sums[:, 0].contiguous()
        a, d_a = _passes(be, h, st.cos, st.Cp, 0, split, 0, labels, gt, CN, dtype, ls, gmax, gsum)
        b, d_b = _passes(be, h, st.cos, st.Cp, split, CN - split, split, labels, gt, CN, dtype, ls, gmax, gsum)
        outs.append(list(full) + [one, a, b, d_a.view(torch.int16), d_b.view(torch.int16)])
    assert outs[0][4][1, 3] != 0 and outs[0][5][1, 3] == 0      # row 1's target logit: the first shard's
    for x, y in zip(*outs):
        assert torch.equal(x, y)


def test_defaults_still_run_the_old_passes(be, dev):
    """`sharded_margin_ce` without the new arguments returns, bit for bit, what vdk_margin_target_cos / vdk_margin_stats / vdk_margin_grad give when called by hand in the
    sequence the function has always run (three bf16 planes, no loss scale)"""
    torch.manual_seed(5)
    h = _head("arcface", be, dev)
    feats = torch.randn(B, D, device=dev)
    labels = torch.tensor(LABELS, device=dev)
    got = heads.sharded_margin_ce(h, feats, labels, h.weight.detach(), 0, CN, label_smoothing=0.1)
    w = h.weight.detach()
    st = heads._forward_cos(be, feats, w)
    gt = _target_cos(be, st.cos, st.Cp, CN, labels)
    stats = torch.empty((B, 4), dtype=torch.float32, device=dev)
    be.check(be.lib.vdk_margin_stats(C.byref(h.cfg), be.ptr(st.cos), st.Cp, B, CN, 0, be.ptr(labels), be.ptr(gt), be.ptr(stats), be.stream()), "vdk_margin_stats")
    gmax = stats[:, 0].contiguous()
    sums = torch.stack([stats[:, 1] * torch.exp(stats[:, 0] - gmax), stats[:, 2], stats[:, 3]], 1).contiguous()
    gsum = sums[:, 0].contiguous()
    loss = gmax + torch.log(gsum) - (1.0 - 0.1) * sums[:, 2] - 0.1 * sums[:, 1] / CN
    dcos = torch.zeros((st.Bp, st.Cp), dtype=torch.bfloat16, device=dev)
    be.check(be.lib.vdk_margin_grad(C.byref(h.cfg), be.ptr(st.cos), st.Cp, B, CN, 0, CN, be.ptr(labels), be.ptr(gt), be.ptr(gmax), be.ptr(gsum), 0.1, 1.0 / B,
                                    be.ptr(dcos), st.Cp, be.stream()), "vdk_margin_grad")
    df, dW = heads._backward_from_dcos(be, st, w, dcos)
    assert torch.equal(got[0], loss) and torch.equal(got[1], df) and torch.equal(got[2], dW)


def test_fp16_gradient_overflows_under_a_huge_scale_and_the_loss_does_not(be, dev):
    """loss scale 2^40: d(loss)/d(cos) leaves fp16's range, so dW holds a non-finite value (what the optimizer pass detects to skip the step); the loss rows, never
    scaled, stay finite"""
    torch.manual_seed(5)
    h = _head("arcface", be, dev)
    feats = torch.randn(B, D, device=dev)
    labels = torch.tensor(LABELS, device=dev)
    loss, df, dW = heads.sharded_margin_ce(h, feats, labels, h.weight.detach(), 0, CN, label_smoothing=0.1, operand="fp16", loss_scale=_scale(2.0 ** 40, dev), cos_planes=1)
    assert not torch.isfinite(dW).all()
    assert torch.isfinite(loss).all()


def test_sharded_form_refuses_an_unknown_operand(emu):
    h = _head("arcface", emu, "cpu")
    with pytest.raises(ValueError):
        heads.sharded_margin_ce(h, torch.randn(B, D), torch.tensor(LABELS), h.weight.detach(), 0, CN, operand="fp8")
