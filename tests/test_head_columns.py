"""The margin heads end to end, every dW column and every dfeats row bounded, on planted heads (tests/headbound.py), on the CPU SIMT emulation and on the device.

tests/test_heads.py compares dfeats and dweight by a whole-tensor norm on Gaussian features, where one class column is 1 / sqrt(C) of |dW|.  Here column y_k of the weight
has cosine c_t with feature row k (its target) and c_n with row k - 1 (its hard negative), target and hard negative each hold 10 .. 90 % of their row, and y_k runs over
the edge columns of the kernels (headbound.edges); the reference is float64 of the reference's modules, the unit of a column's (row's) error the same products with every
factor in absolute value carried through both normalisations, the bound 4 x the worst column (row) of a float32 torch evaluation that rounds f^, W^ and dcos to the case's
16-bit format.  Before a kernel result is looked at, each case asserts from float64 alone that "column j's dW misses its planted row", "row b's dfeats ignores its planted
column" and "an ordinary column comes back zero" would each exceed 3 x the bound, for every pair and every column.

D = 128; C = 5003 (1003 where the epilogue-fused form is forced); B = the edges plus four fillers, 70 in the ArcFace cases (a second 64-row group and Bp padding)."""
import ctypes as C

import pytest
import torch

from tests import headbound as hb
from visiondk_amd import _abi, heads

D, EPS, LS = 128, 0.1, 1024.0
BF, HF = torch.bfloat16, torch.float16
_CASE = {}


def make(mode, Cn, be, dev, mag=False):
    if mag:
        return heads.MagFace(D, Cn, backend=be, device=dev)
    h = hb.head(mode)
    if mode == "arcface":
        return heads.ArcFace(D, Cn, margin_arc=h.m, margin_am=h.m_am, scale=h.s, backend=be, device=dev)
    if mode == "circle":
        return heads.CircleLoss(D, Cn, margin=h.m, gamma=h.s, backend=be, device=dev)
    return heads.MV_Softmax(D, Cn, is_am=(mode == "mv_am"), margin=h.m, mv_weight=h.t, scale=h.s, backend=be, device=dev)


def case(mode, Cn=5003, fmt=BF, planes=3, lscale=1.0, extra=(), mag=False, eps=EPS):
    """inputs, float64 reference, oracle bounds: computed once per case and shared by the forms and backends; the preconditions are asserted here, before any kernel runs.
    fmt None: the fp32-class form -- the oracle is float32 torch without any 16-bit rounding"""
    key = (mode, Cn, fmt, planes, lscale, extra, mag, eps)
    if key not in _CASE:
        n = len(hb.edges(Cn, extra))
        Bn = 70 if mode == "arcface" and not mag else n + 4
        hp = hb.head("arcface", m_am=0.0) if mag else hb.head(mode)
        if mag:
            # margins 0.45 .. 0.5025 from feature norms 5 .. 25 (below l_a and inside; above u_a is in the golden fixture): targets at cosine 0.85 and the negative placed
            # for the middle margin keep both between 10 and 90 % of every row
            ph = hb.planted_head(D, Cn, mode, 8, B=Bn, extra=extra, h=hb.head("arcface", m=0.476, m_am=0.0), fnorm=(5.0, 25.0), c_t=0.85)
        else:
            ph = hb.planted_head(D, Cn, mode, 8, B=Bn, extra=extra, h=hp)
        cf = fmt if planes == 1 else None
        kw = dict(eps=eps, cos_fmt=cf, mag=hb.MAG if mag else None)
        ref = hb.head_e2e(hp, ph.feats, ph.weight, ph.labels, **kw)
        orc = hb.head_e2e(hp, ph.feats, ph.weight, ph.labels, dtype=torch.float32, fmt=fmt, lscale=lscale, **kw)
        bnd = hb.e2e_bounds(ref, orc)
        what = f"{'magface' if mag else mode} C{Cn} B{Bn} {fmt} planes {planes}"
        hb.assert_shares(ref, ph.pairs)
        hb.assert_sensitive(ref, ph.pairs, bnd, what)
        _CASE[key] = (ph, ref, bnd, what)
    return _CASE[key]


def check(df, dW, cs, form, scale=1.0):
    ph, ref, bnd, what = cs
    e = hb.e2e_errors(df.cpu().double() / scale, dW.cpu().double() / scale, ref)
    return [hb.check(kind, e[kind], bnd[kind], what=f"{form}: {what}") for kind in ("dfeats", "dweight")]


def load(h, ph, dev):
    with torch.no_grad():
        h.weight.copy_(ph.weight.to(dev))
    return ph.feats.to(dev), ph.labels.to(dev)


@pytest.mark.parametrize("planes", [3, 1])
@pytest.mark.parametrize("mode", hb.MODES)
def test_margin_ce(be, dev, mode, planes):
    """margin_ce in its default form (three planes) and with single-plane cosines"""
    cs = case(mode, planes=planes)
    h = make(mode, 5003, be, dev)
    feats, labels = load(h, cs[0], dev)
    _, df, dW = h.margin_ce(feats, labels, label_smoothing=EPS, cos_planes=planes)
    check(df, dW, cs, "margin_ce")


@pytest.mark.parametrize("planes", [3, 1])
@pytest.mark.parametrize("mode", hb.MODES)
def test_margin_ce_fp16_under_a_loss_scale(be, dev, mode, planes):
    """operand="fp16" with a device loss scale: the gradients come back scaled"""
    cs = case(mode, fmt=HF, planes=planes, lscale=LS)
    h = make(mode, 5003, be, dev)
    feats, labels = load(h, cs[0], dev)
    ls = torch.tensor([LS, 0.0, 0.0], device=dev)
    _, df, dW = h.margin_ce(feats, labels, label_smoothing=EPS, cos_planes=planes, operand="fp16", loss_scale=ls)
    check(df, dW, cs, "margin_ce fp16", LS)


@pytest.mark.parametrize("kern", [2, 5])
@pytest.mark.parametrize("mode", hb.MODES)
def test_margin_ce_fused(be, dev, mode, kern):
    """fused=True (the head in the cos GEMM's epilogue) on the eight-wave and the four-wave 256x256 TN kernel"""
    cs = case(mode, Cn=1003)
    h = make(mode, 1003, be, dev)
    feats, labels = load(h, cs[0], dev)
    be.lib.vdk_gemm_force_kernel(kern)
    try:
        _, df, dW = h.margin_ce(feats, labels, label_smoothing=EPS, fused=True)
    finally:
        be.lib.vdk_gemm_force_kernel(0)
    check(df, dW, cs, f"fused kernel {kern}")


@pytest.mark.parametrize("mode", hb.MODES)
def test_margin_ce_precise(be, dev, mode):
    """precise=True: fp32 cosines, an fp32 dcos and fp32 gradient products; the oracle is float32 torch without 16-bit rounding"""
    cs = case(mode, fmt=None)
    h = make(mode, 5003, be, dev)
    feats, labels = load(h, cs[0], dev)
    _, df, dW = h.margin_ce(feats, labels, label_smoothing=EPS, precise=True)
    check(df, dW, cs, "precise")


@pytest.mark.parametrize("mode", hb.MODES)
def test_autograd_form(be, dev, mode):
    """h(feats, labels) -> logits, torch's CrossEntropyLoss(label_smoothing) and backward: vdk_margin_ce's logits and vdk_margin_bwd"""
    cs = case(mode)
    h = make(mode, 5003, be, dev)
    feats, labels = load(h, cs[0], dev)
    feats.requires_grad_(True)
    torch.nn.functional.cross_entropy(h(feats, labels), labels, label_smoothing=EPS).backward()
    check(feats.grad, h.weight.grad, cs, "autograd")


@pytest.mark.parametrize("operand", ["bf16", "fp16"])
@pytest.mark.parametrize("mode", hb.MODES)
def test_sharded_form_in_one_process(be, dev, mode, operand):
    """heads.sharded_margin_ce without a process group at c_base = 0: the old passes (bf16) and the _amp passes (fp16 under a loss scale)"""
    f16 = operand == "fp16"
    cs = case(mode, fmt=HF, lscale=LS) if f16 else case(mode)
    h = make(mode, 5003, be, dev)
    feats, labels = load(h, cs[0], dev)
    kw = dict(operand="fp16", loss_scale=torch.tensor([LS, 0.0, 0.0], device=dev)) if f16 else {}
    _, df, dW = heads.sharded_margin_ce(h, feats, labels, h.weight.detach(), 0, 5003, label_smoothing=EPS, **kw)
    check(df, dW, cs, f"sharded {operand}", LS if f16 else 1.0)


@pytest.mark.parametrize("split", [2504, 2501])
@pytest.mark.parametrize("mode", hb.MODES)
def test_two_column_blocks(be, dev, mode, split):
    """the _amp passes on the column blocks [0, split) and [split, 5003) of one cosine matrix, driven as tests/test_sharded_head_fp16.py drives them (fp16, loss scale
    1024), the blocks' dcos joined and sent through the two gradient products: planted targets and hard negatives on both sides of the split"""
    cs = case(mode, fmt=HF, lscale=LS, extra=(split,))
    ph = cs[0]
    Cn, Bn = 5003, ph.feats.shape[0]
    h = make(mode, Cn, be, dev)
    feats, labels = load(h, ph, dev)
    w = h.weight.detach()
    st = heads._forward_cos(be, feats, w, 3, dtype=HF)
    ls = torch.tensor([LS, 0.0, 0.0], device=dev)
    blocks = [(0, split), (split, Cn - split)]
    gt = torch.zeros(Bn, device=dev)
    parts = []
    for c0, cl in blocks:
        g = torch.empty(Bn, device=dev)
        be.check(be.lib.vdk_margin_target_cos(st.cos.data_ptr() + 4 * c0, st.Cp, Bn, cl, c0, be.ptr(labels), be.ptr(g), be.stream()), "vdk_margin_target_cos")
        gt += g
    for c0, cl in blocks:
        s4 = torch.empty((Bn, 4), device=dev)
        be.check(be.lib.vdk_margin_stats_amp(C.byref(h.cfg), st.cos.data_ptr() + 4 * c0, st.Cp, Bn, cl, c0, be.ptr(labels), be.ptr(gt), be.ptr(s4), be.stream()), "vdk_margin_stats_amp")
        parts.append(s4)
    gmax = torch.stack([p[:, 0] for p in parts]).max(0).values.contiguous()
    gsum = sum(p[:, 1] * torch.exp(p[:, 0] - gmax) for p in parts).contiguous()
    dcos = torch.zeros((st.Bp, st.Cp), dtype=HF, device=dev)
    for c0, cl in blocks:
        ldd = (cl + 7) // 8 * 8
        d = torch.full((Bn, ldd), 7.0, dtype=HF, device=dev)
        be.check(be.lib.vdk_margin_grad_amp(C.byref(h.cfg), st.cos.data_ptr() + 4 * c0, st.Cp, Bn, cl, c0, Cn, be.ptr(labels), be.ptr(gt), be.ptr(gmax), be.ptr(gsum), EPS,
                                            1.0 / Bn, be.ptr(ls), be.ptr(d), ldd, _abi.F16_, be.stream()), "vdk_margin_grad_amp")
        dcos[:Bn, c0:c0 + cl] = d[:, :cl]
    df, dW = heads._backward_from_dcos(be, st, w, dcos)
    check(df, dW, cs, f"two blocks split {split}", LS)


def test_magface(be, dev):
    """MagFace: (logits, regulariser) -> CE + mean(regulariser), backward: the per-row margin in vdk_margin_ce / vdk_margin_bwd, the margin's own gradient path and the
    regulariser's; feature norms from below l_a to well inside (l_a, u_a)"""
    cs = case("arcface", mag=True, eps=0.0)
    h = make("arcface", 5003, be, dev, mag=True)
    feats, labels = load(h, cs[0], dev)
    feats.requires_grad_(True)
    logits, reg = h(feats, labels)
    (torch.nn.functional.cross_entropy(logits, labels) + reg.mean()).backward()
    check(feats.grad, h.weight.grad, cs, "magface")
