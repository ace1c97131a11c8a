"""The BatchNorm kernels element by element against float64 (tests/bnbound.py): vdk_bn_act_fwd / _bwd (train, eval, SyncBatchNorm in one process, both 16-bit formats),
vdk_bn_rows_bwd, vdk_batchnorm1d_fwd / _bwd and the global average pool, on far channels (mean = 100 sigma) and a dead one.  Every reduction has a fixed order: each call
is made twice and must give the same bits.

The shapes come from the routing (csrc/resnet_ops.hip, csrc/norm_loss.hip):
  * bn_slices: S = min(1024 / ceil(C / 64), ceil(R / 256)) slices of rps = ceil(R / S) rows; bn_partial_kernel: workgroups of 64 columns x 8 row groups
      2 x 8, 7 x 8      fewer rows than row groups
      257 x 64          two slices, 129 + 128
      300 x 16          part of one column block
      1000 x 72         second column block 8 wide, rps = 250, no multiple of 8
      2049 x 132        9 slices, ragged last (228 + 225)
      4352 x 260        17 slices: more than one pass of the backward's bn_combine_kernel (16 columns x 16 slice groups)
      16640 x 8         65 slices: more than one pass of the forward's bn_combine_fwd_kernel (4 columns x 64 slice groups)
      8200 x 2048       `hip` only: the slice cap, S = 32, rps = 257
  * vdk_batchnorm1d_*: bn1d_*_kernel (a thread per column) below B = 256, bnrows_*_kernel (32 columns x 16 row groups) from there on: B = 255, 256, 257."""
import functools

import pytest
import torch

from tests import bnbound as N
from tests import gemmbound
from tests.lnbound import scaled
from visiondk_amd import ops

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
IDS = {BF: "bf16", HF: "fp16", F32: "f32", None: "none"}
# (R, C): [(res, relu, far, dead, 16-bit format)]
ACT_CASES = {
    (2, 8): [(None, 0, False, False, BF), (F32, 1, True, True, HF)],
    (7, 8): [(None, 1, False, False, BF), (BF, 0, True, True, BF)],
    (257, 64): [(None, 0, False, False, BF), (F32, 1, True, False, BF)],
    (300, 16): [(None, 1, False, False, BF), (F32, 1, True, True, HF), (HF, 0, True, True, HF), (BF, 1, True, True, BF)],
    (1000, 72): [(BF, 1, False, False, BF), (F32, 0, True, True, BF), (F32, 1, True, True, HF), (None, 1, True, True, BF)],
    (2049, 132): [(None, 0, True, True, BF), (BF, 1, True, True, BF)],
    (4352, 260): [(F32, 1, True, True, BF)],
    (16640, 8): [(None, 1, True, True, BF)],
}
ACT = [(R, C) + kw for (R, C), kws in ACT_CASES.items() for kw in kws]
ACT_ID = lambda v: IDS.get(v, str(v)) if not isinstance(v, bool) else str(int(v))


@functools.lru_cache(maxsize=None)
def case(R, C, res=None, relu=False, far=False, dead=False):
    """the inputs of one case: made once, shared by the backends and the tests, never modified"""
    return N.inputs(R, C, seed=1000 * R + C, res=res, relu=bool(relu), far=far, dead=dead)


def same_bits(a, b, what):
    for k in a:
        if a[k] is not None:
            assert torch.equal(gemmbound.bits(a[k]), gemmbound.bits(b[k])), (what, k, "differs between two runs")


def bn_act(be, dev, inp, out16, train=True, want_f32=True, sync_fwd=None, sync_bwd=None, forward_only=False):
    """vdk_bn_act_fwd, then vdk_bn_act_bwd on the forward's own stats buffer [2C + 1] and stored output -> (dict of CPU outputs, the stats buffer)"""
    C = inp["C"]
    d = lambda t: None if t is None else t.to(dev).contiguous()
    x, gamma, beta, dout, res = (d(inp[k]) for k in ("x", "gamma", "beta", "dout", "res"))
    rm, rv = inp["rmean"].clone().to(dev), inp["rvar"].clone().to(dev)
    stats = torch.full((2 * C + 1,), float("nan"), dtype=F32, device=dev)
    with ops.resnet_ops_format(out16, backend=be):
        y16, y, sm, si = ops.bn_act_fwd(x, gamma, beta, rm, rv, training=train, eps=inp["eps"], momentum=inp["momentum"], res=res, relu=inp["relu"], want_f32=want_f32,
                                        stats=stats, sync=sync_fwd, backend=be)
        out = {"mean": sm, "invstd": si, "count": stats[2 * C:], "rmean": rm, "rvar": rv, "y": y, "y16": y16}
        if not forward_only:
            dy16, dres, dg, db = ops.bn_act_bwd(x, dout, y16 if inp["relu"] else None, gamma, None, None, stats=stats, sync=sync_bwd, backend=be)
            out.update({"dy16": dy16, "dres": dres, "dgamma": dg, "dbeta": db})
    if be.device_only:
        torch.cuda.synchronize()
    assert y16.dtype == out16
    return {k: (None if v is None else v.detach().cpu().clone()) for k, v in out.items()}, stats


def given_of(got, inp):
    return {"mean": got["mean"], "invstd": got["invstd"], "stored": got["y16"] if inp["relu"] else None}


def judge(got, inp, out16, what, train=True, sensitive=True):
    """reference, bounds and preconditions from the kernel's own saved statistics and stored output, then every check -> {kind: worst error / bound}"""
    given = given_of(got, inp)
    ref = N.reference64(inp, given, train=train)
    B, e32 = N.bounds(inp, ref, given, train=train)
    if sensitive:
        N.assert_sensitive(inp, ref, B, given, train=train, out16=out16, what=what)
    worst = N.check_all(got, ref, B, e32, what, train=train)
    if inp["dead"] and train:
        N.check_dead(got, inp, what)
    assert float(got["count"][0]) == (inp["R"] if train else 0.0), (what, "saved sample count", float(got["count"][0]))
    return worst


# ---------------------------------------------------------------------------------------------------------------- vdk_bn_act_fwd / _bwd
@pytest.mark.parametrize("R,C,res,relu,far,dead,out16", ACT, ids=ACT_ID)
def test_bn_act_train(be, dev, R, C, res, relu, far, dead, out16):
    inp = case(R, C, res, relu, far, dead)
    what = f"{be.name} bn_act {R} x {C} res={IDS[res]} relu={relu} far={int(far)} dead={int(dead)} {IDS[out16]}"
    got, _ = bn_act(be, dev, inp, out16)
    same_bits(got, bn_act(be, dev, inp, out16)[0], what)
    judge(got, inp, out16, what)
    only16, _ = bn_act(be, dev, inp, out16, want_f32=False)          # as the ResNet engine calls it: the 16-bit output is the activation
    assert only16["y"] is None
    same_bits(only16, got, what + ", 16-bit output only")


@pytest.mark.gpu
def test_bn_act_slice_cap(hip):
    """8200 x 2048: 32 column blocks cap the slices at 32 of 257 rows (ceil(R / 256) would be 33)"""
    R, C = 8200, 2048
    assert N.slices(R, C) == (32, 257)
    inp = case(R, C, None, 0, True, True)
    got, _ = bn_act(hip, "cuda", inp, BF)
    judge(got, inp, BF, f"hip bn_act {R} x {C}", sensitive=False)          # (the preconditions are those of the smaller far + dead cases)


@pytest.mark.parametrize("R,C,res,relu,out16", [(7, 8, None, 1, BF), (300, 16, F32, 1, HF), (1000, 72, BF, 0, BF), (2049, 132, F32, 1, BF)], ids=ACT_ID)
def test_bn_act_eval(be, dev, R, C, res, relu, out16):
    """forward on the running statistics (left untouched, save_mean = running_mean bit for bit, count 0) and the backward's `fwd_count == 0` branch: dy = gamma invstd g"""
    inp = N.warmed(case(R, C, res, relu, True, True))
    what = f"{be.name} bn_act eval {R} x {C} res={IDS[res]} relu={relu} {IDS[out16]}"
    got, _ = bn_act(be, dev, inp, out16, train=False)
    same_bits(got, bn_act(be, dev, inp, out16, train=False)[0], what)
    judge(got, inp, out16, what, train=False)


@pytest.mark.parametrize("R,Ra,C,out16", [(300, 113, 16, BF), (1000, 380, 72, HF), (2049, 1500, 132, BF)], ids=ACT_ID)
def test_sync_batchnorm_in_one_process(be, dev, R, Ra, C, out16):
    """Two ranks' rows in one process: rank B's vector is copied out of a first call, rank A's call adds it in place (the SUM all-reduce, on the same stream), and rank B's
    second call receives the combined vector.  Rank A's statistics, outputs and backward against float64 BatchNorm of ALL rows.  Ordinary channels start from
    running_mean = 0 (K = 0: the raw moments, harmless at a mean of 0.25 sigma); the far channels from the batch mean rounded to fp32, a warmed-up module."""
    whole = dict(case(R, C, F32, 1, True, True))
    mu = whole["x"].double().mean(0).float()
    far = torch.zeros(C, dtype=torch.bool); far[1::3] = True
    whole["rmean"] = torch.where(far, mu, torch.zeros(C))
    a, b = N.rows(whole, slice(0, Ra)), N.rows(whole, slice(Ra, R))
    what = f"{be.name} sync {Ra} + {R - Ra} x {C} {IDS[out16]}"
    box = {}
    copy_out = lambda key: (lambda v: box.__setitem__(key, v.clone()))
    add_in = lambda key, keep: (lambda v: (v.add_(box[key]), box.__setitem__(keep, v.clone())))
    copy_in = lambda key: (lambda v: v.copy_(box[key]))
    bn_act(be, dev, b, out16, sync_fwd=copy_out("fb"), forward_only=True)
    fa, stats_a = bn_act(be, dev, a, out16, sync_fwd=add_in("fb", "fsum"), forward_only=True)
    gb, stats_b = bn_act(be, dev, b, out16, sync_fwd=copy_in("fsum"), sync_bwd=copy_out("bb"))
    assert torch.equal(gemmbound.bits(stats_b.cpu()), gemmbound.bits(stats_a.cpu())), (what, "the two ranks' statistics differ")
    ga, _ = bn_act(be, dev, a, out16, sync_fwd=add_in("fb", "fsum"), sync_bwd=add_in("bb", "bsum"))
    same_bits(fa, ga, what + ": forward")
    assert float(ga["count"][0]) == R and float(box["bsum"][2 * C]) == R
    given = {"mean": ga["mean"], "invstd": ga["invstd"], "stored": torch.cat([ga["y16"], gb["y16"]])}
    ref = N.reference64(whole, given)
    B, e32 = N.bounds(whole, ref, given)
    N.assert_sensitive(whole, ref, B, given, local_rows=Ra, out16=out16, what=what)
    N.check_statistics(ga, ref, B, e32, what)
    rows_a = slice(0, Ra)
    ref_a = {k: (v[rows_a] if k in ("y", "s_y") else v) for k, v in ref.items()}
    N.check_forward(ga, ref_a, B, e32, what)
    local = N.reference64(a, {**given, "stored": ga["y16"]}, N=R)          # dgamma / dbeta stay local sums
    N.check_backward({"dgamma": ga["dgamma"], "dbeta": ga["dbeta"]}, local, B, e32, what + " local sums")
    N.check_backward({"dy16": ga["dy16"], "dres": ga["dres"]}, ref, B, e32, what, rows_of=rows_a)
    N.check_dead(ga, a, what)


# ---------------------------------------------------------------------------------------------------------------- vdk_bn_rows_bwd
@pytest.mark.parametrize("R,C", [(300, 16), (1000, 72), (4352, 260)])
def test_bn_rows_bwd(be, dev, R, C):
    """fp32 dx, no mask, handed the float64 statistics rounded to fp32"""
    inp = case(R, C, None, 0, True, True)
    st = N.statistics(inp)
    given = {"mean": st["mean"].float(), "invstd": st["invstd"].float(), "stored": None}
    what = f"{be.name} bn_rows_bwd {R} x {C}"
    runs = []
    for _ in range(2):
        dx, dg, db = ops.bn_rows_bwd(inp["x"].to(dev), inp["dout"].to(dev), inp["gamma"].to(dev), given["mean"].to(dev), given["invstd"].to(dev), backend=be)
        runs.append({"dy": dx.cpu(), "dgamma": dg.cpu(), "dbeta": db.cpu()})
    same_bits(runs[0], runs[1], what)
    ref = N.reference64(inp, given)
    B, e32 = N.bounds(inp, ref, given)
    N.assert_sensitive(inp, ref, B, given, ("dbeta_row_missing", "dgamma_row_missing"), what=what)
    N.check_backward(runs[0], ref, B, e32, what)
    N.check_dead(runs[0], inp, what)


# ---------------------------------------------------------------------------------------------------------------- vdk_batchnorm1d_fwd / _bwd
def bn1d(be, dev, inp, train, ldx=None):
    B_, F = inp["R"], inp["C"]
    ldx = F if ldx is None else ldx
    wide = torch.full((B_, ldx), float("nan"), dtype=F32)
    wide[:, :F] = inp["x"]
    xw = wide.to(dev)
    gamma, beta, dout = (inp[k].to(dev) for k in ("gamma", "beta", "dout"))
    rm, rv = inp["rmean"].clone().to(dev), inp["rvar"].clone().to(dev)
    y = torch.full((B_, F), float("nan"), dtype=F32, device=dev)
    sm, si = (torch.full((F,), float("nan"), dtype=F32, device=dev) for _ in range(2))
    be.check(be.lib.vdk_batchnorm1d_fwd(be.ptr(xw), ldx, B_, F, be.ptr(gamma), be.ptr(beta), inp["eps"], inp["momentum"], int(train), be.ptr(rm), be.ptr(rv), be.ptr(y), F,
                                        be.ptr(sm), be.ptr(si), be.stream()), "vdk_batchnorm1d_fwd")
    out = {"mean": sm, "invstd": si, "rmean": rm, "rvar": rv, "y": y}
    if train:
        dx, dg, db = (torch.full(s, float("nan"), dtype=F32, device=dev) for s in ((B_, F), (F,), (F,)))
        be.check(be.lib.vdk_batchnorm1d_bwd(be.ptr(dout), F, be.ptr(xw), ldx, B_, F, be.ptr(gamma), be.ptr(sm), be.ptr(si), be.ptr(dx), F, be.ptr(dg), be.ptr(db),
                                            be.stream()), "vdk_batchnorm1d_bwd")
        out.update({"dy": dx, "dgamma": dg, "dbeta": db})
    if be.device_only:
        torch.cuda.synchronize()
    return {k: v.cpu().clone() for k, v in out.items()}


@pytest.mark.parametrize("F", [33, 72, 100, 260])
@pytest.mark.parametrize("B_", [2, 7, 255, 256, 257, 1000])
def test_batchnorm1d(be, dev, B_, F):
    inp = case(B_, F, None, 0, True, True)
    for train in (True, False):
        what = f"{be.name} bn1d {B_} x {F} train={int(train)}"
        got = bn1d(be, dev, inp, train)
        same_bits(got, bn1d(be, dev, inp, train), what)
        given = given_of({**got, "y16": None}, inp)
        ref = N.reference64(inp, given, train=train)
        Bd, e32 = N.bounds(inp, ref, given, train=train)
        faults = [f for f in N.FAULTS if f not in ("truncated_store", "batch_terms_in_eval_backward")]          # (fp32 outputs; no eval-mode backward here)
        N.assert_sensitive(inp, ref, Bd, given, faults, train=train, what=what)
        N.check_all(got, ref, Bd, e32, what, train=train)
        if train:
            N.check_dead(got, inp, what)
    if (B_, F) in ((255, 100), (257, 100)):          # rows further apart than they are long, on both kernels
        same_bits(bn1d(be, dev, inp, True, ldx=F + 12), bn1d(be, dev, inp, True), f"bn1d {B_} x {F}, ldx = F + 12")


# ---------------------------------------------------------------------------------------------------------------- vdk_avgpool_fwd / _bwd
@pytest.mark.parametrize("dtype", [BF, HF], ids=IDS.get)
@pytest.mark.parametrize("Bt,HW,C", [(3, 49, 8), (2, 1, 72), (5, 196, 264)])
def test_avgpool(be, dev, Bt, HW, C, dtype):
    """forward: the half-ulp rule against the float64 mean, slack B S with S = mean |x| and B from torch's float32 mean (or the floor); rows from B on exactly zero.
    backward: dfeat / HW, exact up to the one fp32 division (half an fp32 ulp of the quotient), every pixel of a sample the same"""
    g = torch.Generator().manual_seed(Bt * 1000 + HW + C)
    x = torch.randn(Bt, HW, C, generator=g, dtype=torch.float64).float().to(dtype)
    Bp, ld = Bt + 3, C + 8
    dfeat = torch.randn(Bp, ld, generator=g, dtype=torch.float64).float().to(dtype)
    what = f"{be.name} avgpool {Bt} x {HW} x {C} {IDS[dtype]}"
    with ops.resnet_ops_format(dtype, backend=be):
        out = ops.avgpool_fwd(x.to(dev), Bp, backend=be).cpu()
        dmap = ops.avgpool_bwd(dfeat.to(dev), Bt, HW, C, backend=be).cpu()
    assert out.dtype == dtype and bool((gemmbound.bits(out[Bt:]) == 0).all()), (what, "padded rows")
    x64 = x.double()
    ref, s = x64.mean(1), x64.abs().mean(1)
    e32 = N.worst(scaled(x.float().mean(1), ref, s))[0]
    gemmbound.check_half_ulp(out[:Bt], ref, max(N.FACTOR * e32, N.FLOOR) * s, what + " forward")
    want = (dfeat[:Bt, :C].double() / HW)[:, None, :].expand(Bt, HW, C).reshape(Bt * HW, C)
    gemmbound.check_within(dmap, want, want.abs() * N.U32, what + " backward")
    assert torch.equal(dmap.reshape(Bt, HW, C), dmap.reshape(Bt, HW, C)[:, :1].expand(Bt, HW, C)), (what, "pixels of one sample differ")
