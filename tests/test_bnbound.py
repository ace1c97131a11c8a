"""tests/bnbound.py tested on itself (CPU only, no backend): a float32 torch evaluation passes every check at the shapes of tests/test_batchnorm_forms.py, every planted
fault is flagged, and the assert_close tolerances of tests/test_resnet_ops.py::test_bn_act_fwd_bwd (y 1e-4, 16-bit y 1e-2, running statistics rtol 1e-4 / atol 1e-5, 16-bit
dy rtol 2e-2 / atol 2e-3, dgamma / dbeta 1e-3, dres 1e-6) are set beside the same faults at 1000 x 72 (`OLD_TOLERANCES_SEE`, asserted either way).

What those tolerances do with them, as `OLD_TOLERANCES_SEE` asserts it: they SEE nine of the ten wherever a test reaches the path that has them --
  * a statistic taken from the neighbouring channel, a local count under SyncBatchNorm, batch terms in the eval-mode backward: errors of the size of the values themselves;
  * a biased running variance: 1e-3 of it at R = 1000 against rtol 1e-4;
  * one row missing from a channel's statistics, from dbeta or from dgamma: dout has random signs, so a sum over 1000 rows is about 30 and a missing term of +-1 stands far
    above 1e-3 (1 + |sum|);
  * the mask of one element: dres is compared at 1e-6 and the dead channel's dy carries invstd = 316;
  * E[x^2] - E[x]^2 at a mean of 100 sigma: exact sums rounded to fp32 allow 1.2e-3 of the variance at R = 1000, 6e-4 of invstd, 1.8e-3 of a y of 3 whose tolerance is 4e-4.
    (What ONE seed's two roundings do is luck -- 2.4e-5 of invstd at this file's seed, 1.8e-4 and 3.9e-4 at the next two -- so the record is taken on the largest error
    the roundings allow, not on the planted fault's own draw; the element bound flags the planted fault at every seed's size, `test_every_planted_fault_is_flagged`.)
They MISS a truncated 16-bit store (one 16-bit ulp against 1e-2).
So the old test's tolerances were not what hid the raw-moment variance: its DATA was -- x = 2 N(0, 1) + 0.3 has no far channel, no dead one, no eval mode and no second
rank, so the faults above were never reached."""
import math

import pytest
import torch

from tests import bnbound as N

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
SHAPES = [(2, 8), (7, 8), (257, 64), (300, 16), (1000, 72), (2049, 132), (4352, 260)]
OLD_TOLERANCES_SEE = {"raw_moment_variance": True, "stats_row_missing": True, "neighbour_channel_stats": True, "running_var_biased": True, "dbeta_row_missing": True,
                      "dgamma_row_missing": True, "mask_from_unrounded": True, "local_count_under_sync": True, "batch_terms_in_eval_backward": True,
                      "truncated_store": False}


def _case(R, C, out16=BF, train=True, n=None, **kw):
    inp = N.inputs(R, C, seed=1000 * R + C, **kw)
    inp = inp if train else N.warmed(inp)
    ok = N.evaluate(inp, F32, train=train, N=n, out16=out16)
    given = ok["given"]
    ref = N.reference64(inp, given, train=train, N=n)
    B, e32 = N.bounds(inp, ref, given, train=train, N=n)
    return inp, ok, given, ref, B, e32


def _got(ev, with_f32=True):
    """an evaluation as a kernel's outputs: f32 statistics and sums, y f32 (or not) and the 16-bit copies"""
    out = {k: ev[k].float() for k in N.STATS + ("dgamma", "dbeta", "dres")}
    out.update({"y": ev["y"].float() if with_f32 else None, "y16": ev["y16"], "dy16": ev["dy16"]})
    return out


def _flagged(ev, ref, B, e32, what, train=True, with_f32=True):
    with pytest.raises(AssertionError):
        N.check_all(_got(ev, with_f32), ref, B, e32, what, train=train)


@pytest.mark.parametrize("R,C", SHAPES)
def test_float32_evaluation_passes(R, C):
    for kw in ({}, {"far": True, "dead": True, "res": F32, "relu": True}, {"far": True, "res": BF, "relu": True}, {"dead": True, "relu": True}):
        for out16 in (BF, HF):
            if kw.get("res") == BF and out16 == HF:
                kw = {**kw, "res": HF}
            for train in (True, False):
                inp, ok, given, ref, B, e32 = _case(R, C, out16, train, **kw)
                what = f"float32 {R} x {C} {kw} train={int(train)}"
                faults = N.FAULTS
                if R == 2 and kw.get("relu"):          # (two rows of a channel can both end below the ReLU: nothing of its invstd is left in y, no row in its sums)
                    faults = tuple(f for f in faults if f not in ("neighbour_channel_stats", "dbeta_row_missing", "dgamma_row_missing"))
                N.assert_sensitive(inp, ref, B, given, faults, train=train, out16=out16, what=what)
                N.check_all(_got(ok), ref, B, e32, what, train=train)
                N.check_all(_got(ok, with_f32=False), ref, B, e32, what + ", 16-bit only", train=train)          # the half-ulp rule against float64
                N.check_backward({"dy": ok["dy"].float()}, ref, B, e32, what + ", f32 dy")
                if inp["dead"] and train:
                    N.check_dead(_got(ok), inp, what)


@pytest.mark.parametrize("R,C", SHAPES)
def test_float32_evaluation_in_another_order_passes(R, C):
    """the rows reversed: other float32 sums, the same bound (B is FACTOR x the oracle's error or the floor, not the oracle's own error)"""
    inp, ok, given, ref, B, e32 = _case(R, C, far=True, res=F32, relu=True)
    flip = N.rows(inp, torch.arange(R - 1, -1, -1))
    other = N.evaluate(flip, F32, given={**given, "stored": given["stored"].flip(0)})
    got = _got(other)
    for k in ("y", "y16", "dy16", "dres"):
        got[k] = got[k].flip(0)
    N.check_all(got, ref, B, e32, f"float32, rows reversed {R} x {C}")


def _fault_case(name, R, C):
    """the case that shows `name`: far + dead channels, fp32 residual, ReLU, fp16 stores; eval mode / a two-rank batch for the two faults that need them"""
    train = name != "batch_terms_in_eval_backward"
    local = R // 3 if name == "local_count_under_sync" else None
    inp, ok, given, ref, B, e32 = _case(R, C, HF, train, far=True, dead=True, res=F32, relu=True)
    shown = N.assert_sensitive(inp, ref, B, given, (name,), train=train, local_rows=local, out16=HF, what=f"{name} {R} x {C}")
    assert shown == [name], (name, "not shown at", R, C)
    bad = N.plant(name, inp, given, train=train, local_rows=local, out16=HF)
    return inp, bad, ref, B, e32, train


@pytest.mark.parametrize("R,C", [(7, 8), (300, 16), (1000, 72), (2049, 132), (4352, 260)])
@pytest.mark.parametrize("name", N.FAULTS)
def test_every_planted_fault_is_flagged(name, R, C):
    inp, bad, ref, B, e32, train = _fault_case(name, R, C)
    _flagged(bad, ref, B, e32, f"{name} {R} x {C}", train)
    if name == "truncated_store":          # also without the kernel's own f32 y to compare with
        _flagged(bad, ref, B, e32, f"{name} {R} x {C}, 16-bit only", train, with_f32=False)


@pytest.mark.parametrize("R,C", [(300, 16), (2049, 132)])
def test_row_faults_at_every_edge(R, C):
    """both sides of the slice edge, the first and the last row; an ordinary and a far channel"""
    inp, ok, given, ref, B, e32 = _case(R, C, far=True, res=F32, relu=False)
    rps = N.slices(R, C)[1]
    for r in sorted({0, rps - 1, rps, R - 1}):
        for c in (4, C - 1):
            for name in ("stats_row_missing", "dbeta_row_missing", "dgamma_row_missing"):
                N.assert_sensitive(inp, ref, B, given, (name,), at=(r, c), what=f"{name} at ({r}, {c})")
                _flagged(N.plant(name, inp, given, at=(r, c)), ref, B, e32, f"{name} at ({r}, {c})")


def _close(got, want, rtol, atol):
    got, want = got.double(), want.double()
    return bool(((got - want).abs() <= atol + rtol * want.abs()).all())


def old_tolerances_see(bad, ref):
    """the assertions of test_bn_act_fwd_bwd on `bad`, with float64 where that test has torch's float32 autograd (two 16-bit values compare as it compares them: rounded)"""
    o16 = bad["y16"].dtype
    ok = (_close(bad["y"], ref["y"], 1e-4, 1e-4) and _close(bad["y16"].float(), ref["y"].float().to(o16).float(), 1e-2, 1e-2)
          and _close(bad["rmean"], ref["rmean"], 1e-4, 1e-5) and _close(bad["rvar"], ref["rvar"], 1e-4, 1e-5)
          and _close(bad["dy16"].float(), ref["dy"].float().to(o16).float(), 2e-2, 2e-3) and _close(bad["dgamma"], ref["dgamma"], 1e-3, 1e-3)
          and _close(bad["dbeta"], ref["dbeta"], 1e-3, 1e-3) and _close(bad["dres"], ref["dres"], 1e-6, 1e-6))
    return not ok


@pytest.mark.parametrize("name", N.FAULTS)
def test_old_tolerances_beside_the_element_bound(name):
    """see the module docstring: what assert_close at the old tolerances does with each fault at 1000 x 72 is asserted either way.  A fault in the statistics reaches y, dy
    and the sums through them here, as it does in a kernel: the downstream values are evaluated from the faulty statistics."""
    R, C = 1000, 72
    inp, bad, ref, B, e32, train = _fault_case(name, R, C)
    if name in ("raw_moment_variance", "stats_row_missing"):          # the faulty statistics are what the apply step and the backward are handed
        st = N.statistics(inp, F32, name, N.default_at(inp))
        if name == "raw_moment_variance":
            # What the two fp32 roundings of this one seed do is luck (2.4e-5 of invstd here, 1.8e-4 and 3.9e-4 at the next two seeds).  The record is taken on the
            # largest error that exact sums rounded to fp32 ALLOW: half an fp32 ulp of sum x^2, and of sum x times 2 |mean|, over R.
            c = N.default_at(inp)[1]
            x = inp["x"].double()[:, c]
            half_ulp = lambda v: 2.0 ** (math.floor(math.log2(abs(float(v)))) - 24)
            dvar = (half_ulp((x * x).sum()) + 2 * abs(float(x.mean())) * half_ulp(x.sum())) / R
            exact = N.statistics(inp, torch.float64)
            var = exact["var"].clone(); var[c] += dvar
            st = {**exact, "var": var, "invstd": 1.0 / torch.sqrt(var + inp["eps"])}
            st["rvar"] = (1 - inp["momentum"]) * inp["rvar"].double() + inp["momentum"] * var * R / (R - 1.0)
            print(f"raw moments at 100 sigma, R = {R}: exact sums rounded to fp32 allow {dvar / float(exact['var'][c]):.2e} of the variance")
            st = {k: v.float() for k, v in st.items()}
        bad = N.evaluate(inp, F32, given={"mean": st["mean"], "invstd": st["invstd"], "stored": None}, out16=HF)
        bad.update({k: st[k] for k in N.STATS})
        true = N.evaluate(inp, torch.float64, out16=HF)
        ref = N.reference64(inp, true["given"])
    sees = old_tolerances_see(bad, ref)
    print(f"{name}: the old tolerances {'see' if sees else 'miss'} it")
    assert sees == OLD_TOLERANCES_SEE[name], (name, sees)
