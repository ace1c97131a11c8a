"""TEST INFRASTRUCTURE: per-element bounds for the BatchNorm kernels of csrc/resnet_ops.hip and csrc/norm_loss.hip (tests/test_batchnorm_forms.py; tested on itself by
tests/test_bnbound.py).  The counterpart of tests/lnbound.py for the column statistics.

Everything is float64 of the kernel's OWN inputs.  The apply step and the backward are evaluated with the f32 mean / invstd the kernel is handed or produced itself (and the
ReLU mask with the 16-bit output it stored and reads back), so the statistics' error is no part of their check; the statistics are checked on their own:

  mu = mean_r x,  var = mean_r (x - mu)^2 (two-pass, centred),  invstd = (var + eps)^-1/2          S_mean = mean_r |x|,  S_invstd = invstd  (S_var = var + eps, centred: a
  rmean' = (1 - m) rmean + m mu,  rvar' = (1 - m) rvar + m var R / (R - 1)                                 relative error of invstd beyond B fails however far the mean lies)
                                                                                                     S_rmean = (1 - m) |rmean| + m S_mean,  S_rvar = (1 - m) |rvar| + m S_var R / (R - 1)
  y = gamma (x - mean) invstd + beta [+ res] [relu]   (train: batch statistics; eval: running)        S_y = |gamma (x - mean)| invstd + |beta| + |res|
  g = dout [out16 > 0],  xh = (x - mean) invstd,  dres = g (exactly)
  dbeta = sum_r g,  dgamma = sum_r g xh                                                               S_dbeta = sum_r |g|,  S_dgamma = sum_r |g xh|
  train: dy = gamma invstd / N (N g - sum g - xh sum(g xh)),  N = the sample count behind the statistics     S_dy = |gamma| invstd / N (N |g| + sum |g| + |xh| sum |g xh|)
  eval:  dy = gamma invstd g                                                                          S_dy = |gamma| invstd |g|

and |got - ref64| <= B S per element with B = max(FACTOR x E32, FLOOR): E32 = the worst scaled error of a float32 torch evaluation of the same formulas on the same inputs
(`evaluate(inp, torch.float32, given=...)`), never taken from a kernel; FACTOR = rowbound.FACTOR (another correct summation order).  FLOOR = 16 x 2^-24 counts the roundings
of ONE element's own chain, the longest being dy's: x - mean, . invstd, N . g, - sum g, xh . sum(g xh), -, gamma . invstd, / N, the last product (9), and the tails of the
two column sums it consumes, three each however the rows are ordered (the thread's last addition, the workgroup's last addition, the rounding of the combined sum to fp32):
15, rounded up to 16.  The statistics' chains are shorter (x - mu, square, the sum's tail, / R, + eps, sqrt, reciprocal: 9).  torch's pairwise sums can be luckier than any
kernel's order, which is what a floor is for; it is not tuned against a kernel.

16-bit outputs are RNE16 of the kernel's own fp32 value bit for bit where both are returned, or obey gemmbound's half-ulp rule against float64 with B S as the slack.
A dead channel (all zeros, what a ReLU leaves behind) has mean = 0, invstd = eps^-1/2, y = beta + res, dgamma = 0 as equalities (`check_dead`); its beta is 0, so that with an
fp32 residual one element of it can hold 2^-30: positive in fp32, zero once stored as fp16 -- where a mask taken from the unrounded value differs from the stored one.

`assert_sensitive` holds the preconditions (from float64 alone: every fault of the list moves its element by >= SIGNAL_FACTOR x B S); `evaluate(..., fault=...)` / `plant`
are the faults of the self-test."""
from __future__ import annotations

import math

import torch

from tests import gemmbound
from tests.lnbound import rne16, scaled, truncate16
from tests.rowbound import FACTOR, SIGNAL_FACTOR

U32 = 2.0 ** -24
FLOOR = 16 * U32
EPS, MOMENTUM = 1e-5, 0.1
FAR_MEAN = 200.0                     # sigma = 2: 100 standard deviations, the same as lnbound's far rows
DEAD = 0                             # the dead channel; far channels are 1, 4, 7, ...
TINY = 2.0 ** -30                    # > 0 in fp32, 0 in fp16
STATS = ("mean", "invstd", "rmean", "rvar")
BACKWARD = ("dy", "dgamma", "dbeta")
FAULTS = ("raw_moment_variance", "stats_row_missing", "neighbour_channel_stats", "running_var_biased", "dbeta_row_missing", "dgamma_row_missing", "mask_from_unrounded",
          "local_count_under_sync", "batch_terms_in_eval_backward", "truncated_store")
KINDS_OF = {"raw_moment_variance": ("invstd", "rvar"), "stats_row_missing": ("mean", "invstd"), "neighbour_channel_stats": ("y",), "running_var_biased": ("rvar",),
            "dbeta_row_missing": ("dbeta",), "dgamma_row_missing": ("dgamma",), "mask_from_unrounded": ("dbeta",), "local_count_under_sync": ("dy",),
            "batch_terms_in_eval_backward": ("dy",)}          # where each fault shows first (truncated_store: the 16-bit copies, against the half-ulp rule)


def signed(shape, g):
    """random signs, magnitudes in [0.5, 1.5): no contribution is close to zero"""
    return (torch.rand(shape, generator=g, dtype=torch.float64) + 0.5) * (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)


def worst(e):
    """-> (the largest entry, its index)"""
    i = int(e.argmax())
    return float(e.reshape(-1)[i]), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), e.shape))


def slices(R, C):
    """bn_slices of csrc/resnet_ops.hip -> (S, rows per slice)"""
    S = max(1, min(1024 // ((C + 63) // 64), (R + 255) // 256))
    return S, (R + S - 1) // S


# ---------------------------------------------------------------------------------------------------------------- inputs
def inputs(R, C, seed, *, far=False, dead=False, res=None, relu=False):
    """-> dict: x f32 [R, C] = 2 N(0, 1) + 0.5 (`far`: channels 1, 4, 7, ... moved to a mean of 200 = 100 sigma, channels 5 and 6 to 2.5 and 3.5 sigma; `dead`: channel 0 all zeros, its beta 0), gamma f32 [C] and
    dout f32 [R, C] with random signs and magnitudes in [0.5, 1.5), beta N(0, 1), res (None | a dtype: N(0, 1) rounded to it; with `dead` and float32 one element of the dead
    channel is 2^-30), rmean = N(0, 0.5), rvar in [0.5, 1.5): not the initial 0 / 1, so that the update shows."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, C, generator=g, dtype=torch.float64) * 2 + 0.5
    if far:
        x[:, 1::3] += FAR_MEAN - 0.5
        if C > 6:          # both sides of bn_partial_kernel's rule (raw moments while a slice's mean^2 <= 9 variance): means of 2.5 and 3.5 sigma
            x[:, 5] += 5.0 - 0.5
            x[:, 6] += 7.0 - 0.5
    if dead:
        x[:, DEAD] = 0
    gamma = signed((C,), g).float()
    beta = torch.randn(C, generator=g, dtype=torch.float64).float()
    dout = signed((R, C), g).float()
    r = None
    if res is not None:
        r = torch.randn(R, C, generator=g, dtype=torch.float64).float()
        if dead and res == torch.float32:
            r[R // 2, DEAD] = TINY
        r = r.to(res)
    if dead:
        beta[DEAD] = 0
    rmean = (torch.randn(C, generator=g, dtype=torch.float64) * 0.5).float()
    rvar = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).float()
    return {"x": x.float(), "gamma": gamma, "beta": beta, "dout": dout, "res": r, "rmean": rmean, "rvar": rvar, "relu": relu, "far": far, "dead": dead, "R": R, "C": C,
            "eps": EPS, "momentum": MOMENTUM}


def rows(inp, sl):
    """the same case restricted to the rows `sl` (one rank's share of a SyncBatchNorm batch)"""
    out = dict(inp)
    for k in ("x", "dout", "res"):
        out[k] = None if inp[k] is None else inp[k][sl].contiguous()
    out["R"] = out["x"].shape[0]
    return out


def warmed(inp):
    """the same case with running statistics near the batch's (1.01 mu + 0.1, 1.1 var + 0.01): what eval mode meets in a trained module -- with the random ones a far
    channel's y is +-100 gamma and a ReLU leaves nothing of half of those channels"""
    x = inp["x"].double()
    mu = x.mean(0)
    out = dict(inp)
    out["rmean"] = (1.01 * mu + 0.1).float()
    out["rvar"] = (1.1 * ((x - mu) ** 2).mean(0) + 0.01).float()
    return out


def default_at(inp):
    """where `plant` puts a fault: the last row of the first slice of the statistics kernels, channel 4 (a far one when there are far ones, never the dead one)"""
    return slices(inp["R"], inp["C"])[1] - 1, 4 if inp["C"] > 4 else inp["C"] - 1


# ---------------------------------------------------------------------------------------------------------------- the formulas, in any precision, with an optional fault
def statistics(inp, prec=torch.float64, fault=None, at=(0, 0), train=True):
    """mean, var, invstd and the updated running statistics (eval mode: the running statistics, unchanged), every operation in `prec`"""
    r, c = at
    x, rmean, rvar = (inp[k].to(prec) for k in ("x", "rmean", "rvar"))
    R, eps, m = inp["R"], inp["eps"], inp["momentum"]
    if not train:
        return {"mean": rmean, "var": rvar, "invstd": 1.0 / torch.sqrt(rvar + eps), "rmean": rmean, "rvar": rvar}
    mu = x.sum(0) / R
    var = ((x - mu) ** 2).sum(0) / R
    if fault == "stats_row_missing":          # (still divided by R: the row was never read)
        keep = torch.ones(R, dtype=torch.bool); keep[r] = False
        mu = mu.clone(); var = var.clone()
        mu[c] = x[keep, c].sum() / R
        var[c] = ((x[keep, c] - mu[c]) ** 2).sum() / R
    if fault == "raw_moment_variance":        # sums of any quality, rounded to fp32 once, then E[x^2] - E[x]^2
        x64 = inp["x"].double()[:, c]
        s1, s2 = x64.sum().float().double(), (x64 * x64).sum().float().double()
        var = var.clone()
        var[c] = (s2 / R - (s1 / R) ** 2).clamp_min(0).to(prec)
    unbiased = var * (R / (R - 1.0)) if (R > 1 and fault != "running_var_biased") else var
    return {"mean": mu, "var": var, "invstd": 1.0 / torch.sqrt(var + eps), "rmean": (1 - m) * rmean + m * mu, "rvar": (1 - m) * rvar + m * unbiased}


def apply(inp, mean, invstd, prec=torch.float64, fault=None, at=(0, 0)):
    """y (before any 16-bit store) from the handed statistics"""
    x, gamma, beta, mean, invstd = (t.to(prec) for t in (inp["x"], inp["gamma"], inp["beta"], mean, invstd))
    if fault == "neighbour_channel_stats":
        c = at[1]
        n = c + 1 if c + 1 < inp["C"] else c - 1
        assert invstd[n] != invstd[c]
        invstd = invstd.clone(); invstd[c] = invstd[n]
    y = (x - mean) * (gamma * invstd) + beta
    if inp["res"] is not None:
        y = y + inp["res"].to(prec)
    return y.clamp_min(0) if inp["relu"] else y


def backward(inp, mean, invstd, mask, prec=torch.float64, N=None, train=True, fault=None, at=(0, 0)):
    """dy, dres, dgamma, dbeta from the handed statistics and mask (bool [R, C] or None); N: the sample count behind the statistics (default: the rows of `inp`)"""
    r, c = at
    x, gamma, dout, mean, invstd = (t.to(prec) for t in (inp["x"], inp["gamma"], inp["dout"], mean, invstd))
    N = float(inp["R"] if N is None else N)
    g = dout if mask is None else torch.where(mask, dout, torch.zeros_like(dout))          # (+0 where masked, whatever dout's sign: dres is compared bit for bit)
    xh = (x - mean) * invstd
    pb, pg = g.clone(), g * xh
    if fault in ("dbeta_row_missing", "dgamma_row_missing") and mask is not None:          # (a masked row has nothing to miss: the last row up to `r` that has)
        live = torch.nonzero(mask[:r + 1, c])
        assert live.numel() > 0, ("no unmasked row up to", r, "in channel", c)
        r = int(live[-1])
    if fault == "dbeta_row_missing":
        pb[r, c] = 0
    if fault == "dgamma_row_missing":
        pg[r, c] = 0
    sb, sg = pb.sum(0), pg.sum(0)
    if train or fault == "batch_terms_in_eval_backward":
        dy = gamma * invstd / N * (N * g - sb - xh * sg)
    else:
        dy = gamma * invstd * g
    return {"dy": dy, "dres": g, "dgamma": sg, "dbeta": sb}


def evaluate(inp, prec=torch.float64, *, given=None, fault=None, at=None, train=True, N=None, local_rows=None, out16=torch.bfloat16):
    """The whole chain in `prec`: statistics; y (and y16 = its 16-bit store) and the backward from `given` = {"mean", "invstd" f32 [C], "stored" 16-bit [R, C] | None}, or
    from this evaluation's own statistics rounded to fp32 and its own y16.  `fault` (one of FAULTS) is applied where it arises, at (row, column) `at`."""
    assert fault is None or fault in FAULTS
    at = default_at(inp) if at is None else at
    out = statistics(inp, prec, fault, at, train)
    mean, invstd = (given["mean"], given["invstd"]) if given is not None else (out["mean"].float(), out["invstd"].float())
    out["y"] = apply(inp, mean, invstd, prec, fault, at)
    store = truncate16 if fault == "truncated_store" else rne16
    out["y16"] = store(out["y"].float(), out16)
    mask = None
    if inp["relu"]:
        stored = given["stored"] if given is not None and given.get("stored") is not None else out["y16"]
        mask = (out["y"].float() > 0) if fault == "mask_from_unrounded" else (stored.float() > 0)
    if fault == "local_count_under_sync":
        assert local_rows is not None and local_rows != (inp["R"] if N is None else N)
        N = local_rows
    out.update(backward(inp, mean, invstd, mask, prec, N, train, fault, at))
    out["dy16"] = store(out["dy"].float(), out16)
    out["given"] = {"mean": mean, "invstd": invstd, "stored": out["y16"] if inp["relu"] else None}
    return out


def reference64(inp, given, train=True, N=None):
    """float64 of everything (statistics included) with the handed f32 mean / invstd / stored output, and one scale per element"""
    ref = evaluate(inp, torch.float64, given=given, train=train, N=N)
    x, gamma, beta, dout = (inp[k].double() for k in ("x", "gamma", "beta", "dout"))
    R, m = inp["R"], inp["momentum"]
    mean, invstd = given["mean"].double(), given["invstd"].double()
    ref["s_mean"] = x.abs().mean(0) if train else inp["rmean"].double().abs()
    ref["s_invstd"] = ref["invstd"]
    ref["s_rmean"] = (1 - m) * inp["rmean"].double().abs() + m * ref["s_mean"]
    ref["s_rvar"] = (1 - m) * inp["rvar"].double().abs() + m * (ref["var"] + inp["eps"]) * (R / (R - 1.0) if R > 1 else 1.0)
    ref["s_y"] = (gamma * (x - mean)).abs() * invstd + beta.abs() + (inp["res"].double().abs() if inp["res"] is not None else 0)
    g = ref["dres"].abs()
    xh = ((x - mean) * invstd).abs()
    ref["s_dbeta"], ref["s_dgamma"] = g.sum(0), (g * xh).sum(0)
    n = float(R if N is None else N)
    ref["s_dy"] = gamma.abs() * invstd / n * (n * g + ref["s_dbeta"] + xh * ref["s_dgamma"]) if train else gamma.abs() * invstd * g
    return ref


def bounds(inp, ref, given, train=True, N=None):
    """-> ({kind: B}, {kind: E32}): B = max(FACTOR x E32, FLOOR), E32 from torch's float32 evaluation with the same handed statistics"""
    f32 = evaluate(inp, torch.float32, given=given, train=train, N=N)
    e32 = {k: worst(scaled(f32[k], ref[k], ref["s_" + k]))[0] for k in STATS + ("y",) + BACKWARD}
    assert all(math.isfinite(v) for v in e32.values()), ("the float32 oracle is not finite: the bound would be vacuous", e32)
    return {k: max(FACTOR * v, FLOOR) for k, v in e32.items()}, e32


# ---------------------------------------------------------------------------------------------------------------- checks
def check(kind, got, ref64, s, B, e32, what=""):
    """assert |got - ref64| <= B s element-wise; prints the worst scaled error, E32 and error / bound; -> error / bound"""
    assert got.shape == ref64.shape, (what, kind, got.shape, ref64.shape)
    e, at = worst(scaled(got, ref64, s + torch.zeros_like(ref64)))
    print(f"bn {what} {kind}: worst scaled error {e:.3e} at {at}, E32 {e32:.3e}, bound {B:.3e}, error / bound {e / B:.3f}")
    assert e <= B, (what, kind, "element", at, "scaled error", e, "bound", B, "error / bound", e / B)
    return e / B


def check_statistics(got, ref, B, e32, what="", train=True):
    """save_mean, save_invstd and (train) the updated running statistics; eval mode: save_mean is the running mean itself and the running statistics are untouched"""
    worst = {}
    if not train:
        for k in ("mean", "rmean", "rvar"):
            if got.get(k) is not None:
                gemmbound.check_exact(got[k].detach().cpu(), ref[k].float(), f"{what} {k} (eval mode)")
    for k in (STATS if train else ("invstd",)):
        if got.get(k) is not None:
            worst[k] = check(k, got[k], ref[k], ref["s_" + k], B[k], e32[k], what)
    return worst


def check_forward(got, ref, B, e32, what=""):
    """y f32 against the bound and y16 = RNE16(y) bit for bit; without y: y16 by the half-ulp rule against float64"""
    worst = {}
    if got.get("y") is not None:
        worst["y"] = check("y", got["y"], ref["y"], ref["s_y"], B["y"], e32["y"], what)
        if got.get("y16") is not None:
            gemmbound.check_exact(got["y16"].detach().cpu(), rne16(got["y"].detach().cpu(), got["y16"].dtype), what + " y16 = RNE16(y)")
    elif got.get("y16") is not None:
        worst["y16"] = gemmbound.check_half_ulp(got["y16"], ref["y"], B["y"] * ref["s_y"], what + " y16")
    return worst


def check_backward(got, ref, B, e32, what="", rows_of=None):
    """dgamma, dbeta f32, dres = g exactly, dy f32 (vdk_bn_rows_bwd, bn1d) against the bound or dy16 by the half-ulp rule.  `rows_of`: the slice of the reference's rows that
    `got` holds (one rank of a SyncBatchNorm batch: dy and dres only -- dgamma / dbeta are local sums and are checked against the local reference)"""
    sl = slice(None) if rows_of is None else rows_of
    worst = {}
    for k in ("dgamma", "dbeta"):
        if got.get(k) is not None:
            worst[k] = check(k, got[k], ref[k], ref["s_" + k], B[k], e32[k], what)
    if got.get("dres") is not None:
        gemmbound.check_exact(got["dres"].detach().cpu(), ref["dres"][sl].float(), what + " dres = masked dout")
    if got.get("dy") is not None:
        worst["dy"] = check("dy", got["dy"], ref["dy"][sl], ref["s_dy"][sl], B["dy"], e32["dy"], what)
    if got.get("dy16") is not None:
        worst["dy16"] = gemmbound.check_half_ulp(got["dy16"], ref["dy"][sl], B["dy"] * ref["s_dy"][sl], what + " dy16")
    return worst


def check_all(got, ref, B, e32, what="", train=True):
    return {**check_statistics(got, ref, B, e32, what, train), **check_forward(got, ref, B, e32, what), **check_backward(got, ref, B, e32, what)}


def check_dead(got, inp, what=""):
    """the dead channel's equalities: mean = 0, invstd = fp32 eps^-1/2, y = beta + res [relu] in fp32 arithmetic, dgamma = 0"""
    assert inp["dead"]
    c = DEAD
    if got.get("mean") is not None:
        assert float(got["mean"][c]) == 0.0, (what, "dead channel mean", float(got["mean"][c]))
    if got.get("invstd") is not None:
        want = float(1.0 / torch.sqrt(torch.tensor(inp["eps"], dtype=torch.float32)))
        assert float(got["invstd"][c]) == want, (what, "dead channel invstd", float(got["invstd"][c]), want)
    y = inp["beta"][c] + (inp["res"][:, c].float() if inp["res"] is not None else torch.zeros(inp["R"]))
    y = y.clamp_min(0) if inp["relu"] else y
    if got.get("y") is not None:
        assert torch.equal(got["y"][:, c].cpu(), y), (what, "dead channel y")
    if got.get("y16") is not None:
        assert torch.equal(got["y16"][:, c].cpu(), y.to(got["y16"].dtype)), (what, "dead channel y16")
    if got.get("dgamma") is not None:
        assert float(got["dgamma"][c]) == 0.0, (what, "dead channel dgamma", float(got["dgamma"][c]))


# ---------------------------------------------------------------------------------------------------------------- preconditions
def _moved(bad, ref, kind):
    return scaled(bad[kind], ref[kind], ref["s_" + kind] + torch.zeros_like(ref[kind]))


def assert_sensitive(inp, ref, B, given, faults=FAULTS, *, train=True, N=None, local_rows=None, out16=torch.bfloat16, at=None, what=""):
    """From float64 alone: each fault of `faults` that the case can show, planted at `at` in float64 with the same handed statistics, moves (one of) its element(s) by
    >= SIGNAL_FACTOR x B S; a truncated store leaves >= 10 % of the 16-bit elements beyond the half-ulp rule's allowance by that factor of the slack.  -> the faults shown"""
    shown = []
    for name in faults:
        if not applicable(name, inp, train, local_rows, out16):
            continue
        if name == "truncated_store":
            frac = []          # (dy cancels to nothing at R = 2, a ReLU leaves half of y at zero: one of the two copies has to show it)
            for k in ("y", "dy"):
                t = truncate16(ref[k].float(), out16).double()
                beyond = (t - ref[k]).abs() >= gemmbound.half_ulp_distance(ref[k], out16) + SIGNAL_FACTOR * B[k] * ref["s_" + k]
                frac.append(float(beyond.double().mean()))
            assert max(frac) >= 0.1, (what, name, frac)
        else:
            bad = evaluate(inp, torch.float64, given=given, fault=name, at=at, train=train, N=N, local_rows=local_rows, out16=out16)
            sig = max(float(_moved(bad, ref, k).max()) / B[k] for k in KINDS_OF[name])
            assert sig >= SIGNAL_FACTOR, (what, name, "signal / bound", sig)
        shown.append(name)
    return shown


def applicable(name, inp, train=True, local_rows=None, out16=torch.bfloat16):
    """whether the case can show the fault at all"""
    if name == "raw_moment_variance":
        return train and inp["far"]
    if name in ("stats_row_missing", "running_var_biased"):
        return train and inp["R"] > 1
    if name == "mask_from_unrounded":
        return train and inp["relu"] and inp["dead"] and out16 == torch.float16 and inp["res"] is not None and inp["res"].dtype == torch.float32
    if name == "local_count_under_sync":
        return train and local_rows is not None
    if name == "batch_terms_in_eval_backward":
        return not train
    if name in ("dbeta_row_missing", "dgamma_row_missing"):
        return inp["R"] > 1
    return True


def plant(name, inp, given=None, **kw):
    """a float32-evaluated result with the fault `name` applied (dict as `evaluate`)"""
    return evaluate(inp, torch.float32, given=given, fault=name, **kw)
