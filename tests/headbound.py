"""TEST INFRASTRUCTURE: element, column and row bounds for the margin-softmax heads (tests/test_head_entries.py, tests/test_head_columns.py; tested on itself by
tests/test_headbound.py).  The counterpart of tests/rowbound.py for csrc/margin_head.hip, csrc/vdk_margin.h and the E_MSTAT / E_MGRAD epilogues.

A whole-tensor norm over Gaussian features hides one wrong class column (1 / sqrt(C) of |dW|, 1 / C of a row's probability), and a comparison of one form of the head
with another cancels whatever the shared margin functions get wrong.  This module supplies

  * a restatement of the four heads written from the reference's modules (models/faceX/head/{arcface,circleloss,mv_softmax,magface}.py) followed by the label-smoothed
    cross-entropy, generic over the torch dtype: float64 is the reference, float32 the oracle (`margin_terms`, `head_rows`, `head_e2e`); it reproduces
    tests/golden/heads.npz and magface.npz, the reference modules' own outputs (asserted in tests/test_headbound.py), which is what ties it to the reference and not
    to the kernels;
  * inputs whose tile, pass, load and tail edges carry O(1) probability: `planted_cos` (a float32 cosine matrix for the entry-level tests: every edge column of
    `edges` is the target of one row and the hard negative of another, plus cosines outside [-1, 1], on both sides of MV-Softmax's threshold, below CircleLoss's -m
    and an ArcFace target in the fallback branch, none within GUARD of a branch threshold) and `planted_head` (weight, features and labels for the end-to-end tests,
    chained: column y_k has cosine c_t with row k and c_n with row k - 1);
  * scales built from absolute values: per entry of dcos s = gscale (p + eps / C + (1 - eps) [target]) |jac|, per dW column and dfeats row the same products of
    absolute values carried through the backward of both normalisations;
  * bounds: FACTOR x the oracle's worst scaled error (float32 torch with f^, W^ and dcos rounded to the case's 16-bit format), computed on the same inputs inside the
    test; fp32 outputs against LSE_FACTOR x max(the error of the float32 evaluation, eps32 x sum |terms|);
  * the preconditions (`assert_sensitive`) and the planted faults (`plant`).  FACTOR, SIGNAL_FACTOR and LSE_FACTOR are rowbound.py's."""
from __future__ import annotations

import math
from types import SimpleNamespace as NS

import torch

from tests.rowbound import FACTOR, LSE_FACTOR, SIGNAL_FACTOR, worst

GUARD = 1e-5            # no planted cosine lies this close to a branch threshold: a float32 and a float64 evaluation take the same branch
EPS32 = torch.finfo(torch.float32).eps
MODES = ("arcface", "circle", "mv_am", "mv_arc")
MAG = dict(l_a=10.0, u_a=110.0, l_margin=0.45, u_margin=0.8, lamda=20.0)      # magface.py's defaults


def head(mode, **kw):
    """the parameters of one head: s (scale or gamma), m (margin), m_am (arcface), t (mv_weight), row_margin (float32 [B] or None: MagFace's per-row margin).
    CircleLoss: gamma = 256, the reference's default -- with gamma = 64 the target's logit is at most 64 * 0.25 * 0.25 = 4, below the log-sum of 5003 ordinary columns,
    and no target could hold 10 % of its row"""
    d = {"arcface": dict(s=32.0, m=0.35, m_am=0.1, t=0.0), "circle": dict(s=256.0, m=0.25, m_am=0.0, t=0.0),
         "mv_am": dict(s=32.0, m=0.35, m_am=0.0, t=1.12), "mv_arc": dict(s=32.0, m=0.35, m_am=0.0, t=1.12)}[mode]
    d.update(kw)
    return NS(mode=mode, row_margin=d.pop("row_margin", None), **d)


# ---------------------------------------------------------------------------------------------------------------- the heads, from the reference's modules
def margin_terms(h, cos, labels, dtype=torch.float64):
    """-> (logit, jac = d logit / d cos, labs = the logit's terms in absolute value), each [B, C] in `dtype`, of the raw cosines `cos`.
    arcface.py:20-36 / magface.py:26-47: clamp to [-1, 1] (gradient 1 on the closed interval), the target becomes cos(theta + m) where cos > cos(pi - m), else cos - m_am.
    circleloss.py:21-43: clamp; alpha_p = max(1 + m - cos, 0), alpha_n = max(cos + m, 0), both detached; logits alpha_p (cos - (1 - m)) | alpha_n (cos - m).
    mv_softmax.py:25-44: no clamp; gt = the target's cosine; AM: mask cos > gt - m, target gt - m if gt > m else gt; arc: mask cos > cos(theta_gt + m), target that if gt > 0
    else gt; masked entries t cos + t - 1.  The margin is evaluated on the gathered target entries only."""
    c_raw = cos.to(dtype)
    B, C = c_raw.shape
    rows = torch.arange(B)
    s = h.s
    if h.mode in ("arcface", "circle"):
        c = c_raw.clamp(-1.0, 1.0)
        cg = ((c_raw >= -1.0) & (c_raw <= 1.0)).to(dtype)
        ct, cgt = c[rows, labels], cg[rows, labels]
    if h.mode == "arcface":
        m = (h.row_margin.to(dtype) if h.row_margin is not None else torch.full((B,), h.m, dtype=dtype))
        sn = torch.sqrt(1.0 - ct * ct)
        act = ct > torch.cos(math.pi - m)
        lt = torch.where(act, ct * torch.cos(m) - sn * torch.sin(m), ct - h.m_am)
        jt = torch.where(act, torch.cos(m) + ct / sn * torch.sin(m), torch.ones_like(ct)) * cgt
        at = torch.where(act, ct.abs() * torch.cos(m) + sn * torch.sin(m), ct.abs() + h.m_am)
        logit, jac, labs = s * c, s * cg, s * c.abs()
    elif h.mode == "circle":
        ap, an = (1.0 + h.m - ct).clamp_min(0.0), (c + h.m).clamp_min(0.0)
        lt, jt, at = ap * (ct - (1.0 - h.m)), ap * cgt, (ap > 0) * (1.0 + h.m + ct.abs()) * (ct.abs() + (1.0 - h.m))
        logit, jac, labs = s * an * (c - h.m), s * an * cg, s * (an > 0) * (c.abs() + h.m) ** 2
    else:
        gt = c_raw[rows, labels]
        if h.mode == "mv_am":
            thr = gt - h.m
            lt = torch.where(gt > h.m, gt - h.m, gt)
            jt = torch.ones_like(gt)
            at = torch.where(gt > h.m, gt.abs() + h.m, gt.abs())
        else:
            sn = torch.sqrt(1.0 - gt * gt)
            thr = gt * math.cos(h.m) - sn * math.sin(h.m)
            lt = torch.where(gt > 0.0, thr, gt)
            jt = torch.where(gt > 0.0, math.cos(h.m) + gt / sn * math.sin(h.m), torch.ones_like(gt))
            at = torch.where(gt > 0.0, gt.abs() * math.cos(h.m) + sn * math.sin(h.m), gt.abs())
        hard = c_raw > thr[:, None]
        logit = s * torch.where(hard, h.t * c_raw + h.t - 1.0, c_raw)
        jac = s * torch.where(hard, torch.full_like(c_raw, h.t), torch.ones_like(c_raw))
        labs = s * torch.where(hard, h.t * c_raw.abs() + abs(h.t - 1.0), c_raw.abs())
    logit, jac, labs = logit.clone(), jac.clone(), labs.clone()
    logit[rows, labels], jac[rows, labels], labs[rows, labels] = s * lt, s * jt, s * at
    return logit, jac, labs


def head_rows(h, cos, labels, eps=0.0, gscale=1.0, C_total=None, dtype=torch.float64):
    """the head followed by torch's CrossEntropyLoss(label_smoothing=eps) on WHOLE rows [B, C] (C_total: another class count in the smoothing term, for the planted fault).
    -> NS: logit, jac, labs, mx, se = sum exp(logit - mx), sm = sum logit, lt = the target's logit, lse, loss, p, dcos = gscale (p - eps / C_total - (1 - eps) [target]) jac,
    s_dcos (the same with every factor's absolute value), s_loss (|terms| of a loss row)"""
    logit, jac, labs = margin_terms(h, cos, labels, dtype)
    B, C = logit.shape
    Ct = C if C_total is None else C_total
    rows = torch.arange(B)
    mx = logit.max(1).values
    se = torch.exp(logit - mx[:, None]).sum(1)
    lse = mx + torch.log(se)
    p = torch.exp(logit - lse[:, None])
    sm, lt = logit.sum(1), logit[rows, labels]
    hot = torch.zeros_like(logit)
    hot[rows, labels] = 1.0
    loss = lse - (1.0 - eps) * lt - eps * sm / Ct
    return NS(logit=logit, jac=jac, labs=labs, mx=mx, se=se, sm=sm, lt=lt, lse=lse, loss=loss, p=p, hot=hot,
              dcos=gscale * (p - eps / Ct - (1.0 - eps) * hot) * jac, s_dcos=gscale * (p + eps / Ct + (1.0 - eps) * hot) * jac.abs(),
              s_loss=mx.abs() + torch.log(se).abs() + (1.0 - eps) * labs[rows, labels] + eps * labs.sum(1) / Ct)


def rnd(t, fmt):
    return t if fmt is None else t.to(fmt).to(t.dtype)


def norm_backward(x, inv, g, dim):
    """backward of x -> x^ = x inv along `dim` (F.normalize): inv (g - x^ <x^, g>)"""
    return inv * (g - x * (x * g).sum(dim, keepdim=True))


def head_e2e(h, feats, weight, labels, eps=0.0, gscale=None, dtype=torch.float64, fmt=None, cos_fmt=None, mag=None, lscale=1.0):
    """features [B, D], weight [D, C] -> loss rows, dfeats, dweight of mean CE (gscale: 1 / B), in `dtype`.  fmt (torch.bfloat16 | torch.float16 | None) makes it the
    ORACLE: dcos, and f^ and W^ where they enter the two gradient products, rounded to the format.  cos_fmt: the cosines are those of f^ and W^ rounded to that format
    (cos_planes = 1, torch.mm under the reference's autocast) -- part of the operation's definition, so the float64 reference takes it too (rounded from the float32
    normalisation: at s = 32 the 4e-3 cosine error of bf16 operands is a 10 % error of p, a floor no kernel can be below); None: the split-plane cosines, fp32-class.  mag (dict of magface.py's constants): the margin is the row's magnitude-aware one, and the gradient includes the margin's
    own path and the regulariser lamda (x / u_a^2 + 1 / x), x = clamp(|f|, l_a, u_a), averaged over the rows.
    -> NS: r (head_rows), fh, wh, finv, winv, dfeats, dweight, s_dfeats [B], s_dweight [C]"""
    f, w = feats.to(dtype), weight.to(dtype)
    B = f.shape[0]
    gs = 1.0 / B if gscale is None else gscale
    fn, wn = f.norm(dim=1, keepdim=True), w.norm(dim=0, keepdim=True)
    finv, winv = 1.0 / fn.clamp_min(1e-12), 1.0 / wn.clamp_min(1e-12)
    fh, wh = f * finv, w * winv
    f16, w16 = rnd(fh, fmt), rnd(wh, fmt)
    cos = fh @ wh if cos_fmt is None else rnd(fh.float(), cos_fmt).to(dtype) @ rnd(wh.float(), cos_fmt).to(dtype)
    if mag is not None:
        x = fn[:, 0].clamp(mag["l_a"], mag["u_a"])
        k = (mag["u_margin"] - mag["l_margin"]) / (mag["u_a"] - mag["l_a"])
        h = NS(**{**vars(h), "row_margin": k * (x - mag["l_a"]) + mag["l_margin"]})
    r = head_rows(h, cos, labels, eps, gs, None, dtype)
    d16 = rnd(r.dcos * lscale, fmt) / lscale          # (the loss scale, a power of two, only moves the 16-bit rounding)
    dfh, dwh = d16 @ w16.T, f16.T @ d16
    afh, awh = r.s_dcos @ wh.abs().T, fh.abs().T @ r.s_dcos
    if mag is not None:
        # d logit_t / d m = -s sin(theta + m) where the margin branch is active; dm / df = k f^ and dx / df = f^ inside (l_a, u_a)
        rows = torch.arange(B)
        m = h.row_margin
        ct = cos[rows, labels].clamp(-1.0, 1.0)
        act = (ct > torch.cos(math.pi - m)).to(dtype)
        dlt = gs * (r.p[rows, labels] - eps / cos.shape[1] - (1.0 - eps))
        inside = ((fn[:, 0] > mag["l_a"]) & (fn[:, 0] < mag["u_a"])).to(dtype)
        t1 = dlt * (-h.s) * (torch.sqrt(1.0 - ct * ct) * torch.cos(m) + ct * torch.sin(m)) * act * k
        t2 = mag["lamda"] / B * (1.0 / mag["u_a"] ** 2 - 1.0 / (x * x))
        extra, aextra = ((t1 + t2) * inside)[:, None] * fh, ((t1.abs() + abs(mag["lamda"] / B) * (1.0 / mag["u_a"] ** 2 + 1.0 / (x * x))) * inside)[:, None] * fh.abs()
    else:
        extra = aextra = torch.zeros_like(fh)
    return NS(r=r, cos=cos, fh=fh, wh=wh, finv=finv, winv=winv, h=h, d16=d16,
              dfeats=norm_backward(fh, finv, dfh, 1) + extra, dweight=norm_backward(wh, winv, dwh, 0),
              s_dfeats=((finv * (afh + fh.abs() * (fh.abs() * afh).sum(1, keepdim=True))) + aextra).norm(dim=1),
              s_dweight=(winv * (awh + wh.abs() * (wh.abs() * awh).sum(0, keepdim=True))).norm(dim=0))


# ---------------------------------------------------------------------------------------------------------------- inputs
def edges(C, extra=()):
    """the class columns at which the kernels change hands: the first two; both sides of a 64-column epilogue slice, of a 256-thread stride, of a 1024-column load, of a
    4096-column pass and of the pass's second load; both sides of the scalar tail's start C & ~3; the last column; and `extra` (shard splits) with both neighbours"""
    C4 = C & ~3
    e = {0, 1, 63, 64, 255, 256, 1023, 1024, 4095, 4096, 5119, 5120, C4 - 1, C4, C - 1}
    for x in extra:
        e |= {x - 1, x, x + 1}
    return sorted(x for x in e if 0 <= x < C)


def _target_and_negative(h, c_t, share=1.0):
    """the hard negative's cosine at which its logit lies ln(share) below that of a target at cosine c_t (bisection on the float64 head; MV-Softmax: below the row's
    threshold, where the logit is continuous)"""
    if h.row_margin is not None:                            # per-row margins: the mean margin places the negative
        h = NS(**{**vars(h), "m": float(h.row_margin.double().mean()), "row_margin": None})
    lab = torch.tensor([0])
    want = float(margin_terms(h, torch.tensor([[c_t, 0.0]], dtype=torch.float64), lab)[0][0, 0]) - math.log(share)
    lo, hi = 0.0, c_t
    if h.mode in ("mv_am", "mv_arc"):
        hi = (c_t - h.m if h.mode == "mv_am" else math.cos(math.acos(c_t) + h.m)) - 1e-3
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lg = float(margin_terms(h, torch.tensor([[c_t, mid]], dtype=torch.float64), lab)[0][0, 1])
        lo, hi = (mid, hi) if lg < want else (lo, mid)
    return 0.5 * (lo + hi)


C_T = {"arcface": 0.8, "circle": 0.9, "mv_am": 0.8, "mv_arc": 0.8}
BULK = {"arcface": 0.3, "circle": 0.2, "mv_am": 0.3, "mv_arc": 0.3}      # the bulk is N(0, 1 / D) cut off here: below every planted value and every MV threshold


# planted_head: the ordinary columns' component inside the features' span is multiplied by this.  CircleLoss's negative logit gamma (c^2 - m^2) grows with c^2 and the
# target's is at most gamma / 16: at D = 128 the largest of 10^5 ordinary cosines (4.5 sigma = 0.4) would outweigh every target, whatever gamma is
SHRINK = {"arcface": 1.0, "circle": 0.5, "mv_am": 1.0, "mv_arc": 1.0}


def thresholds(h, cos64, labels):
    """per row, the cosines at which a non-target entry changes branch, [B, n] float64"""
    B = cos64.shape[0]
    gt = cos64[torch.arange(B), labels]
    if h.mode == "mv_am":
        return (gt - h.m)[:, None]
    if h.mode == "mv_arc":
        return (gt * math.cos(h.m) - torch.sqrt(1.0 - gt * gt) * math.sin(h.m))[:, None]
    t = [-1.0, 1.0] + ([-h.m] if h.mode == "circle" else [])
    return torch.tensor(t, dtype=torch.float64).expand(B, len(t))


def assert_guard(h, cos, labels, band=GUARD):
    """from float64: no non-target entry within `band` of a branch threshold of its row; targets >= 1e-3 inside (-1, 1) and `band` away from their own branch points
    (cos(pi - m) for ArcFace, m | 0 for MV-Softmax)"""
    c = cos.double()
    B = c.shape[0]
    rows = torch.arange(B)
    d = torch.stack([(c - t[:, None]).abs() for t in thresholds(h, c, labels).T]).min(0).values
    d[rows, labels] = 1.0
    assert float(d.min()) > band, ("entry on a branch threshold", h.mode, float(d.min()))
    gt = c[rows, labels]
    assert float((1.0 - gt.abs()).min()) >= 1e-3, ("target at the singularity of c / sqrt(1 - c^2)", float(gt.abs().max()))
    if h.mode == "arcface":
        m = h.row_margin.double() if h.row_margin is not None else torch.full((B,), h.m, dtype=torch.float64)
        assert float((gt - torch.cos(math.pi - m)).abs().min()) > band
    elif h.mode in ("mv_am", "mv_arc"):
        assert float((gt - (h.m if h.mode == "mv_am" else 0.0)).abs().min()) > band


def planted_cos(B, C, mode, seed, D=128, extra=(), h=None):
    """-> NS(cos float32 [B, C], labels [B], edges, pairs = [(row, column)] of the planted targets and hard negatives, special = {what: (row, column)}).
    Row k's target is edge column E[k mod n], its hard negative E[(k + 1) mod n]: every edge column is a target and a hard negative (n + 3 <= B).  The three rows after
    the first n carry, on edge columns that are neither: a cosine above 1 and one below -1 (the clamp's zero jacobian; MV-Softmax does not clamp); for MV-Softmax one
    entry on either side of the row's threshold, for CircleLoss one below -m (alpha_n = 0); for ArcFace a target below cos(pi - m) (the fallback branch)."""
    h = head(mode) if h is None else h
    g = torch.Generator().manual_seed(seed)
    cos = (torch.randn(B, C, generator=g, dtype=torch.float64) * D ** -0.5).clamp(-BULK[mode], BULK[mode])
    E = edges(C, extra)
    n = len(E)
    assert n + 3 <= B, (n, B)
    c_t = C_T[mode]
    c_n = _target_and_negative(h, c_t)
    labels = torch.tensor([E[k % n] for k in range(B)])
    pairs, special = [], {}
    for k in range(B):
        neg = E[(k + 1) % n]
        cos[k, labels[k]], cos[k, neg] = c_t + 0.002 * (k % 5), c_n - 0.002 * (k % 3)
        pairs += [(k, int(labels[k])), (k, neg)]
    free = lambda k: [e for e in E if e not in (int(labels[k]), E[(k + 1) % n])]
    k = n
    a, b = free(k)[0], free(k)[-1]
    cos[k, a], cos[k, b] = 1.0 + 2e-5, -1.0 - 2e-5
    special["above_1"], special["below_-1"] = (k, a), (k, b)
    k = n + 1
    a, b = free(k)[1], free(k)[-2]
    if mode in ("mv_am", "mv_arc"):
        thr = float(thresholds(h, cos.float().double(), labels)[k, 0])
        cos[k, a], cos[k, b] = thr + 1e-3, thr - 1e-3
        special["above_thr"], special["below_thr"] = (k, a), (k, b)
    elif mode == "circle":
        cos[k, a] = -h.m - 0.05
        special["below_-m"] = (k, a)
    k = n + 2
    if mode == "arcface":
        cos[k, labels[k]] = -0.97                       # below cos(pi - m) for every m in [0.35, 0.8], 1e-3 and more inside -1
        special["fallback_target"] = (k, int(labels[k]))
    c32 = cos.float()
    # move what lies on a threshold (ordinary entries: CircleLoss's -m lies inside the bulk), then assert the band
    thr = thresholds(h, c32.double(), labels)
    for t in thr.T:
        close = (c32.double() - t[:, None]).abs() <= 2.0 * GUARD
        close[torch.arange(B), labels] = False
        c32 = torch.where(close, (t[:, None] + 4.0 * GUARD).float().expand_as(c32), c32)
    assert_guard(h, c32, labels)
    return NS(cos=c32, labels=labels, edges=E, pairs=pairs, special=special, h=h)


def planted_head(D, C, mode, seed, B=None, extra=(), h=None, fnorm=(0.5, 2.0), c_t=None):
    """-> NS(weight float32 [D, C], feats float32 [B, D], labels, edges, pairs).  Row k < n = len(edges) has target y_k = E[k]; column y_k is built in the span of
    f^_k, f^_{k-1} and a direction orthogonal to both so that its cosine is c_t with row k (its target) and c_n with row k - 1 (its hard negative), cyclically: n chained
    rows, then fillers with ordinary targets up to B.  Weight columns and feature rows carry norms in `fnorm` (both normalisations do work)."""
    h = head(mode) if h is None else h
    g = torch.Generator().manual_seed(seed)
    E = edges(C, extra)
    n = len(E)
    B = n if B is None else B
    assert B >= n
    f = torch.randn(B, D, generator=g, dtype=torch.float64)
    f[:n] = torch.linalg.qr(f[:n].T).Q.T                     # the chained rows orthonormal: (c_t, c_n) is reachable by a unit column whatever the seed
    fh = f / f.norm(dim=1, keepdim=True)
    w = torch.randn(D, C, generator=g, dtype=torch.float64)
    if SHRINK[mode] < 1.0:
        q = torch.linalg.qr(fh.T).Q                          # an orthonormal basis of the features' span
        w = w - (1.0 - SHRINK[mode]) * (q @ (q.T @ w))
    w = w / w.norm(dim=0, keepdim=True)
    c_t = C_T[mode] if c_t is None else c_t
    c_n = _target_and_negative(h, c_t)
    ordinary = [c for c in range(7, C, max(1, min(97, (C - 8) // (B - n + 2)))) if c not in E]
    labels = torch.tensor([E[k] if k < n else ordinary[k - n] for k in range(B)])
    pairs = []
    for k in range(n):                                      # column y_k: target of row k, hard negative of row k - 1 (of row n - 1 for k = 0)
        u, v = fh[k], fh[(k - 1) % n]
        guv = float(u @ v)
        al, be = torch.linalg.solve(torch.tensor([[1.0, guv], [guv, 1.0]], dtype=torch.float64), torch.tensor([c_t, c_n], dtype=torch.float64)).tolist()
        nrm = w[:, labels[k]] - (w[:, labels[k]] @ u) * u
        v_perp = v - guv * u
        nrm = nrm - (nrm @ v_perp) / (v_perp @ v_perp) * v_perp
        nrm = nrm / nrm.norm()
        w[:, labels[k]] = al * u + be * v + math.sqrt(1.0 - (al * al + be * be + 2.0 * al * be * guv)) * nrm
        pairs += [(k, int(labels[k])), ((k - 1) % n, int(labels[k]))]
    lo, hi = fnorm
    w = w * (0.5 + 1.5 * torch.rand(1, C, generator=g, dtype=torch.float64))
    f = fh * (lo + (hi - lo) * torch.rand(B, 1, generator=g, dtype=torch.float64))
    return NS(weight=w.float(), feats=f.float(), labels=labels, edges=E, pairs=pairs, h=h, chained=n)


# ---------------------------------------------------------------------------------------------------------------- errors, bounds, checks
def entry_errors(got, ref, scale):
    """|got - ref| / scale element by element; where the scale is zero (a zero jacobian) the entry must be exactly zero"""
    d = (got.double() - ref.double()).abs()
    return torch.where(scale > 0, d / scale.clamp_min(1e-300), torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, float("inf"))))


def col_errors(got, ref, scale):
    """dweight [D, C]: |got_j - ref_j|_2 / s_j per class column"""
    return (got.double() - ref.double()).norm(dim=0) / scale


def row_errors(got, ref, scale):
    """dfeats [B, D]: |got_b - ref_b|_2 / s_b per row"""
    return (got.double() - ref.double()).norm(dim=1) / scale


def bound16(e_oracle):
    """FACTOR x the oracle's worst scaled error"""
    return FACTOR * worst(e_oracle)[0]


def bound32(e_f32, floor=EPS32):
    """an fp32 output in units of its |terms|: LSE_FACTOR x max(the worst error of the float32 torch evaluation, eps32)"""
    return LSE_FACTOR * max(worst(e_f32)[0], floor)


def check(name, e, bound, factor=FACTOR, what=""):
    """assert max e <= bound; prints the worst error, the oracle's and their ratio; -> the ratio"""
    m, at = worst(e)
    e_or = bound / factor
    ratio = m / e_or if e_or > 0 else (0.0 if m == 0 else float("inf"))
    print(f"head {what} {name}: max e_kernel {m:.3e} at {at}, E_or {e_or:.3e}, ratio {ratio:.2f}")
    assert m <= bound, (what, name, at, m, "bound", bound)
    return ratio


def e2e_errors(got_df, got_dw, ref):
    return {"dfeats": row_errors(got_df, ref.dfeats, ref.s_dfeats), "dweight": col_errors(got_dw, ref.dweight, ref.s_dweight)}


def e2e_bounds(ref, orc):
    return {k: bound16(e) for k, e in e2e_errors(orc.dfeats, orc.dweight, ref).items()}


# ---------------------------------------------------------------------------------------------------------------- planted faults and their signal
def pair_signals(ref, pairs):
    """from float64: the scaled error of "column j's dW misses row b" and of "row b's dfeats ignores column j" for every planted pair -> (dW [n], dfeats [n])"""
    b = torch.tensor([p[0] for p in pairs]); j = torch.tensor([p[1] for p in pairs])
    d = ref.r.dcos[b, j]
    dw = norm_backward(ref.wh[:, j], ref.winv[:, j], d[None, :] * ref.fh[b].T, 0)
    df = norm_backward(ref.fh[b], ref.finv[b], d[:, None] * ref.wh[:, j].T, 1)
    return dw.norm(dim=0) / ref.s_dweight[j], df.norm(dim=1) / ref.s_dfeats[b]


def assert_sensitive(ref, pairs, bnd, what=""):
    """The preconditions, from float64 alone and without exception: every planted pair's fault stands SIGNAL_FACTOR x above the dW and the dfeats bound, and so does
    "column j comes back zero" for EVERY column (|dW_j| / s_j)."""
    sw, sf = pair_signals(ref, pairs)
    zero = ref.dweight.norm(dim=0) / ref.s_dweight
    print(f"head {what}: smallest fault signal / bound: dW pair {float(sw.min()) / bnd['dweight']:.1f}, dfeats pair {float(sf.min()) / bnd['dfeats']:.1f}, "
          f"zero column {float(zero.min()) / bnd['dweight']:.1f}")
    assert float(sw.min()) >= SIGNAL_FACTOR * bnd["dweight"], (what, "dW pair", float(sw.min()), bnd["dweight"])
    assert float(sf.min()) >= SIGNAL_FACTOR * bnd["dfeats"], (what, "dfeats pair", float(sf.min()), bnd["dfeats"])
    assert float(zero.min()) >= SIGNAL_FACTOR * bnd["dweight"], (what, "zero column", int(zero.argmin()), float(zero.min()), bnd["dweight"])


def assert_shares(ref, pairs, lo=0.1, hi=0.9):
    """every planted target and hard negative holds between 10 % and 90 % of its row, from float64"""
    p = ref.r.p[torch.tensor([q[0] for q in pairs]), torch.tensor([q[1] for q in pairs])]
    assert lo <= float(p.min()) and float(p.max()) <= hi, (float(p.min()), float(p.max()))


def plant(kind, dcos, C, col=None, row=None, other=None):
    """a copy of the d(loss)/d(cos) matrix `dcos` [B, >= C] with one fault:
       drop_col: column `col` comes back zero                shift_col: column `col` holds its right-hand (at C - 1: left-hand) neighbour's values
       zero_tail: the scalar tail C & ~3 .. C - 1 is zero    ignore_pair: entry (row, col) is zero (the row's hard negative ignored, a column missing one row)
       replace_row: row `row` is `other` (a row evaluated with the target in the neighbouring column, or with the shard's C in the smoothing term)"""
    out = dcos.clone()
    if kind == "drop_col":
        out[:, col] = 0
    elif kind == "shift_col":
        out[:, col] = dcos[:, col + 1 if col + 1 < C else col - 1]
    elif kind == "zero_tail":
        out[:, C & ~3:C] = 0
    elif kind == "ignore_pair":
        out[row, col] = 0
    elif kind == "replace_row":
        out[row] = other.to(out.dtype)
    else:
        raise KeyError(kind)
    return out


def backward_from_dcos(ref32, dcos16):
    """what the two gradient products and both normalisation backwards make of a (faulty) 16-bit dcos, with the oracle's operands (an NS of head_e2e with fmt set)"""
    fmt = dcos16.dtype
    d = dcos16.to(ref32.fh.dtype)
    return norm_backward(ref32.fh, ref32.finv, d @ rnd(ref32.wh, fmt).T, 1), norm_backward(ref32.wh, ref32.winv, rnd(ref32.fh, fmt).T @ d, 0)
