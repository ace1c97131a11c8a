"""TEST INFRASTRUCTURE: per-element bounds for the LayerNorm kernels of csrc/norm_loss.hip (tests/test_layernorm_forms.py; tested on itself by tests/test_lnbound.py).
The counterpart of tests/rowbound.py, tests/headbound.py and tests/gemmbound.py for the row kernels.

A whole-tensor norm over Gaussian data cannot see one column missing from one row's mean, one row missing from a bias gradient or a stochastic-depth factor taken from the
neighbouring sample (tests/test_lnbound.py shows the first two passing the 2e-6 of tests/test_rowops.py).  Everything here is float64 of the kernel's OWN inputs -- the f32
mean and rstd it is handed included, so the forward's error is no part of the backward's check:

  xh = (x - mean) rstd,  g = s dy gamma  (s = dy_scale or 1)
  dx = rstd (g - mean_c g - xh mean_c(g xh)) + dres         S_dx     = rstd (|g| + mean_c |g| + |xh| mean_c |g xh|) + |dres|
  dgamma = sum_r s dy xh                                     S_dgamma = sum_r |s dy xh|
  dbeta  = sum_r s dy                                        S_dbeta  = sum_r |s dy|

and |got - ref64| <= B S per element with B = max(FACTOR x E32, FLOOR): E32 = the worst scaled error of a float32 torch evaluation of the same formulas on the same inputs
(`evaluate(inp, torch.float32)`), never taken from a kernel; FACTOR = rowbound.FACTOR (another correct summation order); FLOOR = 16 x 2^-24, the roundings of one element's
own chain (x - mu, . rstd, dy . gamma, two means / C, -, ., -, . rstd, + dres and the reduction tail): torch's pairwise sums can be luckier than any kernel's order.

The 16-bit copy dxb is RNE16(dx f) of the kernel's own fp32 dx bit for bit (f = dxb_rs[row // dxb_rps] multiplied in fp32, or nothing), or obeys gemmbound's half-ulp rule
against float64 with B S as the slack where dx is not returned.  The column sums are sums of the kernel's own STORED dxb ("the producer sums what it stores"), same form of
bound with S = sum_r |dxb|.

`assert_sensitive` holds the preconditions that keep this from being vacuous (from float64 alone: every fault of the list moves its element by >= SIGNAL_FACTOR x B S),
`evaluate(..., fault=...)` / `plant` the faults of the self-test.  The forward (`forward64`, `check_forward`) follows the same pattern."""
from __future__ import annotations

import torch

from tests import gemmbound
from tests.rowbound import FACTOR, SIGNAL_FACTOR

U32 = 2.0 ** -24
FLOOR = 16 * U32
DY_SCALE = 2.0 ** -6
BLOCK_ROWS = 16                      # most rows of a workgroup of ln_bwd_kernel until T passes 16 x 1024 (ln_bwd_blocks evens them out: T = 19 is 10 + 9); where `plant` puts a row fault
WIDTHS = (8, 100, 128, 132, 256, 260, 512, 516, 768, 772, 1024, 1028, 4096)      # both sides of every routing edge of ln_bwd_impl, a partly filled slab, the sixteenth slab
T_RAGGED = 19                        # two blocks (10 + 9 rows) with ragged last passes, an odd row count for the half-wave form
SMALL = tuple((T, C) for C in (8, 128, 260, 772) for T in (1, 2, 3))
TALL = ((16392, 8), (16392, 128))    # 17 rows per block: a half-wave's second pass holds one row, and its odd half the next block's row
FAULTS = ("mean_column_dropped", "neighbour_rstd", "dgamma_row_missing", "dbeta_row_missing", "colsum_row_missing", "colsum_before_scale", "truncated_store",
          "row_scale_neighbour")


# ---------------------------------------------------------------------------------------------------------------- inputs
def _signed(shape, g):
    """random signs, magnitudes in [0.5, 1.5): no contribution is close to zero"""
    return (torch.rand(shape, generator=g, dtype=torch.float64) + 0.5) * (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)


def inputs(T, C, dy_dtype, seed, *, dres=True, dres16=False, dy_scale=False, rps=0, far_rows=False):
    """-> dict: x f32 [T, C] = 2 N(0, 1) + 0.5, gamma f32 [C] and dy [T, C] in `dy_dtype` (rounded to it) with random signs and magnitudes in [0.5, 1.5), dres f32 N(0, 1)
    (or None; `dres16`: rounded to fp16 and handed over as fp16), mean and rstd f32 [T] (float64 statistics of x at eps = 1e-6, rounded once), beta f32 [C], dy_scale
    (2^-6 or None), rs f32 [ceil(T / rps)] from {0, 1, 1.25} with neighbours different (or None) and rps.  `far_rows`: every third row has its mean at 100 x its standard
    deviation (the forward's two-pass variance against E[x^2] - E[x]^2)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, C, generator=g, dtype=torch.float64) * 2 + 0.5
    if far_rows:
        x[::3] = (x[::3] - 0.5) + 200.0          # sigma = 2
    x = x.float()
    gamma = _signed((C,), g).float()
    beta = torch.randn(C, generator=g, dtype=torch.float64).float()
    dy = _signed((T, C), g).float().to(dy_dtype)
    dr = torch.randn(T, C, generator=g, dtype=torch.float64).float() if (dres or dres16) else None
    if dres16:
        dr = dr.half()
    x64 = x.double()
    mean = x64.mean(1)
    rstd = 1.0 / torch.sqrt(((x64 - mean[:, None]) ** 2).mean(1) + 1e-6)
    rs = gemmbound.exact_row_scale((T + rps - 1) // rps, seed) if rps else None
    return {"x": x, "gamma": gamma, "beta": beta, "dy": dy, "dres": dr, "mean": mean.float(), "rstd": rstd.float(), "dy_scale": DY_SCALE if dy_scale else None,
            "rs": rs, "rps": rps, "T": T, "C": C}


def rne16(v32, dtype):
    """the single round-to-nearest-even of an fp32 tensor into a 16-bit format"""
    assert v32.dtype == torch.float32 and dtype in (torch.bfloat16, torch.float16)
    return v32.to(dtype)


def truncate16(v32, dtype):
    """round toward zero into a 16-bit format: the nearest value, stepped one towards zero where it rounded away"""
    t = v32.to(dtype)
    away = t.float().abs() > v32.abs()
    return torch.where(away, (t.view(torch.int16) - 1).view(dtype), t)


def row_factor(inp, prec=torch.float32, neighbour_of=None):
    """[T] factor of the 16-bit copy per row (ones without dxb_rs); `neighbour_of` = a row: its whole sample takes the factor of the sample before"""
    T = inp["T"]
    if inp["rs"] is None:
        assert neighbour_of is None
        return torch.ones(T, dtype=prec)
    idx = torch.arange(T) // inp["rps"]
    if neighbour_of is not None:
        s = int(idx[neighbour_of])
        assert s >= 1 and inp["rs"][s] != inp["rs"][s - 1]
        idx[idx == s] = s - 1
    return inp["rs"].to(prec)[idx]


# ---------------------------------------------------------------------------------------------------------------- the formulas, in any precision, with an optional fault
def evaluate(inp, prec=torch.float64, out16=None, fault=None, at=(0, 0)):
    """dx, dgamma, dbeta (and, with out16 = a 16-bit dtype, dxb = 16-bit(fp32(dx) f) and colsum = sum_r dxb) of the formulas above, every operation in `prec`.
    `fault` (one of FAULTS) is applied where it arises, at row / column `at`."""
    assert fault is None or fault in FAULTS
    r, c = at
    x, gamma, dy, mean, rstd = (inp[k].to(prec) for k in ("x", "gamma", "dy", "mean", "rstd"))
    C = inp["C"]
    d = dy * inp["dy_scale"] if inp["dy_scale"] is not None else dy
    xh = (x - mean[:, None]) * rstd[:, None]
    g = d * gamma
    m1 = g.sum(1) / C
    if fault == "mean_column_dropped":
        m1[r] = (g[r].sum() - g[r, c]) / C
    m2 = (g * xh).sum(1) / C
    rs_out = rstd.clone()
    if fault == "neighbour_rstd":
        n = r - 1 if r > 0 else r + 1
        assert rstd[n] != rstd[r]
        rs_out[r] = rstd[n]
    dx = rs_out[:, None] * (g - m1[:, None] - xh * m2[:, None])
    if inp["dres"] is not None:
        dx = dx + inp["dres"].to(prec)
    pg, pb = d * xh, d.clone()
    if fault == "dgamma_row_missing":
        pg[r] = 0
    if fault == "dbeta_row_missing":
        pb[r] = 0
    out = {"dx": dx, "dgamma": pg.sum(0), "dbeta": pb.sum(0)}
    if out16 is not None:
        f = row_factor(inp, torch.float32, r if fault == "row_scale_neighbour" else None)
        v = dx.float() * f[:, None]
        out["dxb"] = truncate16(v, out16) if fault == "truncated_store" else rne16(v, out16)
        summed = out["dxb"].to(prec)
        if fault == "colsum_before_scale":
            assert inp["rs"] is not None
            summed = rne16(dx.float(), out16).to(prec)
        if fault == "colsum_row_missing":
            assert bool((summed[r] != 0).any())
            summed = summed.clone()
            summed[r] = 0
        out["colsum"] = summed.sum(0)
    return out


def reference64(inp):
    """the float64 results and one scale per element (the same terms with every factor replaced by its absolute value) -> dict dx, dgamma, dbeta, s_dx, s_dgamma, s_dbeta"""
    ref = evaluate(inp, torch.float64)
    x, gamma, dy, mean, rstd = (inp[k].double() for k in ("x", "gamma", "dy", "mean", "rstd"))
    d = (dy * inp["dy_scale"] if inp["dy_scale"] is not None else dy).abs()
    xh = ((x - mean[:, None]) * rstd[:, None]).abs()
    g = d * gamma.abs()
    s = rstd[:, None] * (g + g.mean(1, keepdim=True) + xh * (g * xh).mean(1, keepdim=True))
    if inp["dres"] is not None:
        s = s + inp["dres"].double().abs()
    ref.update({"s_dx": s, "s_dgamma": (d * xh).sum(0), "s_dbeta": d.sum(0)})
    return ref


def scaled(got, ref64, s):
    """|got - ref64| / s per element (0 / 0 = 0, a NaN or x / 0 = inf)"""
    err = (got.detach().cpu().double() - ref64).abs()
    e = torch.where(s > 0, err / s, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)


def _worst(e):
    i = int(e.argmax())
    return float(e.reshape(-1)[i]), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), e.shape))


def bounds(inp, ref):
    """-> ({kind: B}, {kind: E32}) for dx, dgamma, dbeta: B = max(FACTOR x E32, FLOOR), E32 from torch's float32 evaluation"""
    f32 = evaluate(inp, torch.float32)
    e32 = {k: _worst(scaled(f32[k], ref[k], ref["s_" + k]))[0] for k in ("dx", "dgamma", "dbeta")}
    return {k: max(FACTOR * v, FLOOR) for k, v in e32.items()}, e32


def check(kind, got, ref64, s, B, e32, what=""):
    """assert |got - ref64| <= B s element-wise; prints the worst scaled error, E32 and their ratio; -> the worst scaled error"""
    assert got.shape == ref64.shape, (what, kind, got.shape, ref64.shape)
    e, at = _worst(scaled(got, ref64, s))
    ratio = e / e32 if e32 > 0 else (0.0 if e == 0 else float("inf"))
    print(f"ln {what} {kind}: worst scaled error {e:.3e} at {at}, E32 {e32:.3e}, ratio {ratio:.2f}, bound {B:.3e}")
    assert e <= B, (what, kind, "element", at, "scaled error", e, "bound", B)
    return e


def check_backward(got, inp, ref, B, e32, what=""):
    """every output present in `got` (dx, dgamma, dbeta f32; dxb 16-bit; colsum f32) against its rule"""
    for k in ("dx", "dgamma", "dbeta"):
        if got.get(k) is not None:
            check(k, got[k], ref[k], ref["s_" + k], B[k], e32[k], what)
    dxb = got.get("dxb")
    if dxb is not None:
        f = row_factor(inp)
        if got.get("dx") is not None:
            gemmbound.check_exact(dxb.detach().cpu(), rne16(got["dx"].detach().cpu() * f[:, None], dxb.dtype), what + " dxb = RNE16(dx f)")
        else:
            f64 = f.double()[:, None]
            gemmbound.check_half_ulp(dxb, ref["dx"] * f64, B["dx"] * ref["s_dx"] * f64.abs(), what + " dxb")
    if got.get("colsum") is not None:
        check_colsum(got["colsum"], dxb, what)


def check_colsum(got, stored, what=""):
    """column sums of the STORED 16-bit tensor: float64 of it, S = sum_r |stored|, B from torch's float32 sum"""
    st = stored.detach().cpu().double()
    ref, s = st.sum(0), st.abs().sum(0)
    e32 = _worst(scaled(stored.detach().cpu().float().sum(0), ref, s))[0]
    return check("colsum", got, ref, s, max(FACTOR * e32, FLOOR), e32, what)


# ---------------------------------------------------------------------------------------------------------------- preconditions
def assert_sensitive(inp, ref, B, out16=None, colsum=False, what=""):
    """From float64 alone: each fault moves (one of) its element(s) by >= SIGNAL_FACTOR x B S.
       * one column missing from a row's mean_c g -- for EVERY row, with the row's smallest |g| as the dropped column (the hardest one); the whole row moves by
         rstd |g| / C, the element with the smallest scale shows it first;
       * one row missing from dbeta: every (row, column);
       * one row missing from dgamma: >= 80 % of (row, column) -- xh may be near zero (the rule of rowbound.py for dq / dk);
       * one row missing from a column sum: >= 80 % of (row, column) among the rows whose factor is not zero (a dx entry may cancel; a zero row has nothing to miss);
       * dxb_rs taken from the neighbouring sample: >= 80 % of the elements, against the half-ulp rule's own allowance (half an ulp + the slack)."""
    x, gamma, dy, mean, rstd = (inp[k].double() for k in ("x", "gamma", "dy", "mean", "rstd"))
    C = inp["C"]
    d = dy * inp["dy_scale"] if inp["dy_scale"] is not None else dy
    g = (d * gamma).abs()
    sig = (rstd * g.min(1).values / C) / ref["s_dx"].min(1).values
    assert float(sig.min()) >= SIGNAL_FACTOR * B["dx"], (what, "mean column", float(sig.min()) / B["dx"])
    msg = f"ln {what} fault signal / bound: mean column {float(sig.min()) / B['dx']:.0f}"
    if inp["T"] > 1:
        sb = (d.abs() / ref["s_dbeta"]).min()
        assert float(sb) >= SIGNAL_FACTOR * B["dbeta"], (what, "dbeta row", float(sb) / B["dbeta"])
        xh = (x - mean[:, None]) * rstd[:, None]
        fg = float(((d * xh).abs() / ref["s_dgamma"] >= SIGNAL_FACTOR * B["dgamma"]).double().mean())
        assert fg >= 0.8, (what, "dgamma rows", fg)
        msg += f", dbeta row {float(sb) / B['dbeta']:.0f}, dgamma rows covered {100 * fg:.1f} %"
    if out16 is not None:
        f = row_factor(inp, torch.float64)
        if colsum and inp["T"] > 1:
            st = evaluate(inp, torch.float64, out16)["dxb"].double()
            live = f != 0
            Bc = max(FACTOR * _worst(scaled(st.float().sum(0), st.sum(0), st.abs().sum(0)))[0], FLOOR)
            fc = float((st[live].abs() / st.abs().sum(0) >= SIGNAL_FACTOR * Bc).double().mean())
            assert fc >= 0.8, (what, "colsum rows", fc)
            msg += f", colsum rows covered {100 * fc:.1f} %"
        if inp["rs"] is not None:
            idx = torch.arange(inp["T"]) // inp["rps"]
            fn = inp["rs"].double()[(idx - 1).clamp_min(0)]
            rows = idx >= 1
            want = ref["dx"] * f[:, None]
            allow = gemmbound.half_ulp_distance(want, out16) + B["dx"] * ref["s_dx"] * f.abs()[:, None] + 0.5 * (want.abs() * (2.0 ** -7 if out16 == torch.bfloat16 else 2.0 ** -10))
            fr = float(((ref["dx"] * (f - fn)[:, None]).abs()[rows] >= SIGNAL_FACTOR * allow[rows]).double().mean())
            assert fr >= 0.8, (what, "row scale", fr)
            msg += f", neighbour's dxb_rs covered {100 * fr:.1f} %"
    print(msg)


def plant(name, inp, out16=None, at=None):
    """a float32-evaluated result with the fault `name` applied (dict as `evaluate`; dx is dropped for the faults of the 16-bit copy that show only against float64).
    Default place: the last row of the first 16-row block (or the last row), column C // 2; neighbour faults: the first row of the second sample."""
    T, C = inp["T"], inp["C"]
    if at is None:
        at = (min(BLOCK_ROWS, T) - 1, C // 2)
        if name == "row_scale_neighbour":
            at = (inp["rps"], C // 2)
        if name == "colsum_row_missing":          # (a row whose factor is zero has nothing to miss: the last row of the block that has)
            live = torch.nonzero(row_factor(inp)[:at[0] + 1] != 0)
            at = (int(live[-1]), C // 2)
    return evaluate(inp, torch.float32, out16, fault=name, at=at)


# ---------------------------------------------------------------------------------------------------------------- forward
def forward64(inp, eps):
    """y, mean, rstd in float64 and their scales: S_y = (|x - mu| + |mu|) rstd |gamma| + |beta| (x - mu in fp32 carries 2^-24 |mu|), S_mean = mean_c |x|,
    S_rstd = rstd max(1, mean_c(|x - mu| (|x - mu| + |mu|)) / (var + eps)): d rstd = -rstd dvar / (2 (var + eps)) and a rounding of x - mu by u (|x - mu| + |mu|) moves
    (x - mu)^2 by 2 |x - mu| times that."""
    x, gamma, beta = inp["x"].double(), inp["gamma"].double(), inp["beta"].double()
    mu = x.mean(1, keepdim=True)
    dlt = x - mu
    var = (dlt ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return {"y": dlt * rstd * gamma + beta, "mean": mu[:, 0], "rstd": rstd[:, 0],
            "s_y": (dlt.abs() + mu.abs()) * rstd * gamma.abs() + beta.abs(), "s_mean": x.abs().mean(1),
            "s_rstd": (rstd * ((dlt.abs() * (dlt.abs() + mu.abs())).mean(1, keepdim=True) / (var + eps)).clamp_min(1.0))[:, 0]}


def forward32(inp, eps, one_pass=False):
    """torch's float32 layer_norm with float32 statistics (`one_pass`: the variance as E[x^2] - E[x]^2 in float32, the fault the far rows are there for)"""
    x, gamma, beta = inp["x"], inp["gamma"], inp["beta"]
    mu = x.mean(1, keepdim=True)
    var = ((x * x).mean(1, keepdim=True) - mu * mu).clamp_min(0) if one_pass else ((x - mu) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (x - mu) * rstd * gamma + beta if one_pass else torch.nn.functional.layer_norm(x, (inp["C"],), gamma, beta, eps)
    return {"y": y, "mean": mu[:, 0], "rstd": rstd[:, 0]}


def forward_bounds(inp, ref, eps):
    f32 = forward32(inp, eps)
    e32 = {k: _worst(scaled(f32[k], ref[k], ref["s_" + k]))[0] for k in ("y", "mean", "rstd")}
    return {k: max(FACTOR * v, FLOOR) for k, v in e32.items()}, e32


def check_forward(got, ref, B, e32, what=""):
    for k in ("y", "mean", "rstd"):
        check(k, got[k], ref[k], ref["s_" + k], B[k], e32[k], what)
