"""TEST INFRASTRUCTURE: per-row bounds for the attention kernels (tests/test_attention_rows.py, tests/test_attention_single_query_rows.py,
tests/test_swin_window_rows.py; tested on itself by tests/test_rowbound.py).

A whole-tensor norm hides one wrong row (it costs 1 / sqrt(rows) of the norm) and dense Gaussian q / k hide one wrong key (each key holds 1 / N of a row's mass, less than
the row's 16-bit rounding noise).  This module supplies both halves of a check that sees them:

  * inputs in which every key is the dominant key of exactly one query (`peaked_inputs`: a fixed permutation pi, k[pi(i)] carries a multiple of q_i), resp. one query with a
    few planted keys (`single_query_inputs`), so that every tile, chunk and tail edge carries O(1) weight in some row of o, dq, dk and dv;
  * a float64 reference with one scale per output ROW (`reference64`): the same products with every factor replaced by its absolute value -- what went into the row, not what
    came out of it (a cancellation-dominated dq row of the 16-bit oracle itself is 25 - 58 % of its own norm away from float64) --, and the scaled row
    error e(r) = |got_r - ref_r|_2 / s(r);
  * the bound: 4 x the worst scaled row error of the 16-bit oracle (oracle/bf16ops.py in the case's mode, gradients rounded) on the same inputs, computed inside the test and
    never taken from a kernel (`oracle16`, `check_rows`); lse element by element against 8 x the error of torch's float32 logsumexp (`check_lse`);
  * the preconditions that make the check meaningful (`signals`, `assert_sensitive`): from float64 alone, the scaled row error that "query pi^-1(j) ignores key j" /
    "key j's row misses query pi^-1(j)" would cause is >= 3 x the bound -- for every key in o and dv, for >= 80 % of the keys per dout seed and for every key in at least
    one of the case's dout seeds in dq and dk (dS_ij = P_ij (dP_ij - D_i) can cancel by chance);
  * the planted faults themselves (`plant`), for the CPU self-test of the checker.

All tensors here are [..., Nq, hd] / [..., Nk, hd] with any leading (batch, head) dimensions."""
from __future__ import annotations

import math

import torch

from oracle import bf16ops

FACTOR = 4.0            # kernel's worst row <= FACTOR x the oracle's worst row
LSE_FACTOR = 8.0        # fast exp / log and another summation order against torch's float32 logsumexp
SIGNAL_FACTOR = 3.0     # a planted fault must stand this far above the bound
MODE = {torch.bfloat16: "bf16_operands", torch.float16: "fp16_operands"}
KINDS = ("o", "dq", "dk", "dv")


# ---------------------------------------------------------------------------------------------------------------- inputs
def permutation(N: int) -> torch.Tensor:
    """pi(i) = (i s + N // 2) mod N with s the first integer >= max(2, N // 3) coprime to N: a query's matched key lies about a third of the sequence further on
    than its neighbour's, so the matched keys of one query tile are spread over every key tile and chunk"""
    s = max(2, N // 3)
    while math.gcd(s, N) != 1:
        s += 1
    return (torch.arange(N) * s + N // 2) % N


def peaked_inputs(B, N, H, hd, dtype, seed, dout_seed=None):
    """-> (qkv [B, N, 3 H hd], dout [B, N, H hd], pi [N]) in `dtype`.  q, v, dout ~ N(0, 1), k ~ 0.7 N(0, 1) and k[pi(i)] += q_i c / |q_i|^2 with c = (ln N + 0.5) sqrt(hd):
    with the hd^-0.5 scale the matched logit sits ln N + 0.5 above the rest, so the matched key holds about half of its query's mass and the rest of the row the other
    half.  `dout_seed` draws another dout for the same qkv (None: `seed`)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, N, hd, generator=g, dtype=torch.float64)
    k = torch.randn(B, H, N, hd, generator=g, dtype=torch.float64) * 0.7
    v = torch.randn(B, H, N, hd, generator=g, dtype=torch.float64)
    pi = permutation(N)
    c = (math.log(N) + 0.5) * math.sqrt(hd)
    k[:, :, pi] += q * (c / q.pow(2).sum(-1, keepdim=True))
    gd = torch.Generator().manual_seed(7919 + (seed if dout_seed is None else dout_seed))
    dout = torch.randn(B, N, H * hd, generator=gd, dtype=torch.float64)
    qkv = torch.cat([t.permute(0, 2, 1, 3).reshape(B, N, H * hd) for t in (q, k, v)], dim=2)
    return qkv.to(dtype), dout.to(dtype), pi


def planted_keys(N: int, edge: int):
    """first, last and one tile-edge key (the last key of the first `edge`-key pass, or the middle one where N does not reach it)"""
    return sorted({0, N - 1, edge - 1 if N > edge else N // 2})


def single_query_inputs(B, N, H, hd, dtype, seed, edge=64, shared_q=False, qg_dtype=None):
    """One query per (batch, head) item -- the same for every batch item with `shared_q` -- and N keys: q, v, dout ~ N(0, 1), k ~ 0.7 N(0, 1) with the keys of
    planted_keys(N, edge) moved to ln N above the rest (each holds about a quarter of the mass, the N - 3 others share the last quarter).  k and v are rounded to `dtype`,
    q and dout to `qg_dtype` (None: `dtype`).  -> (q [B, H, 1, hd], k, v [B, H, N, hd], dout [B, H, 1, hd], planted), all float64-typed"""
    g = torch.Generator().manual_seed(seed)
    rq = lambda t: t.to(dtype if qg_dtype is None else qg_dtype).double()
    q = rq(torch.randn(1 if shared_q else B, H, 1, hd, generator=g, dtype=torch.float64).expand(B, H, 1, hd).clone())
    k = torch.randn(B, H, N, hd, generator=g, dtype=torch.float64) * 0.7
    v = torch.randn(B, H, N, hd, generator=g, dtype=torch.float64)
    dout = rq(torch.randn(B, H, 1, hd, generator=g, dtype=torch.float64))
    planted = planted_keys(N, edge)
    c = math.log(N) * math.sqrt(hd)
    k[:, :, planted] += q * (c / q.pow(2).sum(-1, keepdim=True))
    return q, k.to(dtype).double(), v.to(dtype).double(), dout, planted


def split_heads(qkv, H):
    """[B, N, 3 H hd] -> q, k, v [B, H, N, hd] (timm Attention.forward's layout), same dtype"""
    B, N, D3 = qkv.shape
    x = qkv.reshape(B, N, 3, H, D3 // (3 * H)).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def heads_of(t, H):
    """[B, N, H hd] -> [B, H, N, hd]"""
    B, N, D = t.shape
    return t.reshape(B, N, H, D // H).transpose(1, 2)


# ---------------------------------------------------------------------------------------------------------------- float64 reference and row scales
def reference64(q, k, v, g, sc, bias=None):
    """float64 on the given (16-bit-valued) inputs.  -> dict: o, dq, dk, dv, lse; the row scales s_o, s_dq, s_dk, s_dv; P and dS (for `signals` and `plant`).
    P = softmax(sc q k^T (+ bias)), O = P v, dP = g v^T, D_i = sum_c g_ic O_ic, dS = P o (dP - D); dQ = sc dS k, dK = sc dS^T q, dV = P^T g.  The scales are the same products
    of absolute values: s_o = |P |v||, s_dv = |P^T |g||, A = P o (|dP| + sum_c |g_ic| |O_ic|), s_dq = sc |A |k||, s_dk = sc |A^T |q|| (row 2-norms).  The second term of A
    is sum |g| |O| and not |D|: the rounding of O inside D is part of what goes into a dS row."""
    q, k, v, g = (t.double() for t in (q, k, v, g))
    s = sc * (q @ k.transpose(-2, -1))
    if bias is not None:
        s = s + bias.double()
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    O = P @ v
    dP = g @ v.transpose(-2, -1)
    D = (g * O).sum(-1, keepdim=True)
    dS = P * (dP - D)
    A = P * (dP.abs() + (g.abs() * O.abs()).sum(-1, keepdim=True))
    n2 = lambda t: t.norm(dim=-1)
    return {"o": O, "dq": sc * (dS @ k), "dk": sc * (dS.transpose(-2, -1) @ q), "dv": P.transpose(-2, -1) @ g, "lse": lse, "P": P, "dS": dS, "A": A,
            "s_o": n2(P @ v.abs()), "s_dv": n2(P.transpose(-2, -1) @ g.abs()), "s_dq": sc * n2(A @ k.abs()), "s_dk": sc * n2(A.transpose(-2, -1) @ q.abs())}


def oracle16(q, k, v, g, sc, dtype):
    """oracle/bf16ops.py in the 16-bit mode of `dtype` on the same inputs in float32 (what autocast computes in), gradients rounded to the format (the kernels store 16-bit
    gradients; tests/test_attention.py does the same) -> dict o, dq, dk, dv"""
    q, k, v = (t.float().clone().requires_grad_(True) for t in (q, k, v))
    with bf16ops.precision(MODE[dtype]):
        o = bf16ops.attention(q, k, v, sc)
        o.backward(g.float())
        return {"o": o.detach(), "dq": bf16ops.rb(q.grad), "dk": bf16ops.rb(k.grad), "dv": bf16ops.rb(v.grad)}


def fp32_forward_floor(q, k, sc):
    """For a kernel whose probabilities and output are fp32 (csrc/attn_pool.hip): the worst row of a float32 torch evaluation is a maximum over a handful of rows of pure
    summation-order noise (2e-7) and no measure of another correct order, so such outputs get the deterministic fp32 accumulation bound as a floor.  A score is a chain
    of hd fmas, |ds| <= hd u T with T = max_n sum_c |q_c sc k_nc| and u = 2^-24; the row maximum carries the same, so |dp_n| <= p_n (2 hd T + 4) u (4 u: exp, the
    reciprocal, the product); o = sum_n p_n v_n in N more fmas: |do| <= (N + 2 hd T + 4) u (P |v|).  -> (relative bound on p, bound on o in units of s_o); 1e-5 .. 1e-4."""
    T = float((sc * (q.double().abs() @ k.double().abs().transpose(-2, -1))).max())
    u = 2.0 ** -24
    rel_p = (2.0 * q.shape[-1] * T + 4.0) * u
    return rel_p, rel_p + k.shape[-2] * u


def row_errors(kind, got, ref):
    """scaled row errors e(r) = |got_r - ref_r|_2 / s(r) of one tensor kind, shape [..., rows]"""
    return (got.double() - ref[kind]).norm(dim=-1) / ref["s_" + kind]


def worst(e):
    """(max, index tuple) of a tensor of row errors; a NaN anywhere is the maximum"""
    e = torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)
    i = int(e.argmax())
    return float(e.reshape(-1)[i]), tuple(int(x) for x in torch.unravel_index(torch.tensor(i), e.shape))


def bounds(ref, orc, kinds=KINDS, o_floor=0.0):
    """per tensor kind: FACTOR x the worst scaled row error of the oracle's own result.
    dq and dk have a floor of 2 hd 2^-24, the fp32 accumulation bound of dS itself: dP_ij and D_i are two fp32 sums of hd products each, |error| <= hd u (sum |g| |v_j| + sum
    |g| |O|) with u = 2^-24, which is <= 2 hd u of the row scale wherever one key dominates.  It only matters where dS cancels exactly: with one key (P = 1, dS = 0) the oracle's
    E_or is 0 or 1e-8 by the luck of its summation order and says nothing about another order.  The floor is 8e-6 .. 1e-5, 40 x below the smallest 16-bit bound."""
    out = {kind: FACTOR * worst(row_errors(kind, orc[kind], ref))[0] for kind in kinds}
    if "o" in out:
        out["o"] = max(out["o"], o_floor)          # kernels with an fp32 output: see fp32_forward_floor
    for kind in ("dq", "dk"):
        if kind in out:
            out[kind] = max(out[kind], 2.0 * ref["o"].shape[-1] * 2.0 ** -24)
    return out


def check_rows(kind, got, ref, bound, what=""):
    """assert max_r e_kernel(r) <= bound (= FACTOR x E_or); prints max e_kernel, E_or and the ratio; -> the ratio"""
    e, at = worst(row_errors(kind, got, ref))
    e_or = bound / FACTOR
    ratio = e / e_or if e_or > 0 else (0.0 if e == 0 else float("inf"))
    print(f"rows {what} {kind}: max e_kernel {e:.3e} at (…, row) {at}, E_or {e_or:.3e}, ratio {ratio:.2f}")
    assert e <= bound, (what, kind, "row", at, e, "bound", bound)
    return ratio


def lse_bound(q, k, sc, ref, bias=None):
    """element-wise bound on lse: LSE_FACTOR x max(E32, eps32 |lse64|), E32 = the worst absolute error of a float32 torch evaluation (float32 logits of the same inputs,
    torch.logsumexp) against float64"""
    s32 = sc * (q.float() @ k.float().transpose(-2, -1))
    if bias is not None:
        s32 = s32 + bias.float()
    e32 = float((torch.logsumexp(s32, -1).double() - ref["lse"]).abs().max())
    return LSE_FACTOR * torch.maximum(torch.full_like(ref["lse"], e32), torch.finfo(torch.float32).eps * ref["lse"].abs()), e32


def check_lse(got, q, k, sc, ref, what="", bias=None):
    bound, e32 = lse_bound(q, k, sc, ref, bias)
    err = (got.double() - ref["lse"]).abs()
    over = err / bound
    m, at = worst(over)
    print(f"rows {what} lse: max |err| {float(err.max()):.3e}, E32 {e32:.3e}, worst err / (max(E32, eps |lse|)) {m * LSE_FACTOR:.2f}")
    assert m <= 1.0, (what, "lse", at, float(err[at]), float(bound[at]))
    return m * LSE_FACTOR


# ---------------------------------------------------------------------------------------------------------------- planted faults and their signal
def pairs_of(pi):
    """(query, key) index pairs (pi^-1(j), j) for every key j, as two index tensors ordered by key"""
    inv = torch.empty_like(pi)
    inv[pi] = torch.arange(len(pi))
    return inv, torch.arange(len(pi))


def fault_delta(kind, ref, q, k, v, g, sc, qi, kj):
    """what the faults at the pairs (query qi[n], key kj[n]) (index tensors) remove from their rows, in float64 [..., n, hd] (leading dims of the inputs):
       o:  query qi ignores key kj (the row is renormalised over the other keys): O_i - O'_i = p (v_j - O_i) / (1 - p)
       dq: query qi ignores key kj: sc dS_ij k_j         dk: key kj's row misses query qi: sc dS_ij q_i         dv: key kj's row misses query qi: P_ij g_i"""
    p = ref["P"][..., qi, kj][..., None]
    ds = ref["dS"][..., qi, kj][..., None]
    if kind == "o":
        return p * (v.double()[..., kj, :] - ref["o"][..., qi, :]) / (1.0 - p).clamp_min(1e-300)
    if kind == "dq":
        return sc * ds * k.double()[..., kj, :]
    if kind == "dk":
        return sc * ds * q.double()[..., qi, :]
    return p * g.double()[..., qi, :]


def signals(kind, ref, q, k, v, g, sc, qi, kj):
    """scaled row error the fault at each pair (qi[n], kj[n]) would cause -> [..., n]"""
    rows = qi if kind in ("o", "dq") else kj
    return fault_delta(kind, ref, q, k, v, g, sc, qi, kj).norm(dim=-1) / ref["s_" + kind][..., rows]


def plant(kind, result, ref, q, k, v, g, sc, qi, kj, item):
    """a copy of `result` (dict of [..., rows, hd] tensors) with the fault at (query qi, key kj) applied to `kind` in the (batch, head) item `item` (an index tuple)"""
    out = {n: t.clone() for n, t in result.items()}
    row = qi if kind in ("o", "dq") else kj
    d = fault_delta(kind, ref, q, k, v, g, sc, torch.tensor([qi]), torch.tensor([kj]))[item + (0,)]
    out[kind][item + (row,)] = (out[kind][item + (row,)].double() - d).to(out[kind].dtype)
    return out


def covered(kind, ref, q, k, v, g, sc, qi, kj, bound):
    """[..., pairs] bool: the pair's fault signal is >= SIGNAL_FACTOR x bound"""
    return signals(kind, ref, q, k, v, g, sc, qi, kj) >= SIGNAL_FACTOR * bound


def assert_sensitive(refs, inputs, sc, qi, kj, bnds, what=""):
    """The preconditions, from float64 alone.  `refs`, `inputs`, `bnds`: one entry per dout seed of the case (inputs = (q, k, v, g)).  o and dv: every pair of every
    (batch, head) item in every seed; dq and dk: >= 80 % of all pairs per seed, and every key INDEX in at least one seed and item -- a tile, chunk or tail edge is a position
    in the sequence, the same in every item, and what differs from item to item (a workgroup walking on to its next item) is covered by o and dv in full."""
    assert 1 <= len(refs) <= 3
    if ref_is_trivial(refs[0]):
        return                      # one key: P = 1, dS = 0, nothing to ignore
    for kind in KINDS:
        cov = [covered(kind, r, *inp, sc, qi, kj, b[kind]) for r, inp, b in zip(refs, inputs, bnds)]
        frac = [float(c.double().mean()) for c in cov]
        union = torch.stack(cov).reshape(-1, cov[0].shape[-1]).any(0)          # per key index: over the seeds and the (batch, head) items
        print(f"rows {what} {kind}: fault signal >= {SIGNAL_FACTOR:.0f} x bound for " + ", ".join(f"{100 * f:.1f} %" for f in frac) + f" of the keys per seed, union {100 * float(union.double().mean()):.1f} %")
        if kind in ("o", "dv"):
            assert all(bool(c.all()) for c in cov), (what, kind, frac)
        else:
            assert min(frac) >= 0.8, (what, kind, frac)
            assert bool(union.all()), (what, kind, "keys no dout seed covers", torch.nonzero(~union).tolist()[:8])


def ref_is_trivial(ref):
    return ref["P"].shape[-1] == 1
