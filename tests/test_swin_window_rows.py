"""Swin window attention, every output row bounded (tests/rowbound.py): vdk_window_attention_fwd / bwd (bf16; the public entries take no other format) and
vdk_window_attention_fwd_f32, with and without a shift mask, with and without a row index, on the CPU SIMT emulation and on the device.

Inputs: inside each 49-token window a permutation pi_w is drawn among the keys the window's mask leaves visible to each query (a perfect matching of the visibility
graph), and k[pi_w(i)] carries a multiple of q_i, so that every key of every window is the dominant key of exactly one query (tests/rowbound.py).  Bias and mask are those
of tests/test_swin.py::test_window_attention_fwd_bwd_vs_torch (bias 0.5 randn, a random 0 / -100 mask with an open diagonal), at that test's smallest window and head counts.

Checks: o, dq, dk, dv per (window, head, token) row against float64, scaled by the absolute-value products that went into the row, <= 4 x the worst row of the 16-bit
oracle (the arithmetic of oracle/bf16ops.py's attention with the bias and mask added to the logits); d(bias) per element, scaled by the same products summed over the
windows, against the oracle's fp32 sum of unrounded dS (the kernel sums its fp32 dS, csrc/window_attention.hip); lse element by element.  The fp32 kernel: o rows against
4 x the worst row of the same formula in float32 torch."""
import ctypes as C

import pytest
import torch

from oracle import bf16ops
from tests import rowbound as rb
from tests.test_swin_precise import _run_attn as run_f32

N, HD = 49, 32
SC = HD ** -0.5
TINY = 1e-30          # below the fp32 normal range: a (query, key) every window masks has P = e^-100 in float64 and 0 in fp32
# (windows, heads, nW, indexed): tests/test_swin.py's smallest window and head counts, each without and with a mask, without and with rowidx
CASES = [(3, 2, 0, False), (3, 2, 0, True), (8, 2, 4, False), (8, 2, 4, True)]
_CASE = {}


def _mask(nW, gen):
    m = torch.where(torch.rand(nW, N, N, generator=gen) < 0.3, torch.full((), -100.0), torch.zeros(()))
    m[:, torch.arange(N), torch.arange(N)] = 0.0
    return m


def _matching(visible, order):
    """a permutation pi with visible[i, pi[i]] for every query i (Kuhn's augmenting paths; `order`: the keys in the order each query tries them)"""
    owner = [-1] * N

    def place(i, seen):
        for j in order[i]:
            if visible[i][j] and j not in seen:
                seen.add(j)
                if owner[j] < 0 or place(owner[j], seen):
                    owner[j] = i
                    return True
        return False

    for i in range(N):
        assert place(i, set()), "no perfect matching among the visible keys"
    pi = torch.empty(N, dtype=torch.long)
    for j, i in enumerate(owner):
        pi[i] = j
    return pi


def inputs(windows, heads, nW, dtype, seed=3, dout_seed=0):
    """-> q, k, v, g [windows, heads, 49, 32] (float64-typed, rounded to `dtype`), bias [heads, 49, 49], mask [nW, 49, 49] | None, pi [windows, 49]"""
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(windows, heads, N, HD, generator=gen, dtype=torch.float64)
    k = torch.randn(windows, heads, N, HD, generator=gen, dtype=torch.float64) * 0.7
    v = torch.randn(windows, heads, N, HD, generator=gen, dtype=torch.float64)
    bias = torch.randn(heads, N, N, generator=gen) * 0.5
    mask = _mask(nW, gen) if nW else None
    c = (torch.log(torch.tensor(float(N))).item() + 0.5) * HD ** 0.5
    pis = []
    for w in range(windows):
        order = [torch.randperm(N, generator=gen).tolist() for _ in range(N)]
        vis = (mask[w % nW] == 0).tolist() if nW else [[True] * N] * N
        pi = _matching(vis, order)
        k[w][:, pi] += q[w] * (c / q[w].pow(2).sum(-1, keepdim=True))
        pis.append(pi)
    g = torch.randn(windows, heads, N, HD, generator=torch.Generator().manual_seed(100 + dout_seed), dtype=torch.float64)
    r = lambda t: t.to(dtype).double()
    return r(q), r(k), r(v), r(g), bias, mask, torch.stack(pis)


def logit_bias(bias, mask, windows):
    b = bias[None].double()
    return b if mask is None else b + mask[torch.arange(windows) % mask.shape[0]][:, None].double()


def oracle16(q, k, v, g, lb):
    """oracle/bf16ops.py's attention arithmetic in bf16_operands mode (float32; P rounded once, o rounded, D from the rounded o, dS rounded, gradients rounded) with the
    bias and mask added to the logits; d(bias) = the fp32 sum over the windows of the UNROUNDED dS, as the kernel forms it"""
    q, k, v, g, lb = (t.float() for t in (q, k, v, g, lb))
    with bf16ops.precision("bf16_operands"):
        r = bf16ops.rb
        s = (q @ k.transpose(-2, -1)) * SC + lb
        p = torch.exp(s - torch.logsumexp(s, -1, keepdim=True))
        o = r(r(p) @ v)
        dp = g @ v.transpose(-2, -1)
        ds = p * (dp - (g * o).sum(-1, keepdim=True))
        return {"o": o, "dv": r(r(p).transpose(-2, -1) @ g), "dq": r((r(ds) @ k) * SC), "dk": r((r(ds).transpose(-2, -1) @ q) * SC), "dbias": ds.sum(0)}


def dbias_errors(got, ref):
    return (got.double() - ref["dS"].sum(0)).abs() / (ref["A"].sum(0) + TINY)


def case(windows, heads, nW, dtype):
    key = (windows, heads, nW, dtype)
    if key not in _CASE:
        q, k, v, g, bias, mask, pi = inputs(windows, heads, nW, dtype)
        lb = logit_bias(bias, mask, windows)
        ref = rb.reference64(q, k, v, g, SC, bias=lb)
        if dtype == torch.float32:
            s = (q.float() * SC) @ k.float().transpose(-2, -1) + lb.float()
            orc = {"o": s.softmax(-1) @ v.float()}
            bnd = rb.bounds(ref, orc, kinds=("o",))
        else:
            orc = oracle16(q, k, v, g, lb)
            bnd = rb.bounds(ref, orc)
            bnd["dbias"] = rb.FACTOR * float(dbias_errors(orc["dbias"], ref).max())
        # the preconditions, from float64 alone, window by window (each has its own permutation)
        cov = {kind: [] for kind in bnd if kind != "dbias"}
        for w in range(windows):
            rw = {n: t[w] for n, t in ref.items()}
            qi, kj = rb.pairs_of(pi[w])
            for kind in cov:
                cov[kind].append(rb.covered(kind, rw, q[w], k[w], v[w], g[w], SC, qi, kj, bnd[kind]))
        for kind, c in cov.items():
            c = torch.stack(c)                                                  # [windows, heads, keys]
            frac = float(c.double().mean())
            print(f"rows window W{windows} H{heads} nW{nW} {dtype} {kind}: fault signal >= 3 x bound for {100 * frac:.1f} % of the keys")
            if kind in ("o", "dv"):
                assert bool(c.all()), (kind, frac)
            else:
                assert frac >= 0.8 and bool(c.reshape(-1, N).any(0).all()), (kind, frac)
        _CASE[key] = (q, k, v, g, bias, mask, lb, ref, bnd)
    return _CASE[key]


def _rows(t, heads):
    """[windows * 49, heads * 32] -> [windows, heads, 49, 32]"""
    return t.reshape(-1, N, heads, HD).transpose(1, 2)


def _flat(t):
    W, H = t.shape[:2]
    return t.transpose(1, 2).reshape(W * N, H * HD)


def run_16(be, dev, qkv, dout, bias, mask, windows, heads, rowidx):
    Cc = heads * HD
    nW = 0 if mask is None else mask.shape[0]
    p = be.ptr
    qd, gd, bd = qkv.to(dev).contiguous(), dout.to(dev).contiguous(), bias.to(dev).contiguous()
    md = None if mask is None else mask.to(dev).contiguous()
    rd = None if rowidx is None else rowidx.to(torch.int32).to(dev)
    o = torch.full((windows * N, Cc), float("nan"), dtype=qkv.dtype, device=dev)
    lse = torch.full((windows, heads, N), float("nan"), dtype=torch.float32, device=dev)
    dqkv = torch.full((windows * N, 3 * Cc), float("nan"), dtype=qkv.dtype, device=dev)
    dbias = torch.full((heads, N, N), float("nan"), dtype=torch.float32, device=dev)
    need = C.c_size_t(0)
    be.check(be.lib.vdk_window_attention_fwd_workspace_bytes(nW, heads, C.byref(need)), "fwd workspace")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    be.check(be.lib.vdk_window_attention_fwd(p(qd), 3 * Cc, p(o), Cc, p(lse), p(bd), p(md), nW, windows, heads, N, HD, SC, p(rd), p(ws), ws.numel(), be.stream()), "window fwd")
    be.check(be.lib.vdk_window_attention_bwd_workspace_bytes(windows, nW, heads, C.byref(need)), "bwd workspace")
    wb = torch.empty(need.value, dtype=torch.uint8, device=dev)
    be.check(be.lib.vdk_window_attention_bwd(p(qd), 3 * Cc, p(o), p(gd), Cc, p(lse), p(bd), p(md), nW, windows, heads, N, HD, SC, p(rd), p(dqkv), 3 * Cc, p(dbias), p(wb),
                                             wb.numel(), be.stream()), "window bwd")
    if be.device_only:
        torch.cuda.synchronize()
    return o.cpu(), lse.cpu(), dqkv.cpu(), dbias.cpu()


def _perm(windows, indexed):
    T = windows * N
    return torch.randperm(T, generator=torch.Generator().manual_seed(9)) if indexed else torch.arange(T)         # (window, token) j lives in tensor row perm[j]


@pytest.mark.parametrize("windows,heads,nW,indexed", CASES)
def test_window_attention_rows(be, dev, windows, heads, nW, indexed):
    dtype = torch.bfloat16
    q, k, v, g, bias, mask, lb, ref, bnd = case(windows, heads, nW, dtype)
    perm = _perm(windows, indexed)
    scat = lambda t: torch.empty_like(t).index_copy_(0, perm, t)
    qkv = torch.cat([_flat(q), _flat(k), _flat(v)], dim=1).to(dtype)
    o, lse, dqkv, dbias = run_16(be, dev, scat(qkv), scat(_flat(g).to(dtype)), bias, mask, windows, heads, perm if indexed else None)
    o, dqkv = o[perm], dqkv[perm]
    Cc = heads * HD
    what = f"[window bf16 W{windows} H{heads} nW{nW} indexed{int(indexed)}]"
    got = {"o": _rows(o, heads), "dq": _rows(dqkv[:, :Cc], heads), "dk": _rows(dqkv[:, Cc:2 * Cc], heads), "dv": _rows(dqkv[:, 2 * Cc:], heads)}
    ratios = {"lse": rb.check_lse(lse, q, k, SC, ref, what, bias=lb)}
    for kind in rb.KINDS:
        ratios[kind] = rb.check_rows(kind, got[kind], ref, bnd[kind], what)
    e, at = rb.worst(dbias_errors(dbias, ref))
    ratios["dbias"] = e / (bnd["dbias"] / rb.FACTOR)
    print(f"rows {what} dbias: max e_kernel {e:.3e} at {at}, E_or {bnd['dbias'] / rb.FACTOR:.3e}")
    print(f"rows {what} ratios: " + " ".join(f"{n}={x:.2f}" for n, x in ratios.items()))
    assert e <= bnd["dbias"], (what, "dbias", at, e, bnd["dbias"])


@pytest.mark.parametrize("windows,heads,nW,indexed", CASES)
def test_window_attention_f32_rows(be, dev, windows, heads, nW, indexed):
    q, k, v, g, bias, mask, lb, ref, bnd = case(windows, heads, nW, torch.float32)
    perm = _perm(windows, indexed)
    qkv = torch.cat([_flat(q), _flat(k), _flat(v)], dim=1).float()
    o = run_f32(be, dev, torch.empty_like(qkv).index_copy_(0, perm, qkv), bias, mask, windows, heads, perm if indexed else None)[perm]
    what = f"[window f32 W{windows} H{heads} nW{nW} indexed{int(indexed)}]"
    r = rb.check_rows("o", _rows(o, heads), ref, bnd["o"], what)
    print(f"rows {what} ratios: o={r:.2f}")
