"""SwinV2 cosine window attention (csrc/window_attention_cos.hip: vdk_wa_cos_fwd / vdk_wa_cos_bwd, 64-token windows, head dim 32), both operand formats, every output row
bounded (tests/rowbound.py), on the CPU SIMT emulation and on the device.

Inputs (tests/rowbound.py's construction): inside each window and head a perfect matching pi among the keys the window's mask leaves visible to each query is drawn
(see _preference for the order the queries try the keys in), and k[pi(i)] = 0.7 randn + c_h q_i / |q_i|, so that every key of every window is a heavy key of one query.  Three heads with logit_scale = ln 10, ln 16 and ln 200 (the last
is clamped: tau = 100); bias = 16 sigmoid(0.25 randn); a random 0 / -100 mask with an open diagonal (tests/test_swin_window_rows.py's); rows padded to ld = 3 C + 8 with
NaN in the padding.  Precondition, from float64 alone and with no row exempted: in the two unclamped heads every key receives probability >= 0.1 from at least one query
and no query row's maximum exceeds 0.999 (a saturated row has dS = 0 and checks nothing in the backward).

Checks: o, dq, dk, dv per (window, head, token) row against float64 in units of the absolute-value products that went into the row, <= 4 x the worst row of the 16-bit
restatement (tests/swinv2_ref.py, the arithmetic the kernel's header states); d(bias) per element, d(tau) per head and lse per element likewise.  The row scale of dq
is that of d(qn) divided by max(|q|, 1e-12): the Jacobian is a projection (norm <= 1) followed by that division."""
import ctypes as C
import math

import pytest
import torch

from oracle import bf16ops
from tests import rowbound as rb
from tests import swinv2_ref as ref2
from visiondk_amd import _abi

N, HD = 64, 32
TINY = 1e-30
BF, HF = torch.bfloat16, torch.float16
OPF = {BF: 0, HF: 1}
EINVAL, EWORKSPACE = -1, -2           # VDK_EINVAL, VDK_EWORKSPACE of include/visiondk.h
LOGIT_SCALE = (math.log(10.0), math.log(16.0), math.log(200.0))
C_HEAD = (6.0, 3.8, 8.0)        # weight of the matched direction per head: chosen with SEED so that the precondition holds on all four cases (see _assert_condition)
SEED = 4
MARGIN = 2.5                    # target of the matched logit above the rest of its row: probability about 0.92
# (windows, heads, nW, indexed): 9 and 24 items, so a forward workgroup of four waves has a ragged tail
CASES = [(3, 3, 0, False), (3, 3, 0, True), (8, 3, 4, False), (8, 3, 4, True)]
_CASE = {}


def _mask(nW, gen):
    m = torch.where(torch.rand(nW, N, N, generator=gen) < 0.3, torch.full((), -100.0), torch.zeros(()))
    m[:, torch.arange(N), torch.arange(N)] = 0.0
    return m


def _matching(visible, order):
    """a permutation pi with visible[i][pi[i]] for every query i (Kuhn's augmenting paths; `order`: the keys in the order each query tries them)"""
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


def _preference(q, noise, c, tau, lb):
    """the order in which each query tries the keys when the matching is drawn: by how close taking key j would put the matched logit to MARGIN above the logsumexp of the
    query's other logits, the latter estimated from the keys' noise directions alone.  With a matching drawn uniformly the matched probabilities of a tau = 16 head spread
    over more than the [0.1, 0.999] the precondition allows (bias +-3, the cosine of the noise, the query's background); this order takes the bias and the noise of the
    matched pair out of that spread.  q, noise [64, 32] float64, lb [64, 64] bias + mask"""
    u = q / q.norm(dim=-1, keepdim=True)
    kij = noise[None, :, :] + c * u[:, None, :]                                             # key j if query i took it
    matched = tau * (kij * u[:, None, :]).sum(-1) / kij.norm(dim=-1) + lb
    background = torch.logsumexp(tau * (u @ (noise / noise.norm(dim=-1, keepdim=True)).T) + lb, -1, keepdim=True)
    return ((matched - background - MARGIN).abs()).argsort(dim=-1).tolist()


def inputs(windows, heads, nW, dtype, seed=SEED):
    """-> q, k, v, g [windows, heads, 64, 32] (float64-typed, rounded to `dtype`), logit_scale [heads], bias [heads, 64, 64], mask [nW, 64, 64] | None"""
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(windows, heads, N, HD, generator=gen, dtype=torch.float64)
    k = torch.randn(windows, heads, N, HD, generator=gen, dtype=torch.float64) * 0.7
    v = torch.randn(windows, heads, N, HD, generator=gen, dtype=torch.float64)
    bias = 16.0 * torch.sigmoid(0.25 * torch.randn(heads, N, N, generator=gen))
    mask = _mask(nW, gen) if nW else None
    tau = ref2.tau_of(torch.tensor(LOGIT_SCALE[:heads])).double()
    for w in range(windows):
        vis = (mask[w % nW] == 0) if nW else torch.ones(N, N, dtype=torch.bool)
        for h in range(heads):
            pi = _matching(vis.tolist(), _preference(q[w, h], k[w, h], C_HEAD[h], float(tau[h]), bias[h].double() + (mask[w % nW].double() if nW else 0.0)))
            k[w, h, pi] += C_HEAD[h] * q[w, h] / q[w, h].norm(dim=-1, keepdim=True)
    g = torch.randn(windows, heads, N, HD, generator=torch.Generator().manual_seed(100 + seed), dtype=torch.float64)
    r = lambda t: t.to(dtype).double()
    return r(q), r(k), r(v), r(g), torch.tensor(LOGIT_SCALE[:heads]), bias, mask


def logit_bias(bias, mask, windows):
    b = bias[None].double()
    return b if mask is None else b + mask[torch.arange(windows) % mask.shape[0]][:, None].double()


def reference64(q, k, v, g, tau, lb):
    """float64 on the given 16-bit-valued inputs: tests/rowbound.py's reference per head on the unrounded unit vectors with sc = tau_h, then the Jacobian of the
    normalisation; plus d(bias), d(tau) and their scales"""
    qd, kd = q.norm(dim=-1, keepdim=True).clamp_min(ref2.EPS), k.norm(dim=-1, keepdim=True).clamp_min(ref2.EPS)
    qn, kn = q / qd, k / kd
    per = [rb.reference64(qn[:, h], kn[:, h], v[:, h], g[:, h], float(tau[h]), bias=lb[:, h]) for h in range(q.shape[1])]
    ref = {n: torch.stack([p[n] for p in per], dim=1) for n in per[0]}
    ref["dq"] = (ref["dq"] - qn * (qn * ref["dq"]).sum(-1, keepdim=True)) / qd
    ref["dk"] = (ref["dk"] - kn * (kn * ref["dk"]).sum(-1, keepdim=True)) / kd
    ref["s_dq"] = ref["s_dq"] / qd.squeeze(-1)
    ref["s_dk"] = ref["s_dk"] / kd.squeeze(-1)
    cos = qn @ kn.transpose(-2, -1)
    ref["dbias"], ref["s_dbias"] = ref["dS"].sum(0), ref["A"].sum(0) + TINY
    ref["dtau"], ref["s_dtau"] = (ref["dS"] * cos).sum((0, 2, 3)), (ref["A"] * (qn.abs() @ kn.abs().transpose(-2, -1))).sum((0, 2, 3))
    return ref


def oracle16(q, k, v, g, tau, lb, dtype):
    with bf16ops.precision(rb.MODE[dtype]):
        q, k, v, g = (t.float() for t in (q, k, v, g))
        o, saved = ref2.cos_attention_fwd(q, k, v, tau.float(), lb.float())
        out = ref2.cos_attention_bwd(q, k, v, g, tau.float(), saved)
    out["o"], out["lse"] = o, saved["lse"]
    return out


def _assert_condition(ref, what):
    """float64 alone, the two unclamped heads, no row exempted"""
    P = ref["P"][:, :2]
    weakest, top = float(P.max(dim=-2).values.min()), float(P.max(dim=-1).values.max())
    print(f"cos rows {what}: weakest key's best probability {weakest:.3f}, largest row maximum {top:.5f}")
    assert weakest >= 0.1 and top <= 0.999, (what, weakest, top)


def extra_errors(kind, got, ref):
    return (got.double() - ref[kind]).abs() / ref["s_" + kind]


def bounds_of(ref, orc):
    bnd = rb.bounds(ref, orc)
    for kind in ("dbias", "dtau"):
        bnd[kind] = rb.FACTOR * float(extra_errors(kind, orc[kind], ref).max())
    bnd["lse"] = rb.FACTOR * (orc["lse"].double() - ref["lse"]).abs().amax(dim=(0, 2))          # per head
    return bnd


def case(windows, heads, nW, dtype):
    key = (windows, heads, nW, dtype)
    if key not in _CASE:
        q, k, v, g, ls, bias, mask = inputs(windows, heads, nW, dtype)
        tau = ref2.tau_of(ls)
        lb = logit_bias(bias, mask, windows)
        ref = reference64(q, k, v, g, tau.double(), lb)
        _assert_condition(ref, f"W{windows} H{heads} nW{nW} {dtype}")
        _CASE[key] = (q, k, v, g, ls, tau, bias, mask, lb, ref, bounds_of(ref, oracle16(q, k, v, g, tau, lb, dtype)))
    return _CASE[key]


def _rows(t, heads):
    """[windows * 64, heads * 32] -> [windows, heads, 64, 32]"""
    return t.reshape(-1, N, heads, HD).transpose(1, 2)


def _flat(t):
    W, H = t.shape[:2]
    return t.transpose(1, 2).reshape(W * N, H * HD)


def _padded(x, pad, dev):
    """the rows of x at pitch cols + pad, NaN between them"""
    buf = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), dtype=x.dtype, device=dev)
    buf[:, :x.shape[1]] = x.to(dev)
    return buf


def run_cos(be, dev, qkv, dout, tau, bias, mask, windows, heads, rowidx, pad=8):
    """-> o [T, C], lse [W, H, 64], dqkv [T, 3 C], dbias [H, 64, 64], dtau [H] on the CPU"""
    Cc = heads * HD
    nW = 0 if mask is None else mask.shape[0]
    p = be.ptr
    qd, gd = _padded(qkv, pad, dev), dout.to(dev).contiguous()
    td, bd = tau.float().to(dev).contiguous(), bias.float().to(dev).contiguous()
    md = None if mask is None else mask.float().to(dev).contiguous()
    rd = None if rowidx is None else rowidx.to(torch.int32).to(dev)
    nan = lambda shape, dt: torch.full(shape, float("nan"), dtype=dt, device=dev)
    o, lse, dqkv = nan((windows * N, Cc), qkv.dtype), nan((windows, heads, N), torch.float32), nan((windows * N, 3 * Cc + pad), qkv.dtype)
    dbias, dtau = nan((heads, N, N), torch.float32), nan((heads,), torch.float32)
    opf = OPF[qkv.dtype]
    need = C.c_size_t(0)
    be.check(be.lib.vdk_wa_cos_fwd_workspace_bytes(nW, heads, C.byref(need)), "cos fwd workspace")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    be.check(be.lib.vdk_wa_cos_fwd(p(qd), qd.stride(0), p(o), Cc, p(lse), p(td), p(bd), p(md), nW, windows, heads, p(rd), opf, p(ws), ws.numel(), be.stream()), "cos fwd")
    be.check(be.lib.vdk_wa_cos_bwd_workspace_bytes(windows, nW, heads, C.byref(need)), "cos bwd workspace")
    wb = torch.empty(need.value, dtype=torch.uint8, device=dev)
    be.check(be.lib.vdk_wa_cos_bwd(p(qd), qd.stride(0), p(o), p(gd), Cc, p(lse), p(td), p(bd), p(md), nW, windows, heads, p(rd), p(dqkv), dqkv.stride(0), p(dbias), p(dtau),
                                   opf, p(wb), wb.numel(), be.stream()), "cos bwd")
    if be.device_only:
        torch.cuda.synchronize()
    assert bool(torch.isnan(dqkv[:, 3 * Cc:].float()).all()), "the padding columns of dqkv were written"
    return o.cpu(), lse.cpu(), dqkv[:, :3 * Cc].cpu(), dbias.cpu(), dtau.cpu()


def _perm(windows, indexed):
    T = windows * N
    return torch.randperm(T, generator=torch.Generator().manual_seed(9)) if indexed else torch.arange(T)         # (window, token) j lives in tensor row perm[j]


def _split(o, dqkv, heads):
    Cc = heads * HD
    return {"o": _rows(o, heads), "dq": _rows(dqkv[:, :Cc], heads), "dk": _rows(dqkv[:, Cc:2 * Cc], heads), "dv": _rows(dqkv[:, 2 * Cc:], heads)}


def check_all(got, lse, dbias, dtau, q, k, tau, lb, ref, bnd, what):
    ratios = {}
    # lse: the logits carry the rounding of qn and kn (tau 2^-9 per unit of cosine in bf16), so float32 logsumexp of the unrounded unit vectors (rowbound.check_lse) is no
    # measure; per head, element by element: <= 4 x the restatement's worst element, like the rows
    err = (lse.double() - ref["lse"]).abs().amax(dim=(0, 2))
    for h in range(q.shape[1]):
        e_or = float(bnd["lse"][h]) / rb.FACTOR
        ratios[f"lse{h}"] = float(err[h]) / e_or
        print(f"cos rows {what} lse head {h} (tau {float(tau[h]):.0f}): max |err| {float(err[h]):.3e}, E_or {e_or:.3e}")
        assert float(err[h]) <= float(bnd["lse"][h]), (what, "lse", h, float(err[h]), float(bnd["lse"][h]))
    for kind in rb.KINDS:
        ratios[kind] = rb.check_rows(kind, got[kind], ref, bnd[kind], what)
    for kind, t in (("dbias", dbias), ("dtau", dtau)):
        e, at = rb.worst(extra_errors(kind, t, ref))
        e_or = bnd[kind] / rb.FACTOR
        print(f"cos rows {what} {kind}: max e_kernel {e:.3e} at {at}, E_or {e_or:.3e}, ratio {e / e_or:.2f}")
        assert e <= bnd[kind], (what, kind, at, e, bnd[kind])
    print(f"cos rows {what} ratios: " + " ".join(f"{n}={x:.2f}" for n, x in ratios.items()))


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("windows,heads,nW,indexed", CASES)
def test_window_attention_cos_rows(be, dev, windows, heads, nW, indexed, dtype):
    q, k, v, g, ls, tau, bias, mask, lb, ref, bnd = case(windows, heads, nW, dtype)
    perm = _perm(windows, indexed)
    scat = lambda t: torch.empty_like(t).index_copy_(0, perm, t)
    qkv, dout = torch.cat([_flat(q), _flat(k), _flat(v)], dim=1).to(dtype), _flat(g).to(dtype)
    o, lse, dqkv, dbias, dtau = run_cos(be, dev, scat(qkv), scat(dout), tau, bias, mask, windows, heads, perm if indexed else None)
    o, dqkv = o[perm], dqkv[perm]
    what = f"[{dtype} W{windows} H{heads} nW{nW} indexed{int(indexed)}]"
    check_all(_split(o, dqkv, heads), lse, dbias, dtau, q, k, tau, lb, ref, bnd, what)
    if indexed:           # the row index is addressing only: the same bits as the same data in (window, token) order
        o2, lse2, dqkv2, dbias2, dtau2 = run_cos(be, dev, qkv, dout, tau, bias, mask, windows, heads, None)
        for name, a, b in (("o", o, o2), ("lse", lse, lse2), ("dqkv", dqkv, dqkv2), ("dbias", dbias, dbias2), ("dtau", dtau, dtau2)):
            assert torch.equal(a.view(torch.int16 if a.element_size() == 2 else torch.int32), b.view(torch.int16 if b.element_size() == 2 else torch.int32)), (what, name)


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_logit_scale_gradient_clamp(be, dev, dtype):
    """d(logit_scale_h) = d(tau_h) tau_h [logit_scale_h <= ln 100] (visiondk_amd.swinv2.logit_scale_grad, torch.clamp's rule): exactly 0 for the clamped head, and passed
    on, non-zero, where logit_scale == ln 100 exactly"""
    from visiondk_amd import swinv2
    windows, heads = 3, 3
    q, k, v, g, ls, tau, bias, mask, lb, ref, bnd = case(windows, heads, 0, dtype)
    qkv, dout = torch.cat([_flat(q), _flat(k), _flat(v)], dim=1).to(dtype), _flat(g).to(dtype)
    ls_b = torch.tensor([LOGIT_SCALE[0], LOGIT_SCALE[1], ref2.LOGIT_MAX])
    assert torch.equal(swinv2.tau_of(ls), ref2.tau_of(ls)) and torch.equal(swinv2.tau_of(ls_b), swinv2.tau_of(ls))      # ln 200 and ln 100 give the same tau: one kernel run
    *_, dtau = run_cos(be, dev, qkv, dout, swinv2.tau_of(ls), bias, None, windows, heads, None)
    d = swinv2.logit_scale_grad(dtau, ls)
    d_b = swinv2.logit_scale_grad(dtau, ls_b)
    lsb = ls_b.clone().requires_grad_(True)
    torch.exp(torch.clamp(lsb, max=ref2.LOGIT_MAX)).backward(dtau)
    print(f"cos logit_scale grad {dtype}: dtau {dtau.tolist()} clamped {d.tolist()} boundary {d_b.tolist()} torch {lsb.grad.tolist()}")
    assert float(dtau[2]) != 0.0 and float(d[2]) == 0.0 and float(d[0]) != 0.0 and float(d[1]) != 0.0
    assert float(d_b[2]) != 0.0 and torch.equal(d_b, lsb.grad)


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_window_attention_cos_zero_rows(be, dev, dtype):
    """One all-zero q row and one all-zero k row in a window: qn = 0 (F.normalize), the query's logits are its bias row, and everything is finite and within the bounds of
    the same restatement.  The zero rows' OWN gradients are d(qn) / 1e-12 (torch's rule as well): about 1e10 in the unclamped heads, inside bf16's range and beyond fp16's,
    where the kernel must store what rounding the float64 value to fp16 gives (+-inf); every other row is finite in both formats."""
    windows, heads = 3, 3
    q, k, v, g, ls, bias, mask = inputs(windows, heads, 0, dtype)
    q, k = q.clone(), k.clone()
    q[1, :, 5] = 0.0
    k[1, :, 9] = 0.0
    tau = ref2.tau_of(ls)
    lb = logit_bias(bias, None, windows)
    ref = reference64(q, k, v, g, tau.double(), lb)
    own = {"dq": (1, slice(None), 5), "dk": (1, slice(None), 9)}
    orc = oracle16(q, k, v, g, tau, lb, dtype)
    qkv, dout = torch.cat([_flat(q), _flat(k), _flat(v)], dim=1).to(dtype), _flat(g).to(dtype)
    o, lse, dqkv, dbias, dtau = run_cos(be, dev, qkv, dout, tau, bias, None, windows, heads, None)
    got = _split(o, dqkv, heads)
    assert bool(torch.isfinite(got["o"].float()).all()) and bool(torch.isfinite(got["dv"].float()).all()) and bool(torch.isfinite(lse).all())
    assert bool(torch.isfinite(dbias).all()) and bool(torch.isfinite(dtau).all())
    # the zero rows' own gradients, per head: the elements beyond the format's range are +-inf of the right sign (elements within the restatement's own error of the edge
    # may fall either side), the others within 4 x the restatement's error on the same row
    top = float(torch.finfo(dtype).max)
    for kind, at in own.items():
        r, s_row = ref[kind][at], ref["s_" + kind][at][..., None]
        e_or = ((orc[kind][at].double() - r).abs() / s_row).nan_to_num(posinf=0.0)
        tol = rb.FACTOR * e_or.amax(dim=-1, keepdim=True) * s_row
        gi, gk = torch.isinf(got[kind][at]), got[kind][at].double()
        big, small = r.abs() > top + tol, r.abs() < top - tol
        assert bool(big.any()) == (dtype == HF), "d(qn) / 1e-12 was expected inside bf16's range and beyond fp16's"
        assert bool(gi[big].all()) and not bool(gi[small].any()) and torch.equal(torch.sign(gk)[big], torch.sign(r)[big]), kind
        if bool(small.any()):
            err = ((gk - r).abs() / s_row)[small]
            print(f"cos zero rows {dtype} {kind}: own rows max scaled error {float(err.max()):.3e}, restatement {float(e_or[small].max()):.3e}")
            assert bool((err <= (tol / s_row).expand_as(r)[small] + 2.0 ** -24).all()), kind
        # every other row: bounds and comparison with the own rows taken out (the same finite values there in the reference, the restatement and the result)
        out = r.to(dtype).double().nan_to_num(posinf=0.0, neginf=0.0)
        ref[kind], got[kind], orc[kind] = ref[kind].clone(), got[kind].clone(), orc[kind].clone()
        ref[kind][at], got[kind][at], orc[kind][at] = out, out.to(dtype), out.float()
    bnd = bounds_of(ref, orc)
    for kind in ("dq", "dk"):
        assert bool(torch.isfinite(got[kind].float()).all()), kind
    check_all(got, lse, dbias, dtau, q, k, tau, lb, ref, bnd, f"[zero rows {dtype}]")


def test_window_attention_cos_refusals(be, dev):
    """misaligned pointer (the workspace included), ld < 3 C, windows % nW != 0: VDK_EINVAL with a text, nothing launched; the public 49-token entries still refuse N = 64"""
    windows, heads = 8, 3
    Cc = heads * HD
    p = be.ptr
    qkv = torch.zeros(windows * N * 3 * Cc + 64, dtype=BF, device=dev)
    o = torch.zeros(windows * N, Cc, dtype=BF, device=dev)
    lse = torch.zeros(windows, heads, N, device=dev)
    tau, bias, mask = torch.ones(heads, device=dev), torch.zeros(heads, N, N, device=dev), torch.zeros(4, N, N, device=dev)
    ws = torch.empty(4 * heads * 4096 * 4, dtype=torch.uint8, device=dev)

    def fwd(ptr=None, ld=3 * Cc, W=windows, m=mask, nW=4, wsoff=0):
        return be.lib.vdk_wa_cos_fwd(p(qkv) if ptr is None else ptr, ld, p(o), Cc, p(lse), p(tau), p(bias), p(m), nW, W, heads, None, 0, p(ws) + wsoff, ws.numel() - wsoff,
                                     be.stream())

    for rc in (fwd(ptr=p(qkv) + 2), fwd(ld=3 * Cc - 8), fwd(W=7), fwd(ld=3 * Cc + 4), fwd(nW=1, wsoff=8)):
        assert rc == EINVAL and b"vdk_wa_cos_fwd" in be.lib.vdk_last_error()
    dqkv, dbias, dtau = torch.zeros(windows * N, 3 * Cc, dtype=BF, device=dev), torch.zeros(heads, N, N, device=dev), torch.zeros(heads, device=dev)
    need = C.c_size_t(0)
    be.check(be.lib.vdk_wa_cos_bwd_workspace_bytes(windows, 4, heads, C.byref(need)), "cos bwd workspace")
    wb = torch.empty(need.value, dtype=torch.uint8, device=dev)

    def bwd(ptr=None, ld=3 * Cc, W=windows, wbytes=None):
        return be.lib.vdk_wa_cos_bwd(p(qkv) if ptr is None else ptr, ld, p(o), p(o), Cc, p(lse), p(tau), p(bias), p(mask), 4, W, heads, None, p(dqkv), 3 * Cc, p(dbias), p(dtau), 0,
                                     p(wb), wb.numel() if wbytes is None else wbytes, be.stream())

    for rc in (bwd(ptr=p(qkv) + 2), bwd(ld=3 * Cc - 8), bwd(W=7)):
        assert rc == EINVAL and b"vdk_wa_cos_bwd" in be.lib.vdk_last_error()
    assert bwd(wbytes=need.value - 1) == EWORKSPACE
    rc = be.lib.vdk_window_attention_fwd(p(qkv), 3 * Cc, p(o), Cc, p(lse), p(bias), None, 0, windows, heads, N, HD, 1.0, None, p(ws), ws.numel(), be.stream())
    assert rc == _abi.EUNSUPPORTED
    if be.device_only:
        torch.cuda.synchronize()
