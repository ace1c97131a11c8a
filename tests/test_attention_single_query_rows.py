"""The one-query attention kernels, every output row bounded (tests/rowbound.py): the class-query kernels of csrc/attention_cls.hip through their test hooks
(tests/test_vit_cls_attn.py) and the attention pooling kernels of csrc/attn_pool.hip at head dims 64, 72 and 80 (tests/test_attn_pool_hd.py), bf16 and fp16, on the CPU
SIMT emulation and on the device.

With one query every dK_j / dV_j row has exactly one contributor, so a key row that is dropped, duplicated or written to the wrong place is wrong in full -- and costs the
whole-tensor norms of the existing tests 1 / sqrt(N).  Here dk and dv are bounded on EVERY row, o and the query gradient on theirs, lse (the pooling kernels: the
probabilities) element by element.  Inputs: k = 0.7 randn with three planted keys -- the first, the last and one at a pass edge -- at ln N above the rest, so that each of
them holds about a quarter of the mass and the forward and the query gradient notice when one is ignored (asserted from float64 before a kernel result is looked at).

Oracles.  Class query: oracle/bf16ops.py in the case's 16-bit mode (the kernels keep the rounding points of the full-size ones: P once, o once, dS once, 16-bit
gradients).  Pooling: q, dout, the probabilities, out and dq are fp32 and the kernels round nothing but the dk / dv rows they store (csrc/attn_pool.hip), so the oracle is
the same formula in float32 torch with dk and dv rounded to the operand format."""
import pytest
import torch

from tests import rowbound as rb
from tests.test_attn_pool_hd import run_hd as run_pool
from tests.test_vit_cls_attn import _run as run_cls

FMT = {"bf16": torch.bfloat16, "fp16": torch.float16}
# class query (B, H, N, hd, grid): one key; the test model (6 items: not a multiple of the 4 waves of a workgroup); one key past a pass group of 32 at head dim 64 and of 16 at
# head dim 80; one key past 64; the flagship's N; head dim 80 past 256 keys; and two of them with a single workgroup, so that a wave walks over several items
CLS_SHAPES = [(2, 1, 1, 64, 0), (3, 2, 17, 64, 0), (2, 2, 33, 64, 0), (2, 2, 17, 80, 0), (2, 3, 65, 64, 0), (1, 3, 197, 64, 0), (2, 2, 257, 80, 0), (3, 2, 17, 64, 1), (2, 2, 257, 80, 1)]
# pooling (B, N, H): the shapes of tests/test_attn_pool_hd.py
POOL_SHAPES = [(3, 37, 2), (1, 1, 1), (2, 256, 3), (1, 260, 2)]
_CASE = {}


def _flat(t):
    """[B, H, n, hd] -> [B, n, H hd]"""
    B, H, n, hd = t.shape
    return t.transpose(1, 2).reshape(B, n, H * hd)


def _sensitive(ref, inp, sc, planted, bnd, what):
    """from float64 alone: ignoring a planted key breaks the o bound; a dv row that is lost breaks its bound on every row, a dk row on >= 80 % of the rows (dS_j = P_j (dP_j - D)
    can cancel by chance) and on every planted one or its neighbour"""
    if rb.ref_is_trivial(ref):
        return
    q, k, v, g = inp
    kj = torch.tensor(planted)
    qi = torch.zeros_like(kj)
    so = rb.signals("o", ref, q, k, v, g, sc, qi, kj)
    lost = {kind: ref[kind].norm(dim=-1) / ref["s_" + kind] for kind in ("dk", "dv")}
    cov_dk = lost["dk"] >= rb.SIGNAL_FACTOR * bnd["dk"]
    print(f"rows {what}: planted keys {planted} hold {[round(float(x), 2) for x in ref['P'][0, 0, 0, kj]]}, o signal >= {float(so.min()):.2f}; a lost dv row >= {float(lost['dv'].min()):.2f}, "
          f"a lost dk row stands out in {100 * float(cov_dk.double().mean()):.1f} %")
    assert bool((so >= rb.SIGNAL_FACTOR * bnd["o"]).all())
    assert bool((lost["dv"] >= rb.SIGNAL_FACTOR * bnd["dv"]).all())
    assert float(cov_dk.double().mean()) >= 0.8
    N = k.shape[-2]
    for j in planted:
        assert bool(cov_dk[..., max(j - 1, 0):min(j + 2, N)].reshape(-1, min(j + 2, N) - max(j - 1, 0)).any(0).any()), j


def cls_case(B, H, N, hd, fmt):
    key = ("cls", B, H, N, hd, fmt)
    if key not in _CASE:
        dtype, sc = FMT[fmt], hd ** -0.5
        q, k, v, g, planted = rb.single_query_inputs(B, N, H, hd, dtype, 21, edge=32 if hd == 64 else 16)
        ref = rb.reference64(q, k, v, g, sc)
        bnd = rb.bounds(ref, rb.oracle16(q, k, v, g, sc, dtype))
        _sensitive(ref, (q, k, v, g), sc, planted, bnd, f"cls B{B} H{H} N{N} hd{hd} {fmt}")
        gen = torch.Generator().manual_seed(22)
        qrows = torch.randn(B, N, H * hd, generator=gen, dtype=torch.float64)                # the other rows' q: the kernels must not read them
        qrows[:, :1] = _flat(q)
        qkv = torch.cat([qrows, _flat(k), _flat(v)], dim=2).to(dtype)
        dout = torch.zeros(B, N, H * hd, dtype=torch.float64)
        dout[:, :1] = _flat(g)
        _CASE[key] = (qkv, dout.to(dtype), (q, k, v, g), ref, bnd)
    return _CASE[key]


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("B,H,N,hd,grid", CLS_SHAPES)
def test_cls_kernels_rows(be, dev, B, H, N, hd, grid, fmt):
    qkv, dout, (q, k, v, g), ref, bnd = cls_case(B, H, N, hd, fmt)
    r = run_cls(be, dev, "cls", qkv, dout, H, hd, fmt, grid=grid)
    D, sc = H * hd, hd ** -0.5
    what = f"[cls hd{hd} {fmt} B{B} H{H} N{N} grid{grid}]"
    got = {"o": rb.heads_of(r["o"][:, :1], H), "dq": rb.heads_of(r["dqkv"][:, :1, :D], H), "dk": rb.heads_of(r["dqkv"][..., D:2 * D], H), "dv": rb.heads_of(r["dqkv"][..., 2 * D:], H)}
    ratios = {"lse": rb.check_lse(r["lse"][:, :, :1], q, k, sc, ref, what)}
    for kind in rb.KINDS:
        ratios[kind] = rb.check_rows(kind, got[kind], ref, bnd[kind], what)
    print(f"rows {what} ratios: " + " ".join(f"{n}={x:.2f}" for n, x in ratios.items()))


def _pool_oracle(q, k, v, g, sc, dtype):
    """the formula of csrc/attn_pool.hip in float32 torch; the kernels' only roundings are the stored dk and dv rows"""
    q, k, v = (t.float().clone().requires_grad_(True) for t in (q, k, v))
    p = torch.softmax((q * sc) @ k.transpose(-2, -1), dim=-1)
    o = p @ v
    o.backward(g.float())
    r16 = lambda t: t.to(dtype).float()
    return {"o": o.detach(), "dq": q.grad, "dk": r16(k.grad), "dv": r16(v.grad), "p": p.detach()}


def pool_case(B, N, H, hd, fmt):
    key = ("pool", B, N, H, hd, fmt)
    if key not in _CASE:
        dtype, sc = FMT[fmt], hd ** -0.5
        q, k, v, g, planted = rb.single_query_inputs(B, N, H, hd, dtype, 31, edge=256, shared_q=True, qg_dtype=torch.float32)
        ref = rb.reference64(q, k, v, g, sc)
        orc = _pool_oracle(q, k, v, g, sc, dtype)
        rel_p, o_floor = rb.fp32_forward_floor(q, k, sc)
        bnd = rb.bounds(ref, orc, o_floor=o_floor)
        # the probabilities, element by element, as lse is bounded: LSE_FACTOR x max(E32, eps32 p64), E32 the worst absolute error of the float32 torch softmax; and at
        # least the fp32 accumulation bound of a score
        e32 = float((orc["p"].double() - ref["P"]).abs().max())
        pb = torch.maximum(rb.LSE_FACTOR * torch.maximum(torch.full_like(ref["P"], e32), torch.finfo(torch.float32).eps * ref["P"]), rel_p * ref["P"])
        _sensitive(ref, (q, k, v, g), sc, planted, bnd, f"pool B{B} N{N} H{H} hd{hd} {fmt}")
        kv = torch.cat([_flat(k), _flat(v)], dim=2).reshape(B * N, 2 * H * hd).to(dtype)
        _CASE[key] = (q[0].reshape(-1).float(), kv, _flat(g)[:, 0].float(), (q, k, v, g), ref, bnd, pb)
    return _CASE[key]


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("hd", [64, 72, 80])
@pytest.mark.parametrize("B,N,H", POOL_SHAPES)
def test_attn_pool_rows(be, dev, B, N, H, hd, fmt):
    """head dim 64 through the public vdk_attn_pool_fwd_dt / bwd_dt, 72 and 80 through the _hd entries (the same kernels, tests/test_attn_pool_hd.py)"""
    qf, kv, dout, inp, ref, bnd, pb = pool_case(B, N, H, hd, fmt)
    out, probs, dkv, dq_part = run_pool(be, dev, qf, kv, dout, B, N, H, hd, entry="dt" if hd == 64 else "hd")
    D = H * hd
    what = f"[pool hd{hd} {fmt} B{B} N{N} H{H}]"
    dkv = dkv.reshape(B, N, 2 * D)
    got = {"o": rb.heads_of(out[:, None], H), "dq": rb.heads_of(dq_part[:, None], H), "dk": rb.heads_of(dkv[..., :D], H), "dv": rb.heads_of(dkv[..., D:], H)}
    perr = (probs.double()[:, :, None] - ref["P"]).abs() / pb
    m, at = rb.worst(perr)
    print(f"rows {what} probs: worst err / bound {m:.3f}")
    assert m <= 1.0, (what, "probs", at)
    ratios = {"probs/bound": m}
    for kind in rb.KINDS:
        ratios[kind] = rb.check_rows(kind, got[kind], ref, bnd[kind], what)
    print(f"rows {what} ratios: " + " ".join(f"{n}={x:.2f}" for n, x in ratios.items()))
