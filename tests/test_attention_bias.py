"""Attention with a relative position bias over a whole short sequence (csrc/attention_bias.hip: vdk_attention_bias_fwd / vdk_attention_bias_bwd, N <= 256, head dim 64),
both operand formats, every output bounded by tests/rowbound.py's rule, on the CPU SIMT emulation and on the device.

Inputs: q, v, dout ~ N(0, 1), k ~ 0.7 N(0, 1); bias gathered from a table ~ N(0, 1) through the BEiT index of grid G (tests/beit_ref.py), so the class row and the class
column are constant stripes; with pi = rowbound.permutation(N), k[pi(i)] += q_i c_hi / |q_i|^2 with c_hi = (ln N + 1.5 + 0.5 - bias[h, i, pi(i)]) * 8: the matched logit,
BIAS INCLUDED, sits ln N + 1.5 above a background whose log-sum-exp the unit-variance bias raises by 0.5.  Rows are padded to ld = 3 H 64 + 8 with NaN in the padding.

Precondition, from float64 alone and with no row exempted: every key receives probability >= 0.1 (the 600-item case: >= 0.03) from some query and no row maximum exceeds
0.999.  Sensitivity, from float64 alone: one 32 x 32 bias tile taken from the neighbouring head, or the class column's bias dropped, moves some o row by >= 3 x its bound --
otherwise the test could not tell a biased kernel from the unbiased one.

Checks: o, dq, dk, dv per row and lse per element (rowbound.check_lse) against rowbound.reference64(..., bias=...); the row bound is rowbound.FACTOR x the worst row of the
16-bit restatement (tests/beit_ref.py, the arithmetic the kernel's header states); d(bias) per ELEMENT (class row and class column included) against float64 sum_b dS in
units of sum_b A, bounded by FACTOR x the restatement's worst element; the same bits on two calls; dbias overwritten when pre-filled with NaN; nothing written into the
padding.  VDK_ATTN_GRID=2 runs the small cases with several items per workgroup (the load-add-store path of the d(bias) slab)."""
import ctypes as C
import math

import pytest
import torch

from oracle import bf16ops
from tests import beit_ref
from tests import rowbound as rb
from visiondk_amd import _abi

HD = 64
SC = HD ** -0.5
TINY = 1e-30
BF, HF = torch.bfloat16, torch.float16
DT = {BF: 0, HF: _abi.F16_}            # VDK_BF16, VDK_F16
EINVAL, EWORKSPACE = -1, -2            # VDK_EINVAL, VDK_EWORKSPACE of include/visiondk.h
SEED = 1
# (B, N, H, G): the model's own N (7 tiles, the last holding 5 rows); two tiles with an 8-row DMA tail; a one-row last tile; NKT = 8, the one-wave-per-SIMD forward
CASES = [(2, 197, 3, 14), (3, 37, 2, 6), (2, 65, 2, 8), (1, 226, 2, 15)]
BIG = (300, 197, 2, 14)                # 600 items: more than the resident workgroups, so the persistent loops and the per-head partial sums run over many slots
_CASE = {}


def inputs(B, N, H, G, dtype, seed=SEED):
    """-> q, k, v, g [B, H, N, 64] (float64-typed, rounded to `dtype`), bias f32 [H, N, N]"""
    assert N == G * G + 1
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, N, HD, generator=gen, dtype=torch.float64)
    k = torch.randn(B, H, N, HD, generator=gen, dtype=torch.float64) * 0.7
    v = torch.randn(B, H, N, HD, generator=gen, dtype=torch.float64)
    g = torch.randn(B, H, N, HD, generator=gen, dtype=torch.float64)
    table = torch.randn((2 * G - 1) ** 2 + 3, H, generator=gen)
    bias = beit_ref.gather_bias(table, beit_ref.relative_position_index(G))
    pi = rb.permutation(N)
    c = (math.log(N) + 1.5 + 0.5 - bias[:, torch.arange(N), pi].double()) * math.sqrt(HD)          # [H, N]
    k[:, :, pi] += q * (c[None, :, :, None] / q.pow(2).sum(-1, keepdim=True))
    r = lambda t: t.to(dtype).double()
    return r(q), r(k), r(v), r(g), bias


def reference64(q, k, v, g, bias):
    per = [rb.reference64(q[:, h], k[:, h], v[:, h], g[:, h], SC, bias=bias[h]) for h in range(q.shape[1])]
    ref = {n: torch.stack([p[n] for p in per], dim=1) for n in per[0]}
    ref["dbias"], ref["s_dbias"] = ref["dS"].sum(0), ref["A"].sum(0) + TINY
    return ref


def oracle16(q, k, v, g, bias, dtype):
    with bf16ops.precision(rb.MODE[dtype]):
        q, k, v, g = (t.float() for t in (q, k, v, g))
        o, saved = beit_ref.bias_attention_fwd(q, k, v, SC, bias.float())
        out = beit_ref.bias_attention_bwd(q, k, v, g, SC, saved)
    out["o"] = o
    return out


def dbias_errors(got, ref):
    return (got.double() - ref["dbias"]).abs() / ref["s_dbias"]


def _assert_condition(ref, what, floor):
    P = ref["P"]
    weakest, top = float(P.max(dim=-2).values.min()), float(P.max(dim=-1).values.max())
    print(f"bias rows {what}: weakest key's best probability {weakest:.3f}, largest row maximum {top:.5f}")
    assert weakest >= floor and top <= 0.999, (what, weakest, top)


def _assert_sensitive(q, k, v, g, bias, ref, bnd, what):
    """float64 alone: a bias tile from the neighbouring head / the class column's bias dropped moves some o row by >= 3 x its bound"""
    N, H = bias.shape[-1], bias.shape[0]
    swapped = bias.clone()
    q0, k0 = 32 * ((N - 1) // 64), 32 * ((N - 1) // 32)                 # a middle query tile, the last key tile
    swapped[:, q0:q0 + 32, k0:] = bias.roll(1, 0)[:, q0:q0 + 32, k0:]
    dropped = bias.clone()
    dropped[:, :, 0] = 0.0
    for name, b in (("neighbour head's tile", swapped), ("class column dropped", dropped)):
        o = torch.stack([rb.reference64(q[:, h], k[:, h], v[:, h], g[:, h], SC, bias=b[h])["o"] for h in range(H)], dim=1)
        sig = float(((o - ref["o"]).norm(dim=-1) / ref["s_o"]).max())
        print(f"bias rows {what} sensitivity ({name}): worst o row moves {sig:.3e}, bound {bnd['o']:.3e}")
        assert sig >= rb.SIGNAL_FACTOR * bnd["o"], (what, name, sig, bnd["o"])


def case(B, N, H, G, dtype, floor=0.1):
    key = (B, N, H, G, dtype)
    if key not in _CASE:
        q, k, v, g, bias = inputs(B, N, H, G, dtype)
        ref = reference64(q, k, v, g, bias)
        what = f"B{B} N{N} H{H} {dtype}"
        _assert_condition(ref, what, floor)
        orc = oracle16(q, k, v, g, bias, dtype)
        bnd = rb.bounds(ref, orc)
        bnd["dbias"] = rb.FACTOR * float(dbias_errors(orc["dbias"], ref).max())
        _assert_sensitive(q, k, v, g, bias, ref, bnd, what)
        _CASE[key] = (q, k, v, g, bias, ref, bnd)
    return _CASE[key]


def _flat(t):
    """[B, H, N, 64] -> [B, N, H 64]"""
    B, H, N, _ = t.shape
    return t.transpose(1, 2).reshape(B, N, H * HD)


def _heads(t, H):
    B, N, _ = t.shape
    return t.reshape(B, N, H, HD).transpose(1, 2)


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def run_bias(be, dev, q, k, v, g, bias, dtype, pad=8):
    """-> o [B, H, N, 64], lse [B, H, N], dq, dk, dv, dbias [H, N, N] on the CPU; qkv, o, dout and dqkv rows at pitch + pad with NaN in the padding"""
    B, H, N, _ = q.shape
    D = H * HD
    p = be.ptr
    nan = lambda shape, dt: torch.full(shape, float("nan"), dtype=dt, device=dev)
    qkv = nan((B * N, 3 * D + pad), dtype)
    qkv[:, :3 * D] = torch.cat([_flat(q), _flat(k), _flat(v)], dim=2).reshape(B * N, 3 * D).to(dtype).to(dev)
    dout = nan((B * N, D + pad), dtype)
    dout[:, :D] = _flat(g).reshape(B * N, D).to(dtype).to(dev)
    bd = bias.float().to(dev).contiguous()
    o, lse, dqkv, dbias = nan((B * N, D + pad), dtype), nan((B, H, N), torch.float32), nan((B * N, 3 * D + pad), dtype), nan((H, N, N), torch.float32)
    need = C.c_size_t(0)
    be.check(be.lib.vdk_attention_bias_fwd_workspace_bytes(N, H, C.byref(need)), "bias fwd workspace")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    be.check(be.lib.vdk_attention_bias_fwd(p(qkv), qkv.stride(0), p(o), o.stride(0), p(lse), p(bd), B, N, H, HD, SC, DT[dtype], p(ws), ws.numel(), be.stream()), "bias fwd")
    be.check(be.lib.vdk_attention_bias_bwd_workspace_bytes(B, N, H, C.byref(need)), "bias bwd workspace")
    wb = torch.empty(need.value, dtype=torch.uint8, device=dev)
    be.check(be.lib.vdk_attention_bias_bwd(p(qkv), qkv.stride(0), p(o), p(dout), o.stride(0), p(lse), p(bd), p(dqkv), dqkv.stride(0), p(dbias), B, N, H, HD, SC, DT[dtype],
                                           p(wb), wb.numel(), be.stream()), "bias bwd")
    if be.device_only:
        torch.cuda.synchronize()
    assert bool(torch.isnan(o[:, D:].float()).all()) and bool(torch.isnan(dqkv[:, 3 * D:].float()).all()), "the padding columns of o / dqkv were written"
    o, dqkv = o[:, :D].cpu().reshape(B, N, D), dqkv[:, :3 * D].cpu().reshape(B, N, 3 * D)
    return {"o": _heads(o, H), "lse": lse.cpu(), "dq": _heads(dqkv[..., :D], H), "dk": _heads(dqkv[..., D:2 * D], H), "dv": _heads(dqkv[..., 2 * D:], H), "dbias": dbias.cpu()}


def check_all(got, q, k, bias, ref, bnd, what):
    assert not bool(torch.isnan(got["dbias"]).any()), "dbias (pre-filled with NaN) was not overwritten everywhere"
    rb.check_lse(got["lse"], q, k, SC, ref, what, bias=bias)
    for kind in rb.KINDS:
        rb.check_rows(kind, got[kind], ref, bnd[kind], what)
    e, at = rb.worst(dbias_errors(got["dbias"], ref))
    e_or = bnd["dbias"] / rb.FACTOR
    print(f"bias rows {what} dbias: max e_kernel {e:.3e} at (head, query, key) {at}, E_or {e_or:.3e}, ratio {e / e_or:.2f}")
    assert e <= bnd["dbias"], (what, "dbias", at, e, bnd["dbias"])


def _run_and_check(be, dev, shape, dtype, floor=0.1, what=""):
    q, k, v, g, bias, ref, bnd = case(*shape, dtype, floor=floor)
    got = run_bias(be, dev, q, k, v, g, bias, dtype)
    check_all(got, q, k, bias, ref, bnd, f"[{dtype} {shape}{what}]")
    again = run_bias(be, dev, q, k, v, g, bias, dtype)
    for name in got:
        assert torch.equal(_bits(got[name]), _bits(again[name])), (shape, dtype, name, "two calls differ")


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", CASES, ids=lambda s: "x".join(map(str, s)))
def test_attention_bias_rows(be, dev, shape, dtype):
    _run_and_check(be, dev, shape, dtype)


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", CASES[1:3], ids=lambda s: "x".join(map(str, s)))
def test_attention_bias_rows_several_items_per_workgroup(be, dev, shape, dtype, monkeypatch):
    """two workgroups in all: the forward's persistent loop, and in the backward one workgroup per head that adds every batch item into its d(bias) slab"""
    monkeypatch.setenv("VDK_ATTN_GRID", "2")
    _run_and_check(be, dev, shape, dtype, what=" grid 2")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_attention_bias_rows_600_items(hip, dtype):
    _run_and_check(hip, "cuda", BIG, dtype, floor=0.03)


def test_attention_bias_refusals(be, dev):
    """N = 257, head dims 80 and 32: VDK_EUNSUPPORTED; a misaligned pointer, a pitch that is no multiple of 8: VDK_EINVAL; a workspace one byte short: VDK_EWORKSPACE;
    each with the entry's name in vdk_last_error(), nothing launched"""
    B, N, H = 2, 37, 2
    D = H * HD
    p = be.ptr
    qkv = torch.zeros(B * 257 * 3 * D + 64, dtype=BF, device=dev)
    o, dout, dqkv = torch.zeros(B * 257 * D, dtype=BF, device=dev), torch.zeros(B * 257 * D, dtype=BF, device=dev), torch.zeros(B * 257 * 3 * D, dtype=BF, device=dev)
    lse, bias, dbias = torch.zeros(B, H, 257, device=dev), torch.zeros(H, 257, 257, device=dev), torch.zeros(H, 257, 257, device=dev)
    need = C.c_size_t(0)
    be.check(be.lib.vdk_attention_bias_bwd_workspace_bytes(B, 256, H, C.byref(need)), "bias bwd workspace")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    nf, nb = C.c_size_t(0), C.c_size_t(0)
    be.check(be.lib.vdk_attention_bias_fwd_workspace_bytes(N, H, C.byref(nf)), "bias fwd workspace")
    be.check(be.lib.vdk_attention_bias_bwd_workspace_bytes(B, N, H, C.byref(nb)), "bias bwd workspace")
    assert nf.value == H * 2 * 2 * 4096 and nb.value == nf.value * (1 + B)
    assert be.lib.vdk_attention_bias_fwd_workspace_bytes(257, H, C.byref(nf)) == _abi.EUNSUPPORTED
    assert be.lib.vdk_attention_bias_bwd_workspace_bytes(B, 257, H, C.byref(nb)) == _abi.EUNSUPPORTED

    def fwd(ptr=None, ld=3 * D, n=N, hd=HD, wbytes=None):
        return be.lib.vdk_attention_bias_fwd(p(qkv) if ptr is None else ptr, ld, p(o), D, p(lse), p(bias), B, n, H, hd, SC, 0, p(ws), ws.numel() if wbytes is None else wbytes,
                                             be.stream())

    def bwd(ptr=None, ld=3 * D, n=N, hd=HD, wbytes=None):
        return be.lib.vdk_attention_bias_bwd(p(qkv) if ptr is None else ptr, ld, p(o), p(dout), D, p(lse), p(bias), p(dqkv), 3 * D, p(dbias), B, n, H, hd, SC, 0, p(ws),
                                             ws.numel() if wbytes is None else wbytes, be.stream())

    for fn, name, short in ((fwd, b"vdk_attention_bias_fwd", nf), (bwd, b"vdk_attention_bias_bwd", nb)):
        for rc in (fn(n=257), fn(hd=80), fn(hd=32)):
            assert rc == _abi.EUNSUPPORTED and name in be.lib.vdk_last_error()
        for rc in (fn(ptr=p(qkv) + 2), fn(ld=3 * D + 4)):
            assert rc == EINVAL and name in be.lib.vdk_last_error()
    be.check(be.lib.vdk_attention_bias_fwd_workspace_bytes(N, H, C.byref(nf)), "bias fwd workspace")
    be.check(be.lib.vdk_attention_bias_bwd_workspace_bytes(B, N, H, C.byref(nb)), "bias bwd workspace")
    assert fwd(wbytes=nf.value - 1) == EWORKSPACE and b"vdk_attention_bias_fwd" in be.lib.vdk_last_error()
    assert bwd(wbytes=nb.value - 1) == EWORKSPACE and b"vdk_attention_bias_bwd" in be.lib.vdk_last_error()
    if be.device_only:
        torch.cuda.synchronize()
