"""The one-query attention of AttentionPoolLatent (csrc/attn_pool.hip) with the head dimension as an argument: vdk_attn_pool_fwd_hd / vdk_attn_pool_bwd_hd of
csrc/vdk_internal.h at head dims 64, 72 (SigLIP SO400M: 1152 / 16) and 80.  At 64 they are the kernels of the public vdk_attn_pool_*_dt entries, bit for bit; 72 and 80
are checked against the attention step of oracle/vit_ref.AttentionPoolLatentRef in torch fp32 on the same 16-bit-rounded kv."""
import pytest
import torch

from tests.extent import run_isolated
from visiondk_amd import _abi

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
DT = {BF: 0, HF: 2}
# the shape of tests/test_siglip.py::test_attention_pool_alone_vs_oracle; one key; the SO400M sequence length (every thread of the score pass has exactly one key) with an
# odd head count; more than 256 keys: a thread's second pass
SHAPES = [(3, 37, 2), (1, 1, 1), (2, 256, 3), (1, 260, 2)]


def p(t):
    return t.data_ptr()


def _rel(a, b):
    return ((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-30)).item()


def make_inputs(B, N, H, hd, dtype, seed=0):
    torch.manual_seed(seed)
    D = H * hd
    q = torch.randn(D)
    kv = torch.randn(B * N, 2 * D).to(dtype)
    dout = torch.randn(B, D)
    return q, kv, dout


def run_hd(be, dev, q, kv, dout, B, N, H, hd, entry="hd"):
    """forward and backward on contiguous operands -> (out, probs, dkv, dq_part) on the CPU; entry "dt": the public head-dim-64 entries"""
    D = H * hd
    scale = hd ** -0.5
    dt = DT[kv.dtype]
    q, kv, dout = q.to(dev), kv.to(dev), dout.to(dev)
    out = torch.empty((B, D), dtype=F32, device=dev); probs = torch.empty((B, H, N), dtype=F32, device=dev)
    dkv = torch.empty_like(kv); dq_part = torch.empty((B, D), dtype=F32, device=dev)
    if entry == "hd":
        be.check(be.lib.vdk_attn_pool_fwd_hd(p(q), p(kv), 2 * D, B, N, H, hd, scale, p(out), D, p(probs), dt, be.stream()), "attn_pool_fwd_hd")
        be.check(be.lib.vdk_attn_pool_bwd_hd(p(q), p(kv), 2 * D, p(probs), p(dout), D, B, N, H, hd, scale, p(dkv), 2 * D, p(dq_part), dt, be.stream()), "attn_pool_bwd_hd")
    else:
        assert hd == 64
        be.check(be.lib.vdk_attn_pool_fwd_dt(p(q), p(kv), 2 * D, B, N, H, scale, p(out), D, p(probs), dt, be.stream()), "attn_pool_fwd_dt")
        be.check(be.lib.vdk_attn_pool_bwd_dt(p(q), p(kv), 2 * D, p(probs), p(dout), D, B, N, H, scale, p(dkv), 2 * D, p(dq_part), dt, be.stream()), "attn_pool_bwd_dt")
    return out.cpu(), probs.cpu(), dkv.cpu(), dq_part.cpu()


def reference(q, kv, dout, B, N, H, hd):
    """AttentionPoolLatentRef.forward's attention step (softmax((q * scale) k^T) v) in fp32 on the rounded kv, and its gradients"""
    D = H * hd
    qr = q.clone().requires_grad_(True)
    kvr = kv.float().clone().requires_grad_(True)
    k, v = kvr.reshape(B, N, 2, H, hd).permute(2, 0, 3, 1, 4).unbind(0)          # [B, H, N, hd]
    a = torch.softmax((qr.reshape(1, H, 1, hd) * hd ** -0.5) @ k.transpose(-2, -1), dim=-1)
    out = (a @ v).transpose(1, 2).reshape(B, D)
    out.backward(dout)
    return out.detach(), a.detach().reshape(B, H, N), kvr.grad, qr.grad


def check_vs_reference(q, kv, dout, B, N, H, hd, out, probs, dkv, dq_part, what=""):
    """the bounds of tests/test_siglip.py::test_attention_pool_alone_vs_oracle: 3e-3 on the output, 1e-2 on the gradients"""
    D = H * hd
    o_r, a_r, dkv_r, dq_r = reference(q, kv, dout, B, N, H, hd)
    dq = dq_part.sum(0)
    dk, dv, dk_r, dv_r = dkv[:, :D].float(), dkv[:, D:].float(), dkv_r[:, :D], dkv_r[:, D:]
    if N == 1:
        # one key: P = 1 and dS = dP - sum(P dP) = 0, so dk = dq = 0 exactly and a relative error has no denominator.  What the kernel leaves is measured against the
        # un-cancelled magnitude scale * sum_i |dout_i v_i| * |q| (resp. |k|) of the terms that cancel
        assert float(dk_r.abs().max()) < 1e-6 and float(dq_r.abs().max()) < 1e-6
        mag = (dout.reshape(B, 1, H, hd).abs() * kv.float()[:, D:].reshape(B, N, H, hd).abs()).sum(-1, keepdim=True) * hd ** -0.5
        e_dk = (dk.double().norm() / (mag * q.reshape(1, 1, H, hd).abs()).double().norm()).item()
        e_dq = (dq.double().norm() / (mag * kv.float()[:, :D].reshape(B, N, H, hd).abs()).double().norm()).item()
    else:
        e_dk, e_dq = _rel(dk, dk_r), _rel(dq, dq_r)
    e = {"out": _rel(out, o_r), "probs": _rel(probs, a_r), "dk": e_dk, "dv": _rel(dv, dv_r), "dq": e_dq}
    print(f"attn_pool hd{hd} {kv.dtype} B{B} N{N} H{H} {what}: " + " ".join(f"{k}={v:.3e}" for k, v in e.items()))
    assert e["out"] < 3e-3 and e["probs"] < 3e-3
    for name in ("dk", "dv", "dq"):
        assert e[name] < 1e-2, name


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("hd", [64, 72, 80])
@pytest.mark.parametrize("B,N,H", SHAPES)
def test_attn_pool_hd_vs_reference(be, dev, B, N, H, hd, dtype):
    q, kv, dout = make_inputs(B, N, H, hd, dtype)
    got = run_hd(be, dev, q, kv, dout, B, N, H, hd)
    check_vs_reference(q, kv, dout, B, N, H, hd, *got)
    if hd == 64:                                                         # the same kernels as the public entries: the same bits
        for a, b, name in zip(got, run_hd(be, dev, q, kv, dout, B, N, H, 64, entry="dt"), ("out", "probs", "dkv", "dq_part")):
            assert torch.equal(a, b), name


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("hd,pad", [(64, 8), (72, 8), (80, 8), (72, 0)])
def test_attn_pool_hd_extents(be, dev, hd, pad, dtype):
    """guard-banded operands (tests/extent.py: I1 guards intact, I2 outputs independent of the fill, I3 the bits of the contiguous call) with ldkv = 2 H hd + 8, and at 72
    with ldkv = 2 H hd exactly: there the bytes behind the last head of v in the last row are the guard.  260 keys: the second pass of the score loop."""
    B, N, H = 2, 260, 2
    D = H * hd
    scale = hd ** -0.5
    q0, kv0, dout0 = make_inputs(B, N, H, hd, dtype, seed=3)

    def case(ar):
        q = ar.put(q0, 0, "q"); kv = ar.put(kv0, pad, "kv"); dout = ar.put(dout0, 4, "dout")
        out = ar.out((B, D), F32, 4, "out"); probs = ar.out(B * H * N, F32, 0, "probs"); dkv = ar.out((B * N, 2 * D), dtype, pad, "dkv"); dq_part = ar.out((B, D), F32, 0, "dq_part")
        be.check(be.lib.vdk_attn_pool_fwd_hd(p(q), p(kv), kv.stride(0), B, N, H, hd, scale, p(out), out.stride(0), p(probs), DT[dtype], be.stream()), "attn_pool_fwd_hd")
        be.check(be.lib.vdk_attn_pool_bwd_hd(p(q), p(kv), kv.stride(0), p(probs), p(dout), dout.stride(0), B, N, H, hd, scale, p(dkv), dkv.stride(0), p(dq_part), DT[dtype],
                                             be.stream()), "attn_pool_bwd_hd")
        return {"out": out, "probs": probs, "dkv": dkv, "dq_part": dq_part}

    got, _ = run_isolated(case, dev, sync=torch.cuda.synchronize if be.device_only else None)
    check_vs_reference(q0, kv0, dout0, B, N, H, hd, got["out"].cpu(), got["probs"].cpu().reshape(B, H, N), got["dkv"].cpu(), got["dq_part"].cpu(), what=f"pad {pad}")


def test_attn_pool_hd_refuses_other_head_dims(be, dev):
    """every head_dim but 64, 72 and 80 is VDK_EUNSUPPORTED; a pitch below 2 H head_dim is an argument error"""
    for hd in (32, 88, 96, 128):
        q, kv, dout = (t.to(dev) for t in make_inputs(1, 4, 1, hd, BF))
        out = torch.zeros(1, hd, device=dev); probs = torch.zeros(1, 1, 4, device=dev); dkv = torch.zeros_like(kv); dqp = torch.zeros(1, hd, device=dev)
        assert be.lib.vdk_attn_pool_fwd_hd(p(q), p(kv), 2 * hd, 1, 4, 1, hd, 1.0, p(out), hd, p(probs), 0, be.stream()) == _abi.EUNSUPPORTED
        assert be.lib.vdk_attn_pool_bwd_hd(p(q), p(kv), 2 * hd, p(probs), p(dout), hd, 1, 4, 1, hd, 1.0, p(dkv), 2 * hd, p(dqp), 0, be.stream()) == _abi.EUNSUPPORTED
    q, kv, dout = (t.to(dev) for t in make_inputs(1, 4, 1, 72, BF))
    out = torch.zeros(1, 72, device=dev); probs = torch.zeros(1, 1, 4, device=dev)
    assert be.lib.vdk_attn_pool_fwd_hd(p(q), p(kv), 2 * 64, 1, 4, 1, 72, 1.0, p(out), 72, p(probs), 0, be.stream()) != 0
