"""K3 attention at head dim 80 (csrc/attention_hd.hip: ViT-H/14 CLIP, 1280 / 16 heads) vs plain torch fp32 on the same 16-bit-rounded inputs, on the CPU SIMT emulation
and on the device.  The kernels stream K / V (Q / dO in the kv backward) in chunks of 64 rows, a work unit is (batch, head, group of 4 query tiles of 32 rows)."""
import pytest
import torch

from tests.test_attention import _ref, _rel
from visiondk_amd import _abi, ops

BF, HF = torch.bfloat16, torch.float16
CHUNK = 64                                                 # AH_CROWS of csrc/attention_hd.hip
# the smallest shapes that reach each boundary: one key; one partial tile; a tile edge and one past it; a chunk edge and one past it; the model's N (5 chunks, the last
# with one key; 9 query tiles = 3 groups, the last with three idle waves); 300; an odd item count (15 items: XCD residues with one and with two items)
SHAPES = [(2, 1, 1), (2, 17, 2), (1, 32, 1), (1, 33, 2), (1, CHUNK, 1), (1, CHUNK + 1, 2), (2, 257, 2), (1, 300, 1), (5, 65, 3)]


def make_inputs(B, N, H, hd, dtype, seed=0):
    torch.manual_seed(seed)
    D = H * hd
    qkv = (torch.randn(B, N, 3 * D) * 1.5).to(dtype)
    qkv[0, N // 2, :D] *= 4.0                              # a peaky row: exercises the online-softmax rescale
    dout = torch.randn(B, N, D).to(dtype)
    return qkv, dout


def errors_vs_torch(qkv, dout, H, o, lse, dqkv):
    """relative errors of a kernel result (CPU tensors) against torch fp32 on the same rounded inputs"""
    D = qkv.shape[2] // 3
    qr = qkv.float().requires_grad_(True)
    oref, lseref = _ref(qr, H)
    oref.backward(dout.float())
    e = {"lse": _rel(lse, lseref.detach()), "o": _rel(o.float(), oref.detach())}
    for i, name in enumerate(("dq", "dk", "dv")):
        e[name] = _rel(dqkv[..., i * D:(i + 1) * D].float(), qr.grad[..., i * D:(i + 1) * D])
    if qkv.shape[1] == 1:
        # one key: P = 1 and dS = dP - D = 0, so dq = dk = 0 exactly and a relative error has no denominator.  The kernels form dP and D as two fp32 sums of the same hd
        # products in different orders; what is left is measured against the un-cancelled magnitude scale * sum_i |dO_i v_i| * |k| (resp. |q|) of the terms that cancel
        B, N, _ = qkv.shape
        x = qkv.float().reshape(B, N, 3, H, D // H)
        mag = (dout.float().reshape(B, N, H, D // H).abs() * x[:, :, 2].abs()).sum(-1, keepdim=True) * (D // H) ** -0.5
        for i, name in ((0, "dq"), (1, "dk")):
            assert float(qr.grad[..., i * D:(i + 1) * D].abs().max()) < 1e-6
            e[name] = (dqkv[..., i * D:(i + 1) * D].double().norm() / (mag * x[:, :, 1 - i].abs()).double().norm()).item()
    return e


def _run(be, dev, qkv, dout, H):
    q, g = qkv.to(dev), dout.to(dev)
    o, lse = ops.attention_fwd(q, H, backend=be)
    dqkv = ops.attention_bwd(q, o, g, lse, H, backend=be)                # the backward consumes the forward's own 16-bit o and lse
    return o.cpu(), lse.cpu(), dqkv.cpu()


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,N,H", SHAPES)
def test_attention_hd80_fwd_bwd(be, dev, B, N, H, dtype):
    """bf16: the bounds of tests/test_attention.py (lse 1e-5, o 6e-3, dq / dk / dv 1.5e-2).  fp16: gradients at that file's 2e-3; lse is fp32 arithmetic on exactly
    representable inputs in either format, so 1e-5 holds as well; the forward has no project bound, so the 64-wide kernels at the same (B, N, H) and seed are the
    reference: the 80-wide error against torch fp32 may be at most 1.5 x theirs (the contraction over hd is 1.25 x longer)."""
    qkv, dout = make_inputs(B, N, H, 80, dtype)
    e = errors_vs_torch(qkv, dout, H, *_run(be, dev, qkv, dout, H))
    print(f"hd80 {dtype} B{B} N{N} H{H}: " + " ".join(f"{k}={v:.3e}" for k, v in e.items()))
    assert e["lse"] < 1e-5
    gtol = 1.5e-2 if dtype == BF else 2e-3
    if dtype == BF:
        assert e["o"] < 6e-3
    else:
        qkv64, dout64 = make_inputs(B, N, H, 64, dtype)
        e64 = errors_vs_torch(qkv64, dout64, H, *_run(be, dev, qkv64, dout64, H))
        print(f"hd64 {dtype} B{B} N{N} H{H}: " + " ".join(f"{k}={v:.3e}" for k, v in e64.items()))
        assert e["o"] <= 1.5 * e64["o"]
    for name in ("dq", "dk", "dv"):
        assert e[name] < gtol, name


@pytest.mark.parametrize("grid", [1, 8, 24])
def test_attention_hd80_units_per_workgroup(be, dev, grid, monkeypatch):
    """VDK_ATTN_GRID caps the grid: a workgroup walks over several units, the chunk buffers (and the kv kernel's staged lse / D values) run on across unit boundaries.
    6 items x 3 groups = 18 units; grid 1 -> 8 workgroups (one per XCD residue), 24 -> more workgroups than units.  Any grid gives the same bits, forward and backward."""
    B, N, H = 3, 257, 2
    for dtype in (BF, HF):
        qkv, dout = make_inputs(B, N, H, 80, dtype, seed=2)
        monkeypatch.delenv("VDK_ATTN_GRID", raising=False)
        o2, lse2, d2 = _run(be, dev, qkv, dout, H)
        monkeypatch.setenv("VDK_ATTN_GRID", str(grid))
        o, lse, d = _run(be, dev, qkv, dout, H)
        monkeypatch.delenv("VDK_ATTN_GRID")
        assert torch.equal(o, o2) and torch.equal(lse, lse2) and torch.equal(d, d2)


def test_attention_hd64_routing_untouched(be, dev):
    """head_dim 64 through the same entry points: the same bits before and after the 80-wide path ran in the process; 72 and 96 are VDK_EUNSUPPORTED"""
    B, N, H = 2, 197, 2
    qkv, dout = make_inputs(B, N, H, 64, BF, seed=7)
    before = _run(be, dev, qkv, dout, H)
    q80, g80 = make_inputs(1, 65, 1, 80, BF, seed=8)
    _run(be, dev, q80, g80, 1)
    after = _run(be, dev, qkv, dout, H)
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    for hd in (72, 96):
        D = hd
        q = torch.zeros(1, 8, 3 * D, dtype=BF, device=dev); o = torch.zeros(1, 8, D, dtype=BF, device=dev); g = torch.zeros_like(o); dq = torch.zeros_like(q)
        lse = torch.zeros(1, 1, 8, device=dev); dvec = torch.zeros(1, 1, 8, device=dev)
        p = lambda t: t.data_ptr()
        for dt in (0, 2):
            assert be.lib.vdk_attention_fwd_dt(p(q), 3 * D, p(o), D, p(lse), 1, 8, 1, hd, hd ** -0.5, dt, be.stream()) == _abi.EUNSUPPORTED
            assert be.lib.vdk_attention_bwd_dt(p(q), 3 * D, p(o), p(g), D, p(lse), p(dq), 3 * D, p(dvec), 1, 8, 1, hd, hd ** -0.5, dt, be.stream()) == _abi.EUNSUPPORTED
        assert b"64 or 80" in be.lib.vdk_last_error()
