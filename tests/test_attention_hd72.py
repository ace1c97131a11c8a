"""K3 attention at head dim 72 (csrc/attention_hd.hip: SigLIP SO400M/14, 1152 / 16 heads) vs plain torch fp32 on the same 16-bit-rounded inputs, on the CPU SIMT emulation
and on the device.  It is the 80-wide geometry with a ragged last contraction step (columns 64 .. 79 of which 72 .. 79 do not exist).  The public entries refuse 72
(tests/test_attention_hd80.py pins that), so this file goes through the debug entries of csrc/vdk_internal.h; the ViT engine reaches the kernels in-library."""
import pytest
import torch

from tests.test_attention_hd80 import errors_vs_torch, make_inputs
from tests.test_attention_hd80 import _run as _run_public
from visiondk_amd import _abi

BF, HF = torch.bfloat16, torch.float16
DT = {BF: 0, HF: 2}
HD = 72
# the shapes of tests/test_attention_hd80.py with this model's N = 256 (exactly four chunks, eight query tiles, two full groups) in place of 257, plus a last chunk short by
# one key: one key; one partial tile; a tile edge and one past it; a chunk edge and one past it; 256; 255; 300; an odd item count
SHAPES = [(2, 1, 1), (2, 17, 2), (1, 32, 1), (1, 33, 2), (1, 64, 1), (1, 65, 2), (2, 256, 2), (1, 255, 1), (1, 300, 1), (5, 65, 3)]


def p(t):
    return t.data_ptr()


def run_hd(be, dev, qkv, dout, H, hd=HD):
    """forward and backward through vdk_debug_attention_hd_*: (o, lse, dqkv) on the CPU.  The backward consumes the forward's own 16-bit o and lse."""
    B, N, D3 = qkv.shape
    D = D3 // 3
    assert D == H * hd
    dt = DT[qkv.dtype]
    q, g = qkv.to(dev).contiguous(), dout.to(dev).contiguous()
    o = torch.empty((B, N, D), dtype=qkv.dtype, device=dev); lse = torch.empty((B, H, N), dtype=torch.float32, device=dev)
    dqkv = torch.empty_like(q); dvec = torch.empty_like(lse)
    be.check(be.lib.vdk_debug_attention_hd_fwd(p(q), 3 * D, p(o), D, p(lse), B, N, H, hd, hd ** -0.5, dt, be.stream()), "attention hd fwd")
    be.check(be.lib.vdk_debug_attention_hd_bwd(p(q), 3 * D, p(o), p(g), D, p(lse), p(dqkv), 3 * D, p(dvec), B, N, H, hd, hd ** -0.5, dt, be.stream()), "attention hd bwd")
    return o.cpu(), lse.cpu(), dqkv.cpu()


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,N,H", SHAPES)
def test_attention_hd72_fwd_bwd(be, dev, B, N, H, dtype):
    """bf16: the bounds of tests/test_attention.py (lse 1e-5, o 6e-3, dq / dk / dv 1.5e-2).  fp16: gradients at that file's 2e-3, lse 1e-5, and the forward error against
    torch fp32 at most 1.5 x that of the 64-wide kernels at the same (B, N, H) and seed -- the rule of the 80-wide test (the contraction over hd is 1.125 x longer)."""
    qkv, dout = make_inputs(B, N, H, HD, dtype)
    e = errors_vs_torch(qkv, dout, H, *run_hd(be, dev, qkv, dout, H))
    print(f"hd72 {dtype} B{B} N{N} H{H}: " + " ".join(f"{k}={v:.3e}" for k, v in e.items()))
    assert e["lse"] < 1e-5
    gtol = 1.5e-2 if dtype == BF else 2e-3
    if dtype == BF:
        assert e["o"] < 6e-3
    else:
        qkv64, dout64 = make_inputs(B, N, H, 64, dtype)
        e64 = errors_vs_torch(qkv64, dout64, H, *_run_public(be, dev, qkv64, dout64, H))
        print(f"hd64 {dtype} B{B} N{N} H{H}: " + " ".join(f"{k}={v:.3e}" for k, v in e64.items()))
        assert e["o"] <= 1.5 * e64["o"]
    for name in ("dq", "dk", "dv"):
        assert e[name] < gtol, name


@pytest.mark.parametrize("grid", [1, 8, 24])
def test_attention_hd72_units_per_workgroup(be, dev, grid, monkeypatch):
    """VDK_ATTN_GRID caps the grid: a workgroup walks over several units, the chunk buffers (and the kv kernel's staged lse / D values) run on across unit boundaries.
    6 items x 2 groups = 12 units; grid 1 -> 8 workgroups (one per XCD residue), 24 -> more workgroups than units.  Any grid gives the same bits, forward and backward."""
    B, N, H = 3, 256, 2
    for dtype in (BF, HF):
        qkv, dout = make_inputs(B, N, H, HD, dtype, seed=2)
        monkeypatch.delenv("VDK_ATTN_GRID", raising=False)
        o2, lse2, d2 = run_hd(be, dev, qkv, dout, H)
        monkeypatch.setenv("VDK_ATTN_GRID", str(grid))
        o, lse, d = run_hd(be, dev, qkv, dout, H)
        monkeypatch.delenv("VDK_ATTN_GRID")
        assert torch.equal(o, o2) and torch.equal(lse, lse2) and torch.equal(d, d2)


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_attention_hd72_neighbouring_head_does_not_leak(be, dev, dtype):
    """Columns 72 .. 79 of head h's 80-wide tile are the first 8 columns of head h + 1 in memory.  With ALL of head 1 of q, k and v (and of dout) at 1e4 -- finite, and
    large enough to be unmistakable -- head 0's o, lse, dq, dk and dv are bit-identical to the run where head 1 is zero.  N = 65: a full chunk and a one-key chunk."""
    B, N, H = 2, 65, 2
    qkv, dout = make_inputs(B, N, H, HD, dtype, seed=4)
    D = H * HD

    def with_head1(value):
        x, g = qkv.clone(), dout.clone()
        for i in range(3):
            x[..., i * D + HD:(i + 1) * D] = value
        g[..., HD:] = value
        return run_hd(be, dev, x, g, H)

    o_a, lse_a, d_a = with_head1(1e4)
    o_b, lse_b, d_b = with_head1(0.0)
    assert torch.isfinite(o_a[..., :HD].float()).all() and torch.isfinite(d_a[..., :HD].float()).all()      # (head 1's own results at such inputs are not looked at)
    assert torch.equal(o_a[..., :HD], o_b[..., :HD]) and torch.equal(lse_a[:, 0], lse_b[:, 0])
    for i in range(3):
        assert torch.equal(d_a[..., i * D:i * D + HD], d_b[..., i * D:i * D + HD]), "dq dk dv".split()[i]


def test_attention_hd_debug_entries_serve_72_and_80_only(be, dev):
    """80 through the debug entries: the same bits as the public entries; 64 and 96: VDK_EUNSUPPORTED"""
    qkv, dout = make_inputs(1, 65, 2, 80, BF, seed=8)
    for a, b in zip(run_hd(be, dev, qkv, dout, 2, hd=80), _run_public(be, dev, qkv, dout, 2)):
        assert torch.equal(a, b)
    for hd in (64, 96):
        q = torch.zeros(1, 8, 3 * hd, dtype=BF, device=dev); o = torch.zeros(1, 8, hd, dtype=BF, device=dev); g = torch.zeros_like(o); dq = torch.zeros_like(q)
        lse = torch.zeros(1, 1, 8, device=dev); dvec = torch.zeros(1, 1, 8, device=dev)
        assert be.lib.vdk_debug_attention_hd_fwd(p(q), 3 * hd, p(o), hd, p(lse), 1, 8, 1, hd, hd ** -0.5, 0, be.stream()) == _abi.EUNSUPPORTED
        assert be.lib.vdk_debug_attention_hd_bwd(p(q), 3 * hd, p(o), p(g), hd, p(lse), p(dq), 3 * hd, p(dvec), 1, 8, 1, hd, hd ** -0.5, 0, be.stream()) == _abi.EUNSUPPORTED
