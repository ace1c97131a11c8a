"""The head-dim-72 attention kernels (csrc/attention_hd.hip) read and write nothing outside their operands' extents: tests/test_attention_hd80_extent.py at HD = 72, through
the debug entries of csrc/vdk_internal.h (I1 guards intact, I2 outputs bit-identical across the fill patterns, I3 the same bits as the contiguous call, plus the accuracy
check).  What is specific to 72: the last contraction step covers columns 64 .. 79 of an 80-wide tile, and the 16 bytes of columns 72 .. 79 are the next head's -- or, for
the last head of v in the last row with no pitch padding, the guard band itself, whose 0xFF fill is NaN in both 16-bit formats."""
import pytest
import torch

from tests.extent import run_isolated
from tests.test_attention import _ref, _rel
from tests.test_attention_hd80 import errors_vs_torch

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
DT = {BF: 0, HF: 2}
HD = 72


def p(t):
    return t.data_ptr()


# pads (elements) of qkv, dout / o, dqkv.  "padded": ld = 3 D + 8 and ldo = D + 24 shift the 16-byte row starts from row to row, lddqkv = 3 D + 64 keeps them aligned (the
# 80-wide file's pitches); "exact": ld = 3 D, ldo = D, lddqkv = 3 D -- nothing between the rows, so what follows the last head of v in the last row is the guard
PADS = {"padded": (8, 24, 64), "exact": (0, 0, 0)}


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("pads", ["padded", "exact"])
@pytest.mark.parametrize("B,N,H", [(2, 17, 2), (1, 256, 1), (2, 100, 3)])
def test_attention_hd72_extents(be, dev, B, N, H, pads, dtype):
    """B = H = 1: what lies beyond N (and beyond column 72) is the guard; B * H > 1: it is another item's (or another head's) live data"""
    D = H * HD
    scale = HD ** -0.5
    pq, po, pd = PADS[pads]
    torch.manual_seed(30)
    qkv0 = (torch.randn(B * N, 3 * D) * 1.5).to(dtype); qkv0[N // 2, :D] *= 4.0
    dout0 = torch.randn(B * N, D).to(dtype)

    def case(ar):
        qkv = ar.put(qkv0, pq, "qkv"); dout = ar.put(dout0, po, "dout")
        o = ar.out((B * N, D), dtype, po, "o"); lse = ar.out(B * H * N, F32, 0, "lse"); dqkv = ar.out((B * N, 3 * D), dtype, pd, "dqkv"); dvec = ar.out(B * H * N, F32, 0, "dvec")
        ldo = o.stride(0)                                                # (o and dout share ldo in the ABI: both carry the same pad)
        assert qkv.stride(0) == 3 * D + (0 if ar.plain else pq) and ldo == D + (0 if ar.plain else po)
        be.check(be.lib.vdk_debug_attention_hd_fwd(p(qkv), qkv.stride(0), p(o), ldo, p(lse), B, N, H, HD, scale, DT[dtype], be.stream()), "attention hd fwd")
        be.check(be.lib.vdk_debug_attention_hd_bwd(p(qkv), qkv.stride(0), p(o), p(dout), ldo, p(lse), p(dqkv), dqkv.stride(0), p(dvec), B, N, H, HD, scale, DT[dtype],
                                                   be.stream()), "attention hd bwd")
        return {"o": o, "lse": lse, "dqkv": dqkv}

    got, _ = run_isolated(case, dev, sync=torch.cuda.synchronize if be.device_only else None)
    e = errors_vs_torch(qkv0.reshape(B, N, 3 * D), dout0.reshape(B, N, D), H, got["o"].cpu().reshape(B, N, D), got["lse"].cpu().reshape(B, H, N),
                        got["dqkv"].cpu().reshape(B, N, 3 * D))
    print(f"hd72 extents {pads} {dtype} B{B} N{N} H{H}: " + " ".join(f"{k}={v:.3e}" for k, v in e.items()))
    assert e["lse"] < 1e-5
    if dtype == BF:
        assert e["o"] < 6e-3                                             # the bounds of tests/test_attention.py
    else:                                                                # fp16 forward: against the 64-wide kernels at the same (B, N, H) and seed, as in tests/test_attention_hd72.py
        from visiondk_amd import ops
        torch.manual_seed(30)
        q64 = (torch.randn(B, N, 3 * H * 64) * 1.5).to(dtype); q64[0, N // 2, :H * 64] *= 4.0
        o64, _ = ops.attention_fwd(q64.to(dev), H, backend=be)
        e64 = _rel(o64.float().cpu(), _ref(q64.float(), H)[0])
        print(f"hd64 o={e64:.3e}")
        assert e["o"] <= 1.5 * e64
    for name in ("dq", "dk", "dv"):
        assert e[name] < (1.5e-2 if dtype == BF else 2e-3), name
