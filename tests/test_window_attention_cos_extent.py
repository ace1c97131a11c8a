"""The cosine window-attention kernels (csrc/window_attention_cos.hip) read and write nothing outside their operands' extents (tests/extent.py, as
tests/test_attention_hd72_extent.py): both entries on guard-banded, column-padded operands filled with 0x00 / 0xFF / 0x7B -- I1 guards intact, I2 outputs bit-identical
across the fills, I3 the same bits as the contiguous call -- with workspaces of exactly the reported size (a guarded flat buffer each: one byte past it is guard).
9 and 24 (window, head) items: the forward's last workgroup of four waves and the backward's last head group are ragged."""
import ctypes as C

import pytest
import torch

from tests.extent import run_isolated
from tests.test_window_attention_cos import HD, N, OPF, _flat, _perm, case

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
PADS = (8, 24, 64)          # elements between the rows of qkv, of o and dout (they share ldo), of dqkv


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("windows,heads,nW,indexed", [(3, 3, 0, False), (8, 3, 4, True)])
def test_window_attention_cos_extents(be, dev, windows, heads, nW, indexed, dtype):
    q, k, v, g, ls, tau, bias, mask, lb, ref, bnd = case(windows, heads, nW, dtype)
    Cc, T = heads * HD, windows * N
    perm = _perm(windows, indexed)
    scat = lambda t: torch.empty_like(t).index_copy_(0, perm, t)
    qkv0, dout0 = scat(torch.cat([_flat(q), _flat(k), _flat(v)], dim=1).to(dtype)), scat(_flat(g).to(dtype))
    p = lambda t: None if t is None else t.data_ptr()          # (padded views are not contiguous: be.ptr refuses them)
    need_f, need_b = C.c_size_t(0), C.c_size_t(0)
    be.check(be.lib.vdk_wa_cos_fwd_workspace_bytes(nW, heads, C.byref(need_f)), "cos fwd workspace")
    be.check(be.lib.vdk_wa_cos_bwd_workspace_bytes(windows, nW, heads, C.byref(need_b)), "cos bwd workspace")

    def run(ar):
        pq, po, pd = PADS
        qkv, dout = ar.put(qkv0, pq, "qkv"), ar.put(dout0, po, "dout")
        td, bd = ar.put(tau.float(), 0, "tau"), ar.put(bias.float().reshape(-1), 0, "bias")
        md = None if mask is None else ar.put(mask.float().reshape(-1), 0, "mask")
        rd = ar.put(perm.to(torch.int32), 0, "rowidx") if indexed else None
        o, lse, dqkv = ar.out((T, Cc), dtype, po, "o"), ar.out(windows * heads * N, F32, 0, "lse"), ar.out((T, 3 * Cc), dtype, pd, "dqkv")
        dbias, dtau = ar.out(heads * N * N, F32, 0, "dbias"), ar.out(heads, F32, 0, "dtau")
        wf, wb = ar.out(need_f.value, torch.uint8, 0, "fwd workspace"), ar.out(need_b.value, torch.uint8, 0, "bwd workspace")
        assert o.stride(0) == dout.stride(0)
        be.check(be.lib.vdk_wa_cos_fwd(p(qkv), qkv.stride(0), p(o), o.stride(0), p(lse), p(td), p(bd), p(md), nW, windows, heads, p(rd), OPF[dtype], p(wf), need_f.value,
                                       be.stream()), "cos fwd")
        be.check(be.lib.vdk_wa_cos_bwd(p(qkv), qkv.stride(0), p(o), p(dout), o.stride(0), p(lse), p(td), p(bd), p(md), nW, windows, heads, p(rd), p(dqkv), dqkv.stride(0),
                                       p(dbias), p(dtau), OPF[dtype], p(wb), need_b.value, be.stream()), "cos bwd")
        return {"o": o, "lse": lse, "dqkv": dqkv, "dbias": dbias, "dtau": dtau}

    got, _ = run_isolated(run, dev, sync=torch.cuda.synchronize if be.device_only else None, what=f"cos extents {dtype} W{windows} nW{nW}")
    for name, t in got.items():
        assert bool(torch.isfinite(t.float()).all()), name
