"""The arithmetic family of tests/gemmbound.py on every GEMM kernel structure and operand format: Gaussian operands as tests/test_gemm.py draws them, every output ELEMENT
against float64 -- fp32 outputs within 2 (K + 4) 2^-24 S with S = |alpha| |A| |B|^T (+ |bias| + |residual|), the a-priori bound of any fp32 accumulation of K products;
16-bit outputs by the half-ulp rule with that bound as the slack.  This sees what the integer operands of tests/test_gemm_exact.py cannot: a slab or partial kept in 16
bits, an fp16 accumulator, a store that does not round to nearest.  One ragged shape per kernel structure (300 x 264 x 256: 4 k-tiles), 264 x 256 x 768 with split-K 3,
stream-K on kernel 3, TN split-K, the fp32-MFMA and the fp8 GEMM.  Each case prints its worst ratio to the bound (pytest -s); DESIGN.md section 4 records them.

Where an activation follows the accumulation the slack is what the activation passes on plus its own: GELU is 1.13-Lipschitz (max |GELU'| = 1.129), so
slack = 1.13 x the pre-activation's bound + 8 max(E32, eps32 |g64|); dGELU multiplies the accumulator by |GELU'(aux)| <= 1.13 of a GIVEN aux: the same expression with E32
taken from torch's float32 evaluation of acc x GELU'(aux).  fp16 operands: kernels 1, 5, 6 (tests/test_gemm_exact.py lists what the dispatcher does not serve)."""
import pytest
import torch

from tests import gemmbound as gb
from tests.test_gemm_exact import BF16, F16, F32, KERN_FMT, Forms, _ids, forced, served
from visiondk_amd import ops
from visiondk_amd.ops import ACT_DGELU, ACT_GELU, FP8_E4M3, FP8_E5M2

M, N, K = 300, 264, 256


def _gauss(M, N, K, dtype, seed, bscale=1.0):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).to(dtype); b = (torch.randn(N, K, generator=g) * bscale).to(dtype)
    b[:, 3] += 2.0 * bscale                      # asymmetric operands catch transposed fragment layouts
    return a, b, torch.randn(N, generator=g), torch.randn(M, N, generator=g), torch.randn(M, N, generator=g).to(dtype)


def _act_refs(a, b, bias, u16):
    """float64 references and slacks of the GELU + aux and dGELU forms"""
    acc = a.double() @ b.double().t()
    u = acc + bias.double()
    Su, S = gb.arith_unit(a, b, bias=bias), gb.arith_unit(a, b)
    g64 = gb.gelu(u)
    g_extra = (gb.GELU_GRAD_MAX - 1.0) * gb.arith_bound(Su, a.shape[1]) + gb.act_slack(gb.gelu(u.float()), g64)[0]
    d = gb.gelu_grad(u16.double())
    dg64 = acc * d
    dg_extra = gb.act_slack(acc.float() * gb.gelu_grad(u16.float()), dg64)[0]
    return u, Su, g64, g_extra, dg64, S * gb.GELU_GRAD_MAX, dg_extra


@pytest.mark.parametrize("kern,dtype", KERN_FMT, ids=_ids)
def test_nt_every_element_within_the_accumulation_bound(be, dev, kern, dtype):
    a, b, bias, res, u16 = _gauss(M, N, K, dtype, 5 + kern)
    ref = a.double() @ b.double().t()
    S, Sb, Sbr = gb.arith_unit(a, b), gb.arith_unit(a, b, bias=bias), gb.arith_unit(a, b, bias=bias, residual=res)
    ad, bd, biasd, resd, u16d = (t.to(dev) for t in (a, b, bias, res, u16))
    a2, b2 = a, (b.float() * 0.1).to(dtype)         # pre-activations spread over GELU's curved range, as tests/test_gemm.py draws them
    u, Su, g64, g_extra, dg64, Sd, dg_extra = _act_refs(a2, b2, bias, u16)
    b2d = b2.to(dev)
    tag = f"kernel {kern} {dtype}"
    f = Forms(be, served(kern, dtype, K), tag)
    with forced(be, kern):
        f.run("fp32", lambda: gb.check_arith(ops.gemm_nt(ad, bd, out_dtype=F32, backend=be), ref, S, K, tag + " fp32"))
        f.run("fp32 bias residual", lambda: gb.check_arith(ops.gemm_nt(ad, bd, out_dtype=F32, bias=biasd, residual=resd, backend=be), ref + bias.double() + res.double(), Sbr, K,
                                                          tag + " fp32 bias residual"))
        f.run("fp32 alpha", lambda: gb.check_arith(ops.gemm_nt(ad, bd, out_dtype=F32, alpha=0.37, backend=be), ref * float(torch.tensor(0.37)), 0.37 * S, K, tag + " fp32 alpha"))
        f.run("16-bit", lambda: gb.check_arith(ops.gemm_nt(ad, bd, backend=be), ref, S, K, tag + " 16-bit"))
        f.run("16-bit bias", lambda: gb.check_arith(ops.gemm_nt(ad, bd, bias=biasd, backend=be), ref + bias.double(), Sb, K, tag + " 16-bit bias"))
        def gelu_aux():
            aux = torch.full((M, N), float("nan"), dtype=dtype, device=dev)
            g = ops.gemm_nt(ad, b2d, bias=biasd, act=ACT_GELU, aux=aux, backend=be)
            gb.check_arith(aux, u, Su, K, tag + " saved pre-activation")
            gb.check_arith(g, g64, Su, K, tag + " GELU", extra=g_extra)
        f.run("GELU + aux", gelu_aux)
        f.run("DGELU", lambda: gb.check_arith(ops.gemm_nt(ad, b2d, act=ACT_DGELU, aux=u16d, backend=be), dg64, Sd, K, tag + " DGELU", extra=dg_extra))
    f.done()


@pytest.mark.parametrize("kern,dtype", [(2, BF16), (5, BF16), (5, F16), (6, BF16), (6, F16)], ids=_ids)
def test_split_k_every_element_within_the_accumulation_bound(be, dev, kern, dtype):
    """264 x 256 x 768 in three slabs (NT), and the weight-gradient form from k-major operands: a slab kept in 16 bits or summed in another precision shows here"""
    Ms, Ns, Ks = 264, 256, 768
    a, b, *_ = _gauss(Ms, Ns, Ks, dtype, 9 + kern)
    ref, S = a.double() @ b.double().t(), gb.arith_unit(a, b)
    ad, bd = a.to(dev), b.to(dev)
    at, bt = a.t().contiguous().to(dev), b.t().contiguous().to(dev)
    tag = f"kernel {kern} {dtype} split-K"
    f = Forms(be, kern, tag)
    with forced(be, kern):
        f.run("NT fp32", lambda: gb.check_arith(ops.gemm_nt(ad, bd, out_dtype=F32, splitk=3, backend=be), ref, S, Ks, tag + " NT fp32"))
        f.run("NT 16-bit", lambda: gb.check_arith(ops.gemm_nt(ad, bd, splitk=3, backend=be), ref, S, Ks, tag + " NT 16-bit"))
        f.run("TN fp32", lambda: gb.check_arith(ops.gemm_nt(at, bt, out_dtype=F32, splitk=3, trans=True, backend=be), ref, S, Ks, tag + " TN fp32"))
        f.run("TN fp32 whole", lambda: gb.check_arith(ops.gemm_nt(at, bt, out_dtype=F32, trans=True, backend=be), ref, S, Ks, tag + " TN fp32 whole"))
    f.done()


@pytest.mark.parametrize("grid", [8, 16])
def test_stream_k_every_element_within_the_accumulation_bound(be, dev, grid):
    Ms, Ns, Ks = 520, 520, 256
    a, b, bias, res, _ = _gauss(Ms, Ns, Ks, BF16, 11 + grid)
    ref = a.double() @ b.double().t()
    ad, bd, biasd, resd = (t.to(dev) for t in (a, b, bias, res))
    tag = f"stream-K grid {grid}"
    f = Forms(be, 3, tag)
    be.lib.vdk_gemm_streamk_grid(grid)
    try:
        with forced(be, 3):
            ws = ops.streamk_workspace(dev, backend=be)
            f.run("fp32 bias residual", lambda: gb.check_arith(ops.gemm_nt(ad, bd, out_dtype=F32, bias=biasd, residual=resd, streamk_ws=ws, backend=be),
                                                              ref + bias.double() + res.double(), gb.arith_unit(a, b, bias=bias, residual=res), Ks, tag + " fp32 bias residual"))
            f.run("16-bit bias", lambda: gb.check_arith(ops.gemm_nt(ad, bd, bias=biasd, streamk_ws=ws, backend=be), ref + bias.double(), gb.arith_unit(a, b, bias=bias), Ks,
                                                       tag + " 16-bit bias"))
    finally:
        be.lib.vdk_gemm_streamk_grid(0)
    f.done()


def test_gemm_f32_every_element_within_the_accumulation_bound(be, dev):
    g = torch.Generator().manual_seed(3)
    a, b, bias, res = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    ref, S = a.double() @ b.double().t(), gb.arith_unit(a, b)
    ad, bd, biasd, resd = (t.to(dev) for t in (a, b, bias, res))
    f = Forms(be, None, "gemm_f32")
    f.run("plain", lambda: gb.check_arith(ops.gemm_f32(ad, bd, backend=be), ref, S, K, "gemm_f32 plain"))
    f.run("bias residual alpha", lambda: gb.check_arith(ops.gemm_f32(ad, bd, bias=biasd, residual=resd, alpha=0.5, backend=be), 0.5 * ref + bias.double() + res.double(),
                                                       gb.arith_unit(a, b, alpha=0.5, bias=bias, residual=res), K, "gemm_f32 bias residual alpha"))
    f.run("k-major", lambda: gb.check_arith(ops.gemm_f32(a.t().contiguous().to(dev), b.t().contiguous().to(dev), a_kmajor=True, b_kmajor=True, backend=be), ref, S, K, "gemm_f32 k-major"))
    f.run("k_splits 3", lambda: gb.check_arith(ops.gemm_f32(ad, bd, k_splits=3, backend=be), ref, S, K, "gemm_f32 k_splits 3"))
    a01 = float(torch.tensor(0.1))                   # the float32 the kernel receives
    u = a01 * ref + bias.double()
    Su = gb.arith_unit(a, b, alpha=0.1, bias=bias)
    g64 = gb.gelu(u)
    extra = (gb.GELU_GRAD_MAX - 1.0) * gb.arith_bound(Su, K) + gb.act_slack(gb.gelu(u.float()), g64)[0]
    f.run("GELU", lambda: gb.check_arith(ops.gemm_f32(ad, bd, bias=biasd, act=ACT_GELU, alpha=a01, backend=be), g64, Su, K, "gemm_f32 GELU", extra=extra))
    f.done()


@pytest.mark.parametrize("afmt", [FP8_E4M3, FP8_E5M2], ids=["e4m3", "e5m2"])
def test_gemm_fp8_every_element_within_the_accumulation_bound(be, dev, afmt):
    g = torch.Generator().manual_seed(4 + afmt)
    Mp = 304                                         # quant_fp8 takes multiples of 16 elements
    a8 = ops.quant_fp8(torch.randn(Mp, K, generator=g).to(dev), None, afmt, None, backend=be)[:M].contiguous()
    b8 = ops.quant_fp8((torch.randn(N + 8, K, generator=g) * 0.2).to(dev), None, FP8_E4M3, None, backend=be)[:N].contiguous()
    deq = lambda t, fmt: t.cpu().view(torch.float8_e4m3fn if fmt == FP8_E4M3 else torch.float8_e5m2).double()
    a, b = deq(a8, afmt), deq(b8, FP8_E4M3)
    bias, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    sa, sb = torch.tensor([0.37]), torch.tensor([1.9])
    alpha = float(sa) * float(sb)                    # the product of the two float32 scales (its own rounding is one of the bound's + 4)
    ref = alpha * (a @ b.t())
    biasd, resd, sad, sbd = (t.to(dev) for t in (bias, res, sa, sb))
    tag = f"fp8 a_fmt {afmt}"
    f = Forms(be, None, tag)
    f.run("fp32", lambda: gb.check_arith(ops.gemm_fp8_nt(a8, b8, sad, sbd, a_fmt=afmt, out_dtype=F32, backend=be), ref, gb.arith_unit(a, b, alpha=alpha), K, tag + " fp32"))
    f.run("fp32 bias residual", lambda: gb.check_arith(ops.gemm_fp8_nt(a8, b8, sad, sbd, a_fmt=afmt, out_dtype=F32, bias=biasd, residual=resd, backend=be),
                                                      ref + bias.double() + res.double(), gb.arith_unit(a, b, alpha=alpha, bias=bias, residual=res), K, tag + " fp32 bias residual"))
    f.run("bf16 bias", lambda: gb.check_arith(ops.gemm_fp8_nt(a8, b8, sad, sbd, a_fmt=afmt, bias=biasd, backend=be), ref + bias.double(), gb.arith_unit(a, b, alpha=alpha, bias=bias), K,
                                             tag + " bf16 bias"))
    u16 = torch.randn(M, N, generator=g).bfloat16()
    acc = a @ b.t()
    u = acc + bias.double()
    Su = gb.arith_unit(a, b, bias=bias)
    g64 = gb.gelu(u)
    g_extra = (gb.GELU_GRAD_MAX - 1.0) * gb.arith_bound(Su, K) + gb.act_slack(gb.gelu(u.float()), g64)[0]
    dg64 = acc * gb.gelu_grad(u16.double())
    dg_extra = gb.act_slack(acc.float() * gb.gelu_grad(u16.float()), dg64)[0]
    def gelu_aux():
        aux = torch.full((M, N), float("nan"), dtype=BF16, device=dev)
        gg = ops.gemm_fp8_nt(a8, b8, a_fmt=afmt, bias=biasd, act=ACT_GELU, aux=aux, backend=be)
        gb.check_arith(aux, u, Su, K, tag + " saved pre-activation")
        gb.check_arith(gg, g64, Su, K, tag + " GELU", extra=g_extra)
    f.run("GELU + aux", gelu_aux)
    f.run("DGELU", lambda: gb.check_arith(ops.gemm_fp8_nt(a8, b8, a_fmt=afmt, act=ACT_DGELU, aux=u16.to(dev), backend=be), dg64, gb.GELU_GRAD_MAX * gb.arith_unit(a, b), K,
                                         tag + " DGELU", extra=dg_extra))
    f.done()
