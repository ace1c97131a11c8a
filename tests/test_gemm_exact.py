"""Every GEMM kernel structure, operand format and epilogue form on operands whose correct result is ONE bit pattern per element (tests/gemmbound.py): A and B from
{+-1, +-2, +-3}, so that every partial sum in any order -- tiles, k-tile pairs, split-K slabs, stream-K partials -- is exact in the fp32 accumulator, and epilogue
operands that keep every intermediate exact.  A dropped, duplicated or misplaced product moves an element by at least 1; no tolerance is involved.  The GELU-class
epilogues run on an exact pre-activation (B x 2^-4) under the half-ulp rule.  Each case forces its kernel and asserts vdk_gemm_last_kernel().

Combinations that vdk_gemm_bf16_nt documents as unsupported and that are therefore ABSENT from the grids (or asserted to raise where said):
  * fp16 operands on the eight-wave kernel 2 and its stream-K launch 3, with a_colsum and with conv (VdkGemmDesc.ab_dtype): kernels 1, 5, 6 only;
  * col_scale / row_scale with a 16-bit output, an activation, split-K, TN or a row remap (asserted to raise for the 16-bit output); row_scale without a residual;
  * split-K with a fused epilogue; TN with M % 8 != 0 or K % 64 != 0; a_colsum with M % 256 != 0 or off kernel 2; c_colsum off the plain / dGELU 16-bit forms;
  * the persistent four-wave kernel 5 multiplies k-tiles in pairs: K % 128 != 0 is handed to kernel 2 (bf16) or kernel 6 (fp16) -- asserted, not excluded;
  * a_row_group is served by kernel 2 whatever is forced (asserted); the implicit convolution runs on kernel 1 (forward, transposed) and kernel 5 (weight gradient);
  * fp8: M, N >= 256, K % 128 == 0, the q8 copy with the GELU / dGELU forms and N % 64 == 0 only.
The (M, N, K) cross {264, 300} x {136, 264, 520} x {64, 128, 192, 384} is thinned to NT_SHAPES (every value of every dimension, both M with an odd and an even k-tile count) and, for the activation forms, to ACT_SHAPES for
the run time of the emulated suite: by shape, never by kernel structure or epilogue form.  What went: 20 of the 24 (M, N, K) triples of the cross; at K = 192 / 384
only BASIC_FORMS run (the other store forms differ in the epilogue alone and run at K = 64 / 128 on every kernel and format); the emulated walk runs BASIC_FORMS."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from tests import gemmbound as gb
from visiondk_amd import ops
from visiondk_amd.ops import ACT_DGELU, ACT_GELU, ACT_GELU_SAVE_GRAD, ACT_MUL_AUX, FP8_E4M3, FP8_E5M2

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
NT_SHAPES = [(264, 136, 64), (300, 520, 128), (264, 264, 192), (300, 136, 384)]
KERN_FMT = [(1, BF16), (1, F16), (2, BF16), (5, BF16), (5, F16), (6, BF16), (6, F16)]
_ids = lambda v: {BF16: "bf16", F16: "fp16"}.get(v, None) if isinstance(v, torch.dtype) else None


def served(kern, dtype, K):
    """the kernel that serves an NT / TN problem when `kern` is forced: kernel 5 hands K % 128 != 0 to the eight-wave kernel (bf16) or the 256x128 kernel (fp16)"""
    if kern == 5 and K % 128:
        return 2 if dtype == BF16 else 6
    return kern


@contextlib.contextmanager
def forced(be, kern):
    be.lib.vdk_gemm_force_kernel(kern)
    try:
        yield
    finally:
        be.lib.vdk_gemm_force_kernel(0)


class Forms:
    """runs the forms of one case, asserts the kernel after each, collects every failure (one wrong form does not hide the next)"""
    def __init__(self, be, want_kernel, tag):
        self.be, self.want, self.tag, self.errors, self.n = be, want_kernel, tag, [], 0

    def run(self, what, fn, kernel=None):
        self.n += 1
        try:
            fn()
            k = self.be.lib.vdk_gemm_last_kernel()
            want = self.want if kernel is None else kernel       # (None: vdk_gemm_f32_nt / vdk_gemm_fp8_nt have ONE kernel structure each and no dispatcher record)
            assert want is None or k == want, f"served by kernel {k}, expected {want}"
        except AssertionError as e:
            self.errors.append(f"[{self.tag}] {what}: {e}")

    def done(self):
        assert not self.errors, f"{len(self.errors)} of {self.n} forms failed:\n" + "\n".join(self.errors)


def _tokens(M):
    """(samples, patch rows per sample) with samples * rows == M and a 256-row tile edge inside a sample"""
    np_ = {264: 44, 300: 50, 1300: 50}[M]
    return M // np_, np_


# ---------------------------------------------------------------------------------------------------------------- NT: store forms
@pytest.mark.parametrize("M,N,K", NT_SHAPES)
@pytest.mark.parametrize("kern,dtype", KERN_FMT, ids=_ids)
def test_nt_store_forms_are_bit_exact(be, dev, kern, dtype, M, N, K):
    """every store form at 1 and 2 k-tiles; at 3 and 6 k-tiles (the main loop's other trip counts, and kernel 5's hand-over) the three forms BASIC_FORMS names"""
    _nt_store_forms(be, dev, kern, dtype, M, N, K, seed=M + N + K + kern, full=K <= 128)


BASIC_FORMS = ("plain 16-bit", "bias 16-bit", "fp32 bias residual")      # one compile-time form of each store path: 16-bit direct, 16-bit row-staged, fp32 slab


def _nt_store_forms(be, dev, kern, dtype, M, N, K, seed, full=True):
    a, b = gb.exact_operands(M, N, K, dtype, seed)
    acc = gb.acc_exact(a, b)
    bias, res, cs = gb.exact_bias(N, seed), gb.exact_residual(M, N, seed), gb.exact_col_scale(N, seed)
    RPS = 49
    rs = gb.exact_row_scale((M + RPS - 1) // RPS, seed)
    ad, bd, biasd, resd, csd, rsd = (t.to(dev) for t in (a, b, bias, res, cs, rs))
    f = Forms(be, served(kern, dtype, K), f"kernel {kern} {dtype} {M}x{N}x{K}")
    E = gb.epilogue_exact
    with forced(be, kern):
        f.run("plain 16-bit", lambda: gb.check_exact(ops.gemm_nt(ad, bd, backend=be), gb.to_out(acc, dtype), "plain 16-bit"))
        f.run("bias 16-bit", lambda: gb.check_exact(ops.gemm_nt(ad, bd, bias=biasd, backend=be), gb.to_out(E(acc, bias=bias), dtype), "bias 16-bit"))
        f.run("fp32 bias residual", lambda: gb.check_exact(ops.gemm_nt(ad, bd, out_dtype=F32, bias=biasd, residual=resd, backend=be),
                                                          gb.to_out(E(acc, bias=bias, residual=res), F32), "fp32 bias residual"))
        if not full:
            f.done()
            return
        f.run("fp32 plain", lambda: gb.check_exact(ops.gemm_nt(ad, bd, out_dtype=F32, backend=be), gb.to_out(acc, F32), "fp32 plain"))
        f.run("fp32 bias", lambda: gb.check_exact(ops.gemm_nt(ad, bd, out_dtype=F32, bias=biasd, backend=be), gb.to_out(E(acc, bias=bias), F32), "fp32 bias"))
        f.run("alpha 0.5 fp32 bias residual", lambda: gb.check_exact(ops.gemm_nt(ad, bd, out_dtype=F32, bias=biasd, residual=resd, alpha=0.5, backend=be),
                                                                    gb.to_out(E(acc, alpha=0.5, bias=bias, residual=res), F32), "alpha 0.5 fp32"))
        f.run("alpha 0.5 16-bit", lambda: gb.check_exact(ops.gemm_nt(ad, bd, alpha=0.5, backend=be), gb.to_out(E(acc, alpha=0.5), dtype), "alpha 0.5 16-bit"))
        f.run("col_scale", lambda: gb.check_exact(ops.gemm_nt(ad, bd, out_dtype=F32, bias=biasd, col_scale=csd, backend=be),
                                                 gb.to_out(E(acc, col_scale=cs, bias=bias), F32), "col_scale"))
        f.run("col_scale residual", lambda: gb.check_exact(ops.gemm_nt(ad, bd, out_dtype=F32, bias=biasd, residual=resd, col_scale=csd, backend=be),
                                                          gb.to_out(E(acc, col_scale=cs, bias=bias, residual=res), F32), "col_scale residual"))
        f.run("row_scale", lambda: gb.check_exact(ops.gemm_nt(ad, bd, out_dtype=F32, bias=biasd, residual=resd, row_scale=rsd, rows_per_scale=RPS, backend=be),
                                                 gb.to_out(E(acc, bias=bias, row_scale=rs, rows_per_scale=RPS, residual=res), F32), "row_scale"))
        # token-row remap into a [B, 1 + np, D] buffer whose class rows must keep their bits; pos_embed is the residual
        Bs, np_ = _tokens(M)
        pos = gb.exact_residual(1 + np_, N, seed + 1)
        fill = torch.full((Bs, 1 + np_, N), float("nan")); fill[:, 0] = torch.randn(Bs, N, generator=torch.Generator().manual_seed(seed))
        want = fill.clone()
        want[:, 1:] = gb.to_out(E(acc, bias=bias) + pos[1:].double().repeat(Bs, 1), F32).view(Bs, np_, N)
        def rowgroup():
            buf = fill.clone().to(dev).view(Bs * (1 + np_), N)
            ops.gemm_nt(ad, bd, out_dtype=F32, bias=biasd, residual=pos.to(dev), row_group=np_, out=buf, backend=be)
            gb.check_exact(buf, want.view(Bs * (1 + np_), N), "row_group > 0")
        f.run("row_group > 0", rowgroup)
        f.run("row_group < 0", lambda: gb.check_exact(ops.gemm_nt(ad, bd, out_dtype=F32, bias=biasd, residual=pos[1:].contiguous().to(dev), row_group=-np_, backend=be),
                                                     gb.to_out(E(acc, bias=bias) + pos[1:].double().repeat(Bs, 1), F32), "row_group < 0"))
        wide = torch.full((M, K + 24), 7.0, dtype=dtype); wide[:, 8:8 + K] = a       # lda > K, 16-byte aligned start; what lies beside the operand is not zero
        av = wide.to(dev)[:, 8:8 + K]
        f.run("strided A fp32", lambda: gb.check_exact(ops.gemm_nt(av, bd, out_dtype=F32, bias=biasd, residual=resd, backend=be), gb.to_out(E(acc, bias=bias, residual=res), F32), "strided A fp32"))
        f.run("strided A 16-bit", lambda: gb.check_exact(ops.gemm_nt(av, bd, bias=biasd, backend=be), gb.to_out(E(acc, bias=bias), dtype), "strided A 16-bit"))
        rows = be.lib.vdk_gemm_c_colsum_rows(M, N, K)
        assert (rows > 0) == (kern != 1)
        if rows > 0:      # by-product: column sums of the STORED 16-bit output -- integers, exact in any order
            def ocs():
                part = torch.full((rows, N), float("nan"), dtype=F32, device=dev)
                out = ops.gemm_nt(ad, bd, c_colsum=part, backend=be)
                gb.check_exact(out, gb.to_out(acc, dtype), "plain 16-bit + c_colsum")
                gb.check_exact(part.sum(0)[None], out.double().sum(0).float()[None].cpu(), "c_colsum")
            f.run("c_colsum", ocs)
    with pytest.raises(Exception):      # 16-bit outputs do not take col_scale / row_scale
        ops.gemm_nt(ad, bd, bias=biasd, col_scale=csd, backend=be)
    with pytest.raises(Exception):
        ops.gemm_nt(ad, bd, bias=biasd, residual=resd, row_scale=rsd, rows_per_scale=RPS, backend=be)
    f.done()


# ---------------------------------------------------------------------------------------------------------------- NT: activation forms
ACT_SHAPES = [(300, 264, 128), (264, 136, 192)]


@pytest.mark.parametrize("M,N,K", ACT_SHAPES)
@pytest.mark.parametrize("kern,dtype", KERN_FMT, ids=_ids)
def test_nt_activation_forms_on_an_exact_pre_activation(be, dev, kern, dtype, M, N, K):
    seed = M + N + K + kern + 7
    a, b = gb.exact_operands(M, N, K, dtype, seed, b_shift=gb.GELU_SHIFT)
    dy, _ = gb.exact_operands(M, 8, K, dtype, seed + 1)
    bias = gb.exact_bias(N, seed)
    u = gb.epilogue_exact(gb.acc_exact(a, b, b_shift=gb.GELU_SHIFT), bias=bias)            # u = acc / 16 + bias, exact
    acc2 = gb.acc_exact(dy, b, b_shift=gb.GELU_SHIFT)
    u16 = gb.to_out(u, dtype)                                                            # the saved pre-activation: RNE16(u)
    g64 = gb.gelu(u)
    g_slack, _ = gb.act_slack(gb.gelu(u.float()), g64)
    d64 = gb.gelu_grad(u)
    d_slack, _ = gb.act_slack(gb.gelu_grad(u.float()), d64)
    d16 = d64.float().half()                                                             # a given fp16 derivative for the one-multiplication backward
    # dGELU: the exact accumulator times GELU' of the GIVEN 16-bit pre-activation
    dg64 = acc2 * gb.gelu_grad(u16.double())
    dg_slack, _ = gb.act_slack(acc2.float() * gb.gelu_grad(u16.float()), dg64)
    mul64 = acc2 * d16.double()
    ad, bd, dyd, biasd, u16d, d16d = (t.to(dev) for t in (a, b, dy, bias, u16, d16))
    f = Forms(be, served(kern, dtype, K), f"kernel {kern} {dtype} {M}x{N}x{K}")
    with forced(be, kern):
        def gelu_aux():
            aux = torch.full((M, N), float("nan"), dtype=dtype, device=dev)
            g = ops.gemm_nt(ad, bd, bias=biasd, act=ACT_GELU, aux=aux, backend=be)
            gb.check_exact(aux, u16, "saved pre-activation")
            gb.check_half_ulp(g, g64, g_slack, "GELU")
        f.run("GELU + aux", gelu_aux)
        def gelu_save_grad():
            dsv = torch.full((M, N), float("nan"), dtype=F16, device=dev)
            g = ops.gemm_nt(ad, bd, bias=biasd, act=ACT_GELU_SAVE_GRAD, aux=dsv, backend=be)
            gb.check_half_ulp(g, g64, g_slack, "GELU (derivative saved)")
            gb.check_half_ulp(dsv, d64, d_slack, "saved fp16 GELU'")
        f.run("GELU_SAVE_GRAD", gelu_save_grad)
        f.run("DGELU", lambda: gb.check_half_ulp(ops.gemm_nt(dyd, bd, act=ACT_DGELU, aux=u16d, backend=be), dg64, dg_slack, "DGELU"))
        f.run("MUL_AUX", lambda: gb.check_exact(ops.gemm_nt(dyd, bd, act=ACT_MUL_AUX, aux=d16d, backend=be), gb.to_out(mul64, dtype), "MUL_AUX"))
        rows = be.lib.vdk_gemm_c_colsum_rows(M, N, K)
        if rows > 0:      # the same two backward forms with the column sums of what they store: same bits, sums within the fp32 bound of M additions
            def with_ocs(act, aux, name):
                part = torch.full((rows, N), float("nan"), dtype=F32, device=dev)
                out = ops.gemm_nt(dyd, bd, act=act, aux=aux, c_colsum=part, backend=be)
                gb.check_exact(out, ops.gemm_nt(dyd, bd, act=act, aux=aux, backend=be), name + " + c_colsum")
                gb.check_within(part.sum(0)[None].cpu(), out.double().sum(0)[None].cpu(), gb.arith_bound(out.double().abs().sum(0)[None].cpu(), M), name + " c_colsum")
            f.run("DGELU + c_colsum", lambda: with_ocs(ACT_DGELU, u16d, "DGELU"))
            f.run("MUL_AUX + c_colsum", lambda: with_ocs(ACT_MUL_AUX, d16d, "MUL_AUX"))
    f.done()


# ---------------------------------------------------------------------------------------------------------------- NT: a_colsum, split-K, stream-K
@pytest.mark.parametrize("M,N,K", [(512, 264, 192), (256, 520, 128)])
def test_a_colsum_byproduct_is_bit_exact(be, dev, M, N, K):
    a, b = gb.exact_operands(M, N, K, BF16, M + K)
    acc = gb.acc_exact(a, b)
    ad, bd = a.to(dev), b.to(dev)
    f = Forms(be, 2, f"kernel 2 a_colsum {M}x{N}x{K}")
    with forced(be, 2):
        rows = be.lib.vdk_gemm_a_colsum_rows(M, N, K)
        assert rows == M // 256 and be.lib.vdk_gemm_a_colsum_rows(300, N, K) == 0
        for dt in (BF16, F32):
            def run(dt=dt):
                with forced(be, 1):
                    ops.gemm_nt(ad[:8], bd[:8], backend=be)                      # leaves "1" in the dispatcher's record: the by-product launch must write its own
                be.lib.vdk_gemm_force_kernel(2)
                part = torch.full((rows, K), float("nan"), dtype=F32, device=dev)
                gb.check_exact(ops.gemm_nt(ad, bd, out_dtype=dt, a_colsum=part, backend=be), gb.to_out(acc, dt), "output")
                gb.check_exact(part.sum(0)[None], a.double().sum(0).float()[None], "a_colsum")
            f.run(f"a_colsum {dt}", run)
    f.done()


@pytest.mark.parametrize("kern,dtype", [(2, BF16), (5, BF16), (5, F16), (6, BF16), (6, F16)], ids=_ids)
@pytest.mark.parametrize("M,N,K,splitk", [(300, 136, 192, 2), (264, 264, 384, 2), (264, 136, 640, 3), (300, 264, 320, 3)])
def test_nt_split_k_is_bit_exact(be, dev, kern, dtype, M, N, K, splitk):
    """ragged last split: 192 = 128 + 64, 384 = 256 + 128, 640 = 256 + 256 + 128, 320 = 128 + 128 + 64"""
    a, b = gb.exact_operands(M, N, K, dtype, M + K + kern)
    acc = gb.acc_exact(a, b)
    ad, bd = a.to(dev), b.to(dev)
    f = Forms(be, served(kern, dtype, K), f"kernel {kern} {dtype} {M}x{N}x{K} / {splitk}")
    with forced(be, kern):
        f.run("fp32", lambda: gb.check_exact(ops.gemm_nt(ad, bd, out_dtype=F32, splitk=splitk, backend=be), gb.to_out(acc, F32), "split-K fp32"))
        f.run("16-bit", lambda: gb.check_exact(ops.gemm_nt(ad, bd, splitk=splitk, backend=be), gb.to_out(acc, dtype), "split-K 16-bit"))
        f.run("alpha", lambda: gb.check_exact(ops.gemm_nt(ad, bd, out_dtype=F32, splitk=splitk, alpha=0.5, backend=be), gb.to_out(acc * 0.5, F32), "split-K alpha"))
    f.done()


@pytest.mark.parametrize("grid", [8, 16])
@pytest.mark.parametrize("M,N,K", [(520, 520, 256), (600, 776, 384)])
def test_stream_k_is_bit_exact_and_leaves_its_counters_zero(be, dev, M, N, K, grid):
    a, b = gb.exact_operands(M, N, K, BF16, M + K + grid)
    _, bs = gb.exact_operands(M, N, K, BF16, M + K + grid, b_shift=gb.GELU_SHIFT)
    acc = gb.acc_exact(a, b)
    bias, res = gb.exact_bias(N, grid), gb.exact_residual(M, N, grid)
    ad, bd, biasd, resd = (t.to(dev) for t in (a, b, bias, res))
    u = gb.epilogue_exact(gb.acc_exact(a, bs, b_shift=gb.GELU_SHIFT), bias=bias)
    g64 = gb.gelu(u)
    g_slack, _ = gb.act_slack(gb.gelu(u.float()), g64)
    f = Forms(be, 3, f"stream-K grid {grid} {M}x{N}x{K}")
    be.lib.vdk_gemm_streamk_grid(grid)
    try:
        with forced(be, 3):
            ws = ops.streamk_workspace(dev, backend=be)
            f.run("fp32 bias residual", lambda: gb.check_exact(ops.gemm_nt(ad, bd, out_dtype=F32, bias=biasd, residual=resd, streamk_ws=ws, backend=be),
                                                              gb.to_out(gb.epilogue_exact(acc, bias=bias, residual=res), F32), "fp32 bias residual"))
            f.run("bias 16-bit", lambda: gb.check_exact(ops.gemm_nt(ad, bd, bias=biasd, streamk_ws=ws, backend=be), gb.to_out(gb.epilogue_exact(acc, bias=bias), BF16), "bias 16-bit"))
            f.run("plain 16-bit", lambda: gb.check_exact(ops.gemm_nt(ad, bd, streamk_ws=ws, backend=be), gb.to_out(acc, BF16), "plain 16-bit"))
            f.run("fp32 plain", lambda: gb.check_exact(ops.gemm_nt(ad, bd, out_dtype=F32, streamk_ws=ws, backend=be), gb.to_out(acc, F32), "fp32 plain"))
            def gelu_aux():
                aux = torch.full((M, N), float("nan"), dtype=BF16, device=dev)
                g = ops.gemm_nt(ad, bs.to(dev), bias=biasd, act=ACT_GELU, aux=aux, streamk_ws=ws, backend=be)
                gb.check_exact(aux, gb.to_out(u, BF16), "saved pre-activation")
                gb.check_half_ulp(g, g64, g_slack, "GELU")
            f.run("GELU + aux", gelu_aux)
            assert int(ws[:65536].view(torch.int32).abs().sum()) == 0, "tile counters not left at zero"
    finally:
        be.lib.vdk_gemm_streamk_grid(0)
    f.done()


# ---------------------------------------------------------------------------------------------------------------- TN
TN_SHAPES = [(64, 264, 136, 1, 0), (192, 72, 264, 1, 0), (512, 264, 136, 1, 0), (192, 264, 136, 2, 0), (512, 264, 264, 3, 0), (192, 264, 264, 1, 16)]
TN_CASES = [(kern, dtype) + sh for kern, dtype in [(2, BF16), (5, BF16), (5, F16), (6, BF16), (6, F16)] for sh in TN_SHAPES
            if not (sh[4] and dtype == F16)]      # a_row_group is the eight-wave kernel's, which is bf16 only


@pytest.mark.parametrize("kern,dtype,K,M,N,splitk,rg", TN_CASES, ids=lambda v: _ids(v) if isinstance(v, torch.dtype) else str(v))
def test_tn_is_bit_exact(be, dev, kern, dtype, K, M, N, splitk, rg):
    """C = A^T B from k-major operands; M % 8 == 0, ragged against 256; split-K (192 = 128 + 64, 512 = 256 + 256: whole pairs of k-tiles per split); the token-row remap"""
    at, bt = gb.exact_operands(K, K, M, dtype, K + M + kern)[0], gb.exact_operands(K, K, N, dtype, K + N + kern + 1)[0]      # [K, M], [K, N]
    acc = gb.acc_exact(at, bt, a_kmajor=True, b_kmajor=True)
    if rg:
        phys = K + K // rg + 1
        a_full = torch.full((phys, M), 5.0, dtype=dtype)           # the class rows between the groups hold something that must not be multiplied
        a_full[torch.tensor([t + t // rg + 1 for t in range(K)])] = at
    else:
        a_full = at
    ad, bd = a_full.to(dev), bt.to(dev)
    kps = K if splitk == 1 else ((K + splitk - 1) // splitk + (127 if K % 128 == 0 else 63)) // (128 if K % 128 == 0 else 64) * (128 if K % 128 == 0 else 64)
    want_k = 2 if rg else (served(kern, dtype, K) if kps % 128 == 0 or kern != 5 else (2 if dtype == BF16 else 6))
    f = Forms(be, want_k, f"TN kernel {kern} {dtype} K {K} {M}x{N} / {splitk} rg {rg}")
    kw = dict(trans=True, a_row_group=rg, a_rows=K, backend=be)
    with forced(be, kern):
        f.run("fp32", lambda: gb.check_exact(ops.gemm_nt(ad, bd, out_dtype=F32, splitk=splitk, **kw), gb.to_out(acc, F32), "TN fp32"))
        f.run("16-bit", lambda: gb.check_exact(ops.gemm_nt(ad, bd, splitk=splitk, **kw), gb.to_out(acc, dtype), "TN 16-bit"))
        if splitk == 1:
            f.run("alpha (run-time-flag form)", lambda: gb.check_exact(ops.gemm_nt(ad, bd, out_dtype=F32, alpha=0.5, **kw), gb.to_out(acc * 0.5, F32), "TN alpha"))
    f.done()


# ---------------------------------------------------------------------------------------------------------------- the persistent walk
@pytest.mark.parametrize("kern,dtype", [(5, BF16), (5, F16), (6, BF16), (6, F16)], ids=_ids)
def test_walk_on_the_emulated_cus(emu, kern, dtype):
    """1300 x 776 x 128: 24 tiles of 256x256 / 42 of 256x128 on the 16 emulated CUs -- the walk onto the next tile with the DMA cursor running into it"""
    _nt_store_forms(emu, "cpu", kern, dtype, 1300, 776, 128, seed=kern, full=False)


@pytest.mark.gpu
@pytest.mark.parametrize("kern,dtype", [(5, BF16), (5, F16), (6, BF16), (6, F16)], ids=_ids)
def test_walk_on_the_real_cus(hip, kern, dtype):
    """more tiles than the device has CUs (kernel 5: 256x256 tiles, about 17 x 17 on 256 CUs) resp. more than twice as many 256x128 tiles as CUs (kernel 6), ragged in M and
    N, K = 128: fp32 + bias + residual and bias 16-bit, bit-exact"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if kern == 5:
        t = int(cus ** 0.5) + 1                      # t x t > CUs
        M, N = 256 * (t - 1) + 44, 256 * (t - 1) + 8
        assert t * t > cus
    else:
        tm = int((2 * cus) ** 0.5 / 1.4) + 1         # tm x tn > 2 CUs with tn about twice tm
        tn = (2 * cus) // tm + 1
        M, N = 256 * (tm - 1) + 44, 128 * (tn - 1) + 8
        assert tm * tn > 2 * cus
    _nt_store_forms(hip, "cuda", kern, dtype, M, N, 128, seed=kern, full=False)


# ---------------------------------------------------------------------------------------------------------------- implicit convolution
@pytest.mark.parametrize("k,s,p,Ci", [(3, 1, 1, 16), (3, 2, 1, 16), (1, 2, 0, 16), (7, 2, 3, 3)])
@pytest.mark.parametrize("H,Co", [(7, 24), (9, 72)])
def test_implicit_convolution_is_bit_exact(be, dev, k, s, p, Ci, H, Co):
    """integer NHWC input and integer weights against float64 conv2d and its gradients: forward, transposed (input gradient) and the rows-form weight gradient
    (rows = 3 * OH * OW is never a multiple of 128); Cin 3 is padded to 8"""
    B = 3
    g = torch.Generator().manual_seed(k * 100 + s * 10 + H)
    draw = lambda *shape: torch.tensor(gb.VALUES, dtype=torch.float64)[torch.randint(0, 6, shape, generator=g)]
    x, w = draw(B, Ci, H, H), draw(Co, Ci, k, k)
    OH = (H + 2 * p - k) // s + 1
    dy = draw(B, Co, OH, OH)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, stride=s, padding=p)
    y.backward(dy)
    for t in (y.detach(), xr.grad, wr.grad):
        gb.assert_f32_exact(t, "convolution reference")
    cip = (Ci + 7) // 8 * 8
    a = ops.nchw_to_nhwc_bf16(x.float().to(dev), cip, backend=be)
    wf, wd = ops.conv_weight_prep(w.float().to(dev), cip, backend=be)
    dyb = dy.permute(0, 2, 3, 1).contiguous().float().bfloat16().to(dev)
    f = Forms(be, 1, f"conv {k}x{k} s{s} p{p} Cin {Ci} H {H} Co {Co}")
    nchw = lambda t, h, c: t.cpu().view(B, h, h, c).permute(0, 3, 1, 2)
    f.run("forward", lambda: gb.check_exact(nchw(ops.conv_gemm(a, wf, oh=OH, ow=OH, kh=k, kw=k, stride=s, pad=p, backend=be), OH, Co).reshape(B * Co, -1),
                                           y.detach().float().reshape(B * Co, -1), "forward"))
    f.run("forward 16-bit", lambda: gb.check_exact(nchw(ops.conv_gemm(a, wf, oh=OH, ow=OH, kh=k, kw=k, stride=s, pad=p, out_dtype=BF16, backend=be), OH, Co).reshape(B * Co, -1),
                                                  y.detach().float().bfloat16().reshape(B * Co, -1), "forward 16-bit"))
    def dgrad():
        dx = nchw(ops.conv_gemm(dyb, wd, oh=H, ow=H, kh=k, kw=k, stride=s, pad=p, transposed=True, backend=be), H, cip)
        gb.check_exact(dx[:, :Ci].reshape(B * Ci, -1), xr.grad.float().reshape(B * Ci, -1), "transposed")
        assert int(torch.count_nonzero(dx[:, Ci:])) == 0, "padded input channels received a gradient"
    f.run("transposed", dgrad)
    for sk in (1, 2):
        def wgrad(sk=sk):
            dwi = ops.conv_wgrad_implicit(dyb.view(-1, Co), a, oh=OH, ow=OH, kh=k, kw=k, stride=s, pad=p, splitk=sk, backend=be)
            gb.check_exact(ops.conv_wgrad_unpermute(dwi, Ci, k, k, backend=be).cpu().reshape(Co, -1), wr.grad.float().reshape(Co, -1), f"weight gradient / {sk}")
        f.run(f"rows-form weight gradient / {sk}", wgrad, kernel=5)
    f.done()


# ---------------------------------------------------------------------------------------------------------------- fp32 MFMA GEMM
@pytest.mark.parametrize("M,N,K", [(72, 40, 64), (132, 200, 100), (264, 136, 192)])
def test_gemm_f32_is_bit_exact(be, dev, M, N, K):
    seed = M + K
    a, b = gb.exact_operands(M, N, K, F32, seed)
    acc = gb.acc_exact(a, b)
    bias, res = gb.exact_bias(N, seed), gb.exact_residual(M, N, seed)
    ad, bd, biasd, resd = (t.to(dev) for t in (a, b, bias, res))
    bt, at_ = b.t().contiguous().to(dev), a.t().contiguous().to(dev)
    f = Forms(be, None, f"gemm_f32 {M}x{N}x{K}")
    run = f.run
    run("plain", lambda: gb.check_exact(ops.gemm_f32(ad, bd, backend=be), gb.to_out(acc, F32), "plain"))
    run("bias residual alpha", lambda: gb.check_exact(ops.gemm_f32(ad, bd, bias=biasd, residual=resd, alpha=0.5, backend=be),
                                                      gb.to_out(gb.epilogue_exact(acc, alpha=0.5, bias=bias, residual=res), F32), "bias residual alpha"))
    run("b_kmajor", lambda: gb.check_exact(ops.gemm_f32(ad, bt, b_kmajor=True, backend=be), gb.to_out(acc, F32), "b_kmajor"))
    run("a_kmajor b_kmajor", lambda: gb.check_exact(ops.gemm_f32(at_, bt, a_kmajor=True, b_kmajor=True, backend=be), gb.to_out(acc, F32), "a_kmajor b_kmajor"))
    run("k_splits 3", lambda: gb.check_exact(ops.gemm_f32(ad, bd, k_splits=3, backend=be), gb.to_out(acc, F32), "k_splits 3"))          # 64 = 24 + 24 + 16, 100 = 36 + 36 + 28, 192 = 3 x 64
    run("k_splits 3 k-major", lambda: gb.check_exact(ops.gemm_f32(at_, bt, a_kmajor=True, b_kmajor=True, k_splits=3, backend=be), gb.to_out(acc, F32), "k_splits 3 k-major"))
    a4, b4 = gb.exact_operands(M, N, K, F32, seed, b_shift=gb.GELU_SHIFT)
    u = gb.epilogue_exact(gb.acc_exact(a4, b4, b_shift=gb.GELU_SHIFT), bias=bias)
    g64 = gb.gelu(u)
    slack, _ = gb.act_slack(gb.gelu(u.float()), g64)
    run("GELU", lambda: gb.check_within(ops.gemm_f32(a4.to(dev), b4.to(dev), bias=biasd, act=ACT_GELU, backend=be), g64, slack, "GELU fp32"))      # the slack alone: no half-ulp term
    f.done()


# ---------------------------------------------------------------------------------------------------------------- fp8
@pytest.mark.parametrize("afmt", [FP8_E4M3, FP8_E5M2], ids=["e4m3", "e5m2"])
@pytest.mark.parametrize("M,N,K", [(264, 320, 128), (300, 264, 384)])
def test_gemm_fp8_is_bit_exact(be, dev, M, N, K, afmt):
    seed = M + K + afmt
    adt = torch.float8_e4m3fn if afmt == FP8_E4M3 else torch.float8_e5m2
    a = gb.exact_operands(M, 8, K, adt, seed)[0]
    b = gb.exact_operands(8, N, K, torch.float8_e4m3fn, seed + 1)[1]
    b4 = gb.exact_operands(8, N, K, torch.float8_e4m3fn, seed + 1, b_shift=gb.GELU_SHIFT)[1]
    acc = gb.acc_exact(a.float(), b.float())
    bias, res = gb.exact_bias(N, seed), gb.exact_residual(M, N, seed)
    sa, sb = torch.tensor([0.5]), torch.tensor([0.25])                                  # power-of-two scale_inv: the scaled accumulator stays exact
    a8, b8, b48 = (t.view(torch.uint8).to(dev) for t in (a, b, b4))
    biasd, resd, sad, sbd = (t.to(dev) for t in (bias, res, sa, sb))
    E = gb.epilogue_exact
    f = Forms(be, None, f"fp8 {M}x{N}x{K} a_fmt {afmt}")
    run = f.run
    run("fp32", lambda: gb.check_exact(ops.gemm_fp8_nt(a8, b8, sad, sbd, a_fmt=afmt, out_dtype=F32, backend=be), gb.to_out(acc * 0.125, F32), "fp32"))
    run("fp32 bias residual", lambda: gb.check_exact(ops.gemm_fp8_nt(a8, b8, sad, sbd, a_fmt=afmt, out_dtype=F32, bias=biasd, residual=resd, backend=be),
                                                     gb.to_out(E(acc, alpha=0.125, bias=bias, residual=res), F32), "fp32 bias residual"))
    run("bf16", lambda: gb.check_exact(ops.gemm_fp8_nt(a8, b8, sad, sbd, a_fmt=afmt, backend=be), gb.to_out(acc * 0.125, BF16), "bf16"))
    run("bf16 bias", lambda: gb.check_exact(ops.gemm_fp8_nt(a8, b8, sad, sbd, a_fmt=afmt, bias=biasd, backend=be), gb.to_out(E(acc, alpha=0.125, bias=bias), BF16), "bf16 bias"))
    run("bf16 no scales", lambda: gb.check_exact(ops.gemm_fp8_nt(a8, b8, a_fmt=afmt, backend=be), gb.to_out(acc, BF16), "bf16 no scales"))
    u = E(gb.acc_exact(a.float(), b4.float(), b_shift=gb.GELU_SHIFT), bias=bias)
    g64 = gb.gelu(u)
    slack, _ = gb.act_slack(gb.gelu(u.float()), g64)
    def gelu_q8():
        aux = torch.full((M, N), float("nan"), dtype=BF16, device=dev)
        sc = torch.tensor([16.0], device=dev); am = torch.zeros(1, device=dev)
        g, g8 = ops.gemm_fp8_nt(a8, b48, a_fmt=afmt, bias=biasd, act=ACT_GELU, aux=aux, backend=be, q8={"fmt": FP8_E4M3, "scale": sc, "amax": am})
        gb.check_exact(aux, gb.to_out(u, BF16), "saved pre-activation")
        gb.check_half_ulp(g, g64, slack, "GELU")
        am_ref = torch.zeros(1, device=dev)
        gb.check_exact(g8, ops.quant_fp8(g, sc, FP8_E4M3, am_ref, backend=be), "q8 copy")
        assert torch.equal(am, am_ref) and am.item() > 0
    if N % 64 == 0:
        run("GELU + aux + q8", gelu_q8)
    f.done()
