"""The LayerScale residual kernels (csrc/layerscale_residual.hip: vdk_ls_residual_fwd / vdk_ls_residual_bwd) against torch, on the CPU SIMT emulation and on the device.

  y  = x + gamma * float(h)          one fp32 multiply and one fp32 add per element: torch's fp32 `x + gamma * h.float()` BIT FOR BIT
  dh = RNE16(gamma * dy)             torch's `(gamma * dy).to(dtype)` bit for bit, subnormal fp16 results included
  dgamma[c] = sum_r dy[r, c] h[r, c] in fp32, a fixed order: bit-exact on integer operands (tests/gemmbound.py's VALUES: every partial sum in any order is an integer below
                                     9 rows < 2^24), within gemmbound's a-priori bound 2 (rows + 4) 2^-24 sum |dy h| on Gaussian operands, and the same bits on a second call.

Every 2-D operand lies at pitch C + 8 with NaN between the rows; the NaNs must still be there afterwards.  By construction of the inputs a dropped row changes y, dh and the
integer dgamma; a column taken from its neighbour changes them because gamma cycles through {1e-5, 2^-20, +u, -u} (u in [0.05, 1]) and every column has its own magnitude; h read
as the other 16-bit format changes y and dgamma (Gaussian h means something else in the other format)."""
import ctypes as C

import pytest
import torch

from tests.gemmbound import VALUES, arith_bound, assert_f32_exact

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
OPF = {BF: 0, HF: 1}
PAD = 8
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4
ROWS, COLS = (1, 37, 52, 2740), (8, 384, 1024)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _padded(x, dev):
    """-> (the [rows, C + PAD] tensor on dev with NaN in the padding, its [rows, C] window)"""
    rows, Cc = x.shape
    big = torch.full((rows, Cc + PAD), float("nan"), dtype=x.dtype)
    big[:, :Cc] = x
    big = big.to(dev)
    return big, big[:, :Cc]


def _pad_intact(big, Cc):
    return bool(torch.isnan(big[:, Cc:].float()).all())


def make_gamma(Cc, g, all_tiny=False):
    """column c: 1e-5 | 2^-20 | +u | -u by c mod 4, u uniform in [0.05, 1]: neighbours always differ"""
    if all_tiny:
        return torch.full((Cc,), 1e-5)
    u = 0.05 + 0.95 * torch.rand(Cc, generator=g)
    k = torch.arange(Cc) % 4
    return torch.where(k == 0, torch.full((Cc,), 1e-5), torch.where(k == 1, torch.full((Cc,), 2.0 ** -20), torch.where(k == 2, u, -u))).float()


def _colmag(Cc):
    return (0.5 + (torch.arange(Cc) % 5).float())[None, :]


def _sync(be):
    if be.device_only:
        torch.cuda.synchronize()


def call_fwd(be, dev, x, h, gamma):
    """-> y [rows, C] (cpu); the padding of every operand checked"""
    rows, Cc = x.shape
    xb, xv = _padded(x, dev)
    hb, hv = _padded(h, dev)
    yb, yv = _padded(torch.zeros(rows, Cc), dev)
    gd = gamma.to(dev)
    be.check(be.lib.vdk_ls_residual_fwd(xv.data_ptr(), xv.stride(0), hv.data_ptr(), hv.stride(0), be.ptr(gd), yv.data_ptr(), yv.stride(0), rows, Cc, OPF[h.dtype], be.stream()),
             "vdk_ls_residual_fwd")
    _sync(be)
    assert _pad_intact(xb, Cc) and _pad_intact(hb, Cc) and _pad_intact(yb, Cc)
    assert torch.equal(_bits(xv), _bits(x)) and torch.equal(_bits(hv), _bits(h))
    # in place: y aliases x
    be.check(be.lib.vdk_ls_residual_fwd(xv.data_ptr(), xv.stride(0), hv.data_ptr(), hv.stride(0), be.ptr(gd), xv.data_ptr(), xv.stride(0), rows, Cc, OPF[h.dtype], be.stream()),
             "vdk_ls_residual_fwd (in place)")
    _sync(be)
    assert _pad_intact(xb, Cc) and torch.equal(_bits(xv), _bits(yv)), "y aliasing x gives other bits"
    return yv.cpu()


def workspace_bytes(be, rows, Cc):
    need = C.c_size_t(0)
    be.check(be.lib.vdk_ls_residual_bwd_workspace_bytes(rows, Cc, C.byref(need)), "vdk_ls_residual_bwd_workspace_bytes")
    return need.value


def call_bwd(be, dev, dy, h, gamma):
    """-> (dh, dgamma) on the cpu from a workspace of exactly the reported size"""
    rows, Cc = dy.shape
    db, dv = _padded(dy, dev)
    hb, hv = _padded(h, dev)
    ob, ov = _padded(torch.zeros(rows, Cc, dtype=h.dtype), dev)
    gd = gamma.to(dev)
    dg = torch.full((Cc,), float("nan"), device=dev)
    n = workspace_bytes(be, rows, Cc)
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    be.check(be.lib.vdk_ls_residual_bwd(dv.data_ptr(), dv.stride(0), hv.data_ptr(), hv.stride(0), be.ptr(gd), ov.data_ptr(), ov.stride(0), be.ptr(dg), rows, Cc, OPF[h.dtype],
                                        be.ptr(ws), n, be.stream()), "vdk_ls_residual_bwd")
    _sync(be)
    assert _pad_intact(db, Cc) and _pad_intact(hb, Cc) and _pad_intact(ob, Cc)
    assert torch.equal(_bits(dv), _bits(dy)) and torch.equal(_bits(hv), _bits(h))
    return ov.cpu(), dg.cpu()


def run_case(be, dev, rows, Cc, dtype, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + rows + Cc)
    gamma = make_gamma(Cc, g)
    mag = _colmag(Cc)
    x = torch.randn(rows, Cc, generator=g) * mag
    h = (torch.randn(rows, Cc, generator=g) * mag.flip(1)).to(dtype)
    dy = torch.randn(rows, Cc, generator=g) * mag
    # forward, and dh: bit for bit
    y = call_fwd(be, dev, x, h, gamma)
    want = x + gamma * h.float()
    assert torch.equal(_bits(y), _bits(want)), f"y: {int((_bits(y) != _bits(want)).sum())} of {y.numel()} elements differ in their bits"
    dh, dg = call_bwd(be, dev, dy, h, gamma)
    want = (gamma * dy).to(dtype)
    assert torch.equal(_bits(dh), _bits(want)), f"dh: {int((_bits(dh) != _bits(want)).sum())} of {dh.numel()} elements differ in their bits"
    # dgamma on Gaussian operands: the a-priori bound of an fp32 sum of `rows` products, per column; a second call returns the same bits
    prod = dy.double() * h.double()
    err, bound = (dg.double() - prod.sum(0)).abs(), arith_bound(prod.abs().sum(0), rows)
    worst = float((err / bound).max())
    print(f"ls_residual {dtype} rows {rows} C {Cc}: dgamma worst |err| / bound {worst:.3f}")
    assert bool((err <= bound).all()), (worst, int((err / bound).argmax()))
    dh2, dg2 = call_bwd(be, dev, dy, h, gamma)
    assert torch.equal(_bits(dg), _bits(dg2)) and torch.equal(_bits(dh), _bits(dh2)), "two runs, two results"
    # dgamma on integer operands: one bit pattern
    assert 9 * rows < 2 ** 24
    pick = lambda: torch.tensor(VALUES)[torch.randint(0, len(VALUES), (rows, Cc), generator=g)]
    dyi, hi = pick(), pick().to(dtype)
    want64 = (dyi.double() * hi.double()).sum(0)
    assert_f32_exact(want64, "dgamma of the integer operands")
    dhi, dgi = call_bwd(be, dev, dyi, hi, gamma)
    assert torch.equal(_bits(dgi), _bits(want64.float())), f"dgamma (integer operands): {int((_bits(dgi) != _bits(want64.float())).sum())} of {Cc} columns differ"
    assert torch.equal(_bits(dhi), _bits((gamma * dyi).to(dtype)))


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("Cc", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_ls_residual(be, dev, rows, Cc, dtype):
    run_case(be, dev, rows, Cc, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_ls_residual_more_partials_than_one_workgroup(hip, dtype):
    """20 000 x 1024: the backward runs more than a hundred row splits per column block"""
    assert workspace_bytes(hip, 20000, 1024) > 8 * 1024 * 4
    run_case(hip, "cuda", 20000, 1024, dtype)


def test_ls_residual_fp16_subnormal_dh(be, dev):
    """gamma = 1e-5, |dy| ~ 1: gamma * dy lies below fp16's smallest normal (6.1e-5); dh keeps the subnormals torch's conversion keeps"""
    g = torch.Generator().manual_seed(3)
    rows, Cc = 52, 384
    gamma = make_gamma(Cc, g, all_tiny=True)
    dy = torch.randn(rows, Cc, generator=g)
    h = torch.randn(rows, Cc, generator=g).to(HF)
    dh, _ = call_bwd(be, dev, dy, h, gamma)
    want = (gamma * dy).to(HF)
    assert float(want.float().abs().max()) < 6.1e-5 and int((want != 0).sum()) > rows * Cc // 2
    assert int((dh != 0).sum()) > 0 and torch.equal(_bits(dh), _bits(want))


def test_ls_residual_refusals(be, dev):
    rows, Cc = 5, 16
    ld = Cc + PAD
    x, y, dy = (torch.zeros(rows, ld, device=dev) for _ in range(3))
    h, dh = (torch.zeros(rows, ld, dtype=BF, device=dev) for _ in range(2))
    gamma, dg = torch.ones(Cc + 4, device=dev), torch.zeros(Cc + 4, device=dev)
    n = workspace_bytes(be, rows, Cc)
    assert n >= Cc * 4
    ws = torch.empty(n + 16, dtype=torch.uint8, device=dev)
    p = lambda t: t.data_ptr()
    st = be.stream()

    def fwd(x_=p(x), ldx=ld, h_=p(h), ldh=ld, g_=p(gamma), y_=p(y), ldy=ld, rows_=rows, C_=Cc, opf=0):
        return be.lib.vdk_ls_residual_fwd(x_, ldx, h_, ldh, g_, y_, ldy, rows_, C_, opf, st)

    def bwd(dy_=p(dy), lddy=ld, h_=p(h), ldh=ld, g_=p(gamma), dh_=p(dh), lddh=ld, dg_=p(dg), rows_=rows, C_=Cc, opf=0, ws_=p(ws), n_=n):
        return be.lib.vdk_ls_residual_bwd(dy_, lddy, h_, ldh, g_, dh_, lddh, dg_, rows_, C_, opf, ws_, n_, st)

    assert fwd() == 0 and fwd(opf=1) == 0 and bwd() == 0 and bwd(opf=1) == 0
    for kw in (dict(C_=12), dict(C_=0), dict(rows_=0), dict(ldx=ld + 2), dict(ldh=ld + 4), dict(ldy=ld + 2), dict(ldx=Cc - 4), dict(ldh=Cc - 8), dict(ldy=Cc - 4),
               dict(x_=p(x) + 4), dict(h_=p(h) + 8), dict(g_=p(gamma) + 4), dict(y_=p(y) + 8), dict(x_=None), dict(h_=None), dict(g_=None), dict(y_=None)):
        assert fwd(**kw) == EINVAL, kw
    for kw in (dict(C_=12), dict(C_=0), dict(rows_=0), dict(lddy=ld + 2), dict(ldh=ld + 4), dict(lddh=ld + 4), dict(lddy=Cc - 4), dict(ldh=Cc - 8), dict(lddh=Cc - 8),
               dict(dy_=p(dy) + 4), dict(h_=p(h) + 8), dict(g_=p(gamma) + 4), dict(dh_=p(dh) + 8), dict(dg_=p(dg) + 4), dict(ws_=p(ws) + 8), dict(dy_=None), dict(h_=None),
               dict(g_=None), dict(dh_=None), dict(dg_=None)):
        assert bwd(**kw) == EINVAL, kw
    for bad in (2, -1):
        assert fwd(opf=bad) == EUNSUPPORTED and bwd(opf=bad) == EUNSUPPORTED
    assert bwd(n_=n - 1) == EWORKSPACE and bwd(n_=0) == EWORKSPACE and bwd(ws_=None) == EWORKSPACE
    need = C.c_size_t(0)
    assert be.lib.vdk_ls_residual_bwd_workspace_bytes(rows, 12, C.byref(need)) == EINVAL and be.lib.vdk_ls_residual_bwd_workspace_bytes(0, Cc, C.byref(need)) == EINVAL
    assert be.lib.vdk_ls_residual_bwd_workspace_bytes(rows, Cc, None) == EINVAL
    _sync(be)
