"""Autograd nodes over the library's kernels that are not specific to one model: LayerNorm, Linear and MLP on the 16-bit MFMA GEMM (bias / GELU / residual epilogues, weight
gradients in the TN form), the average pool, the relative-position bias gather and the fp32 Linear of a pooled head.  `dt` is the operand format (torch.bfloat16 |
torch.float16) of the caller; swin.SwinTransformerAutograd, swinv2.SwinTransformerV2 and vit.VisionTransformerMap are built from them."""
from __future__ import annotations

import torch

from . import ops
from ._abi import ACT_DGELU, ACT_GELU


def _wgrad(be, dyb: torch.Tensor, xb: torch.Tensor) -> torch.Tensor:
    """dW f32 [N, K] = dY^T X for 16-bit dY [T, N], X [T, K]: the TN GEMM straight from both tensors when T % 64 == 0, else through zero-padded transposes"""
    T, Nn = dyb.shape
    K = xb.shape[1]
    if T % 64 == 0 and Nn % 8 == 0 and K % 8 == 0:
        tiles = ((Nn + 255) // 256) * ((K + 255) // 256)
        sk = max(1, min(256 // tiles, (T // 64) // 4, 64))
        return ops.gemm_nt(dyb, xb, out_dtype=torch.float32, trans=True, splitk=sk, backend=be)
    dyt = ops.transpose_pad(dyb, backend=be)                    # [N, Tp]
    xt = ops.transpose_pad(xb, backend=be)                      # [K, Tp]
    return ops.gemm_nt(dyt, xt, out_dtype=torch.float32, backend=be)


def _cast(be, t: torch.Tensor, dt) -> torch.Tensor:
    return t if t.dtype == dt else ops.cast_16(t.contiguous(), dt, backend=be)


def _wt(be, w: torch.Tensor, dt) -> torch.Tensor:
    """w f32 [out, in] -> dt [in, out]: the B operand of dX = dY W"""
    if dt == torch.bfloat16:
        wt = ops.transpose_cast(w.detach().contiguous(), backend=be)          # (columns padded to a multiple of 8)
        return wt[:, :w.shape[0]] if wt.shape[1] != w.shape[0] else wt
    return ops.transpose_pad(ops.cast_16(w.detach().contiguous(), dt, backend=be), rpad=w.shape[0], backend=be)


def _colsum(be, dyb: torch.Tensor) -> torch.Tensor:
    """f32 column sums of a 16-bit [T, N] gradient (a Linear's bias gradient).  fp16: dY^T 1 on the MFMA GEMM, an fp32 sum of the stored values like vdk_colsum_bf16's"""
    if dyb.dtype == torch.bfloat16:
        return ops.colsum_bf16(dyb, backend=be)
    ones = torch.ones((dyb.shape[0], 8), dtype=dyb.dtype, device=dyb.device)
    return _wgrad(be, dyb, ones)[:, 0].contiguous()


def _grad_bf16(be, dy: torch.Tensor, rows: int, dt) -> torch.Tensor:
    """the 16-bit [rows, C] operand of a gradient: the copy its producer attached (_LNRes.backward), else a cast"""
    c = getattr(dy, "_vdk_bf16", None)
    # the attached copy is trusted only if it is in the operand format asked for and the gradient is still the producer's tensor, untouched: an in-place accumulation (a
    # second consumer of the activation, a tensor hook) bumps _version, a re-materialised sum has another data pointer -- then the copy is stale and the gradient is cast again
    if c is not None and c[0].dtype == dt and c[0].numel() == dy.numel() and c[1] == dy._version and c[2] == dy.data_ptr():
        return c[0].view(rows, -1)
    return _cast(be, dy.contiguous().view(rows, -1), dt)


class _LN(torch.autograd.Function):
    """LayerNorm over the last dimension of f32 rows -> the operand format (a GEMM operand) or f32 (the residual stream)"""

    @staticmethod
    def forward(ctx, x, w, b, eps, out_dtype, be):
        x2 = x.contiguous().view(-1, w.numel())
        y, mean, rstd = ops.layernorm_fwd(x2, w.detach(), b.detach(), eps, out_dtype, backend=be)
        ctx.save_for_backward(x2, mean, rstd, w)
        ctx.be, ctx.shape = be, x.shape
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, mean, rstd, w = ctx.saved_tensors
        dy2 = dy.contiguous().view(x2.shape)
        dx, _, dg, db = ops.layernorm_bwd(dy2, x2, mean, rstd, w.detach(), want_bf16=False, backend=ctx.be)
        return dx.view(ctx.shape), dg, db, None, None, None


class _LNRes(torch.autograd.Function):
    """(LayerNorm(x) in the operand format, x): a block's pre-norm with the shortcut routed through the same node, so that the backward adds the shortcut's gradient inside
    the LayerNorm backward kernel (its `dres` input) instead of an autograd accumulation pass over the f32 stream.  The f32 dx carries its 16-bit copy (written by the same
    kernel) as `_vdk_bf16`: the next consumer is a GEMM and takes it instead of casting (see _grad_bf16)."""

    @staticmethod
    def forward(ctx, x, w, b, eps, dt, be):
        x2 = x.contiguous().view(-1, w.numel())
        y, mean, rstd = ops.layernorm_fwd(x2, w.detach(), b.detach(), eps, dt, backend=be)
        ctx.save_for_backward(x2, mean, rstd, w)
        ctx.be, ctx.shape = be, x.shape
        return y.view(x.shape), x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dres):
        x2, mean, rstd, w = ctx.saved_tensors
        dy2 = dy.contiguous().view(x2.shape)
        dr = dres.contiguous().view(x2.shape) if dres is not None else None
        dx, dxb, dg, db = ops.layernorm_bwd(dy2, x2, mean, rstd, w.detach(), dres=dr, want_bf16=True, backend=ctx.be)
        dx = dx.view(ctx.shape)
        dx._vdk_bf16 = (dxb, dx._version, dx.data_ptr())      # valid only while this very tensor reaches the consumer unmodified (see _grad_bf16)
        return dx, dg, db, None, None, None


class _Lin(torch.autograd.Function):
    """y = x W^T (+ b) (+ residual): 16-bit operands on the MFMA GEMM; y in the operand format, or f32 (when it joins the residual stream)"""

    @staticmethod
    def forward(ctx, x, w, b, residual, out_dtype, dt, be):
        xb = _cast(be, x.contiguous().view(-1, x.shape[-1]), dt)
        wb = ops.cast_16(w.detach().contiguous(), dt, backend=be)
        res = residual.contiguous().view(-1, w.shape[0]) if residual is not None else None
        y = ops.gemm_nt(xb, wb, out_dtype=out_dtype, bias=b.detach().contiguous() if b is not None else None, residual=res, backend=be)
        ctx.save_for_backward(xb, w)
        ctx.be, ctx.dt, ctx.has_b, ctx.has_r, ctx.xshape, ctx.xdtype = be, dt, b is not None, residual is not None, x.shape, x.dtype
        return y.view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        xb, w = ctx.saved_tensors
        be, dt = ctx.be, ctx.dt
        dyb = _grad_bf16(be, dy, dy.numel() // w.shape[0], dt)
        dx = ops.gemm_nt(dyb, _wt(be, w, dt), out_dtype=dt if ctx.xdtype == dt else torch.float32, backend=be)
        dw = _wgrad(be, dyb, xb)
        db = _colsum(be, dyb) if ctx.has_b else None
        return dx.view(ctx.xshape), dw, db, dy if ctx.has_r else None, None, None, None


class _Mlp(torch.autograd.Function):
    """fc2(gelu(fc1(x))) (+ residual): fc1 with the GELU epilogue (pre-activation kept), fc2 in the operand format or, with the residual epilogue, f32; backward with the
    dGELU epilogue on the fc2 input-gradient GEMM"""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, residual, dt, be):
        xb = _cast(be, x.contiguous().view(-1, x.shape[-1]), dt)
        w1b, w2b = ops.cast_16(w1.detach().contiguous(), dt, backend=be), ops.cast_16(w2.detach().contiguous(), dt, backend=be)
        u = torch.empty((xb.shape[0], w1.shape[0]), dtype=dt, device=x.device)
        g = ops.gemm_nt(xb, w1b, bias=b1.detach(), act=ACT_GELU, aux=u, backend=be)
        if residual is not None:
            y = ops.gemm_nt(g, w2b, out_dtype=torch.float32, bias=b2.detach(), residual=residual.contiguous().view(-1, w2.shape[0]), backend=be)
        else:
            y = ops.gemm_nt(g, w2b, bias=b2.detach(), backend=be)
        ctx.save_for_backward(xb, u, g, w1, w2)
        ctx.be, ctx.dt, ctx.has_r, ctx.xshape, ctx.xdtype = be, dt, residual is not None, x.shape, x.dtype
        return y.view(*x.shape[:-1], w2.shape[0])

    @staticmethod
    def backward(ctx, dy):
        xb, u, g, w1, w2 = ctx.saved_tensors
        be, dt = ctx.be, ctx.dt
        dyb = _grad_bf16(be, dy, dy.numel() // w2.shape[0], dt)
        du = ops.gemm_nt(dyb, _wt(be, w2, dt), act=ACT_DGELU, aux=u, backend=be)
        dw2, db2 = _wgrad(be, dyb, g), _colsum(be, dyb)
        dx = ops.gemm_nt(du, _wt(be, w1, dt), out_dtype=dt if ctx.xdtype == dt else torch.float32, backend=be)
        dw1, db1 = _wgrad(be, du, xb), _colsum(be, du)
        return dx.view(ctx.xshape), dw1, db1, dw2, db2, dy if ctx.has_r else None, None, None


class _BiasGather(torch.autograd.Function):
    """a per-head table [(2 ws - 1)^2, H] -> bias [H, N, N] through index [N, N] (an index gather); the backward sums each table entry's <= N uses in a fixed order with one
    gather kernel (timm's index backward is an index_add with atomics).  uses [(2 ws - 1)^2, N]: where each table entry is used (see swin._uses_table)"""

    @staticmethod
    def forward(ctx, table, index, uses, be):
        n = index.shape[0]
        ctx.be, ctx.uses, ctx.shape, ctx.n = be, uses, table.shape, n
        return table.detach()[index.view(-1)].view(n, n, -1).permute(2, 0, 1).contiguous()

    @staticmethod
    def backward(ctx, dbias):
        be, uses = ctx.be, ctx.uses
        R, H = ctx.shape
        dbias = dbias.contiguous()
        dtable = torch.empty((R, H), dtype=torch.float32, device=dbias.device)
        be.check(be.lib.vdk_relpos_bias_table_grad(be.ptr(dbias), be.ptr(uses), R, uses.shape[1], H, ctx.n * ctx.n, be.ptr(dtable), be.stream()), "vdk_relpos_bias_table_grad")
        return dtable, None, None, None


class _Pool(torch.autograd.Function):
    """global average pool over the tokens of f32 NHWC rows"""

    @staticmethod
    def forward(ctx, x, be):
        B, H, W, Cc = x.shape
        out = torch.empty((B, Cc), dtype=torch.float32, device=x.device)
        be.check(be.lib.vdk_avgpool_rows_f32_fwd(be.ptr(x.contiguous()), be.ptr(out), B, H * W, Cc, be.stream()), "vdk_avgpool_rows_f32_fwd")
        ctx.be, ctx.shape = be, x.shape
        return out

    @staticmethod
    def backward(ctx, dy):
        B, H, W, Cc = ctx.shape
        dx = torch.empty(ctx.shape, dtype=torch.float32, device=dy.device)
        ctx.be.check(ctx.be.lib.vdk_avgpool_rows_f32_bwd(ctx.be.ptr(dy.contiguous()), ctx.be.ptr(dx), None, B, H * W, Cc, ctx.be.stream()), "vdk_avgpool_rows_f32_bwd")
        return dx, None


def _pad4(t: torch.Tensor) -> torch.Tensor:
    """zero-pad the contraction (last) dim to a multiple of 4 (16-byte rows for the fp32 GEMM)"""
    k = t.shape[-1]
    return t.contiguous() if k % 4 == 0 else torch.nn.functional.pad(t, (0, 4 - k % 4)).contiguous()


def _wgrad_f32(dy: torch.Tensor, x: torch.Tensor, be) -> torch.Tensor:
    """dW [out, in] = dy^T x for [rows, out] / [rows, in] fp32 operands with few rows (the pooled [B, D] tail): fp32 MFMA GEMM over the transposed operands"""
    return ops.gemm_f32(_pad4(dy.t()), _pad4(x.t()), backend=be)


class _LinearFn(torch.autograd.Function):
    """y = x W^T + b on the fp32 MFMA GEMM (the classifier head on pooled [B, D] rows)"""

    @staticmethod
    def forward(ctx, x, w, b, be):
        ctx.save_for_backward(x, w); ctx.be = be
        return ops.gemm_f32(x.contiguous(), w.detach(), bias=b.detach(), backend=be)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        Cn = dy.shape[1]
        if Cn % 4:      # class counts that are not multiples of 4: zero columns / rows keep the contraction 16-byte aligned
            dx = ops.gemm_f32(_pad4(dy), torch.nn.functional.pad(w.detach(), (0, 0, 0, 4 - Cn % 4)).contiguous(), b_kmajor=True, backend=ctx.be)
        else:
            dx = ops.gemm_f32(dy, w.detach(), b_kmajor=True, backend=ctx.be)
        return dx, _wgrad_f32(dy, x, ctx.be), dy.sum(0), None
