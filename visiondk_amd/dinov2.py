"""DINOv2 ViT-S/B/L/14 (timm `vit_{small,base,large}_patch14_dinov2`) on the HIP kernels: the family the reference's configs list as a drop-in backbone
(`timm-vit_large_patch14_dinov2.lvd142m # imgsz 518`).  Autograd-node form, modelled on `swinv2.SwinTransformerV2`: a torch Module with timm's state_dict names whose
arithmetic runs in autograd nodes over the library's kernels.  What the family adds to a plain ViT is LayerScale on the residual stream -- x = x + ls1(attn(norm1 x)),
x = x + ls2(mlp(norm2 x)), ls(h) = h * gamma, gamma [dim] initialised to 1e-5 -- served by csrc/layerscale_residual.hip.  A LayerScale mode of the native `vdk_vit_*` engine
(and with it FusedTrainStep / FaceTrainStep / forward_precise) is the follow-up; this module trains under a plain torch optimizer (with a loss scale for fp16 operands).

timm 0.9.16 semantics as restated here (vision_transformer.py; pinned against transformers.Dinov2Model through tests/dinov2_ref.py, tests/test_dinov2_ref.py):
  * patch_embed.proj = Conv 14 x 14 stride 14 with bias; tokens = flatten(2).transpose(1, 2).
  * x = cat(cls_token.expand(B), tokens); x = x + pos_embed [1, 1 + (S / 14)^2, D] (class token first, then the add; no register tokens in these three ids).
  * depth x Block (pre-norm): x = x + ls1(attn(norm1(x))); x = x + ls2(mlp(norm2(x))).  LayerNorm eps 1e-6, qkv_bias, softmax(q k^T / sqrt(hd)) v, exact-erf GELU,
    ls.gamma [D] with init_values = 1e-5.
  * norm on every token; global_pool = 'token' takes token 0, no fc_norm, head = Linear(D, classes).  num_classes = 0 with global_pool = '' returns the normed tokens [B, N, D].
  * init: timm's (trunc_normal 0.02 pos_embed, normal 1e-6 cls_token, gamma 1e-5), then the reference's override (classify_model.py:70-81): N(0, 0.02) for every Conv /
    Linear weight, zero Linear biases; gamma stays 1e-5.
Not served: `vit_giant_patch14_dinov2` (SwiGLU MLP) and the `_reg4_` ids (register tokens): KeyError with the served list.

Arithmetic: `operand` "bf16" | "fp16" is the format of every GEMM and attention operand; residual stream and master weights fp32.  A block is built from _nodes.py: _LNRes (the
pre-norm with the shortcut routed through it), _Lin (qkv, proj; 16-bit outputs as under the reference's autocast), _Attn (ops.attention_fwd / attention_bwd), _Mlp, and _LSRes:
the branch's last GEMM output h stays in the operand format, `h * gamma` promotes to fp32 and the add is fp32 (vdk_ls_residual_fwd); the backward rounds gamma * dy once
into the gradient of h and sums dgamma = sum_rows dy * h in fp32 in a fixed order (vdk_ls_residual_bwd); the shortcut's gradient is dy itself, no copy.  Each _LSRes saves h:
T * D * 2 bytes, two per block.  The patch rows come from ops.patchify (K = 588 padded to 592: 16-byte rows); the class-token cat and the pos_embed add are torch ops on the
device; the head runs on the fp32 GEMM (_LinearFn)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn

from . import _lib, ops
from ._engine import OPERANDS, _Holder, check_image
from ._nodes import _LinearFn, _Lin, _LN, _LNRes, _Mlp

_OPF = {torch.bfloat16: 0, torch.float16: 1}

NEEDS_ENGINE = ("{what} needs a native engine; the DINOv2 ViTs (vit_*_patch14_dinov2) are served as autograd nodes over the kernels and train under a plain torch optimizer "
                "over model.parameters() (with a loss scale for fp16 operands).  The LayerScale mode of the native vdk_vit_* engine and its fused train step are a follow-up.")


@dataclass(frozen=True)
class Dinov2Spec:
    img_size: int = 518
    patch_size: int = 14
    in_chans: int = 3
    num_classes: int = 1000
    dim: int = 1024
    depth: int = 24
    heads: int = 16
    mlp_dim: int = 4096
    ln_eps: float = 1e-6
    init_values: float = 1e-5
    global_pool: str = "token"      # 'token' (the family's default) | '' (with num_classes = 0: the normed tokens)


TIMM_DINOV2S = {
    "vit_small_patch14_dinov2": dict(dim=384, depth=12, heads=6, mlp_dim=1536),
    "vit_base_patch14_dinov2": dict(dim=768, depth=12, heads=12, mlp_dim=3072),
    "vit_large_patch14_dinov2": dict(dim=1024, depth=24, heads=16, mlp_dim=4096),
}


# ---- the two nodes of this family (the model-independent ones: _nodes.py) -----------------------------------------------------------------------------
class _Attn(torch.autograd.Function):
    """softmax(q k^T / sqrt(hd)) v on 16-bit qkv rows [B, N, 3 D] -> o [B, N, D] (ops.attention_fwd / attention_bwd: the streaming kernels above 256 tokens)"""

    @staticmethod
    def forward(ctx, qkv, heads, be):
        qkv = qkv.contiguous()
        o, lse = ops.attention_fwd(qkv, heads, backend=be)
        ctx.save_for_backward(qkv, o, lse)
        ctx.heads, ctx.be = heads, be
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse = ctx.saved_tensors
        return ops.attention_bwd(qkv, o, do.contiguous(), lse, ctx.heads, backend=ctx.be), None, None


class _LSRes(torch.autograd.Function):
    """x + gamma * h: x f32 [..., C] (the residual stream), h in the operand format (the branch's last GEMM output, saved), gamma f32 [C] -> f32.  Backward: the shortcut gets
    dy itself, h gets RNE16(gamma * dy), gamma gets sum_rows dy * h (csrc/layerscale_residual.hip)."""

    @staticmethod
    def forward(ctx, x, h, gamma, be):
        Cc = gamma.numel()
        x2, h2, g = x.contiguous().view(-1, Cc), h.contiguous().view(-1, Cc), gamma.detach().contiguous()
        y = torch.empty_like(x2)
        be.check(be.lib.vdk_ls_residual_fwd(be.ptr(x2), Cc, be.ptr(h2), Cc, be.ptr(g), be.ptr(y), Cc, x2.shape[0], Cc, _OPF[h2.dtype], be.stream()), "vdk_ls_residual_fwd")
        ctx.save_for_backward(h2, gamma)
        ctx.be, ctx.shape = be, x.shape
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        h2, gamma = ctx.saved_tensors
        be = ctx.be
        T, Cc = h2.shape
        dy2, g = dy.contiguous().view(T, Cc), gamma.detach().contiguous()
        dh = torch.empty_like(h2)
        dg = torch.empty(Cc, dtype=torch.float32, device=h2.device)
        ws, n = ops._ws(be, be.lib.vdk_ls_residual_bwd_workspace_bytes, T, Cc, device=h2.device)
        be.check(be.lib.vdk_ls_residual_bwd(be.ptr(dy2), Cc, be.ptr(h2), Cc, be.ptr(g), be.ptr(dh), Cc, be.ptr(dg), T, Cc, _OPF[h2.dtype], be.ptr(ws), n, be.stream()),
                 "vdk_ls_residual_bwd")
        return dy, dh.view(ctx.shape), dg.view(gamma.shape), None


# ---- modules with timm's names -------------------------------------------------------------------------------------------------------------------------
class LayerScale(nn.Module):
    def __init__(self, dim: int, init_values: float, dev):
        super().__init__()
        self.gamma = nn.Parameter(init_values * torch.ones(dim, device=dev))


class Attention(nn.Module):
    def __init__(self, dim: int, dev):
        super().__init__()
        self.qkv = nn.Linear(dim, 3 * dim, bias=True, device=dev)
        self.proj = nn.Linear(dim, dim, device=dev)


class Mlp(nn.Module):
    def __init__(self, dim: int, hidden: int, dev):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden, device=dev)
        self.fc2 = nn.Linear(hidden, dim, device=dev)


class Block(nn.Module):
    def __init__(self, spec: Dinov2Spec, be, dt, dev):
        super().__init__()
        self.heads, self.eps, self.be, self.dt = spec.heads, spec.ln_eps, be, dt
        self.norm1 = nn.LayerNorm(spec.dim, eps=spec.ln_eps, device=dev)
        self.attn = Attention(spec.dim, dev)
        self.ls1 = LayerScale(spec.dim, spec.init_values, dev)
        self.norm2 = nn.LayerNorm(spec.dim, eps=spec.ln_eps, device=dev)
        self.mlp = Mlp(spec.dim, spec.mlp_dim, dev)
        self.ls2 = LayerScale(spec.dim, spec.init_values, dev)

    def forward(self, x):
        """the block on the f32 tokens [B, N, D]; each branch leaves its last GEMM in the operand format, as under the reference's autocast, and _LSRes widens it"""
        be, dt, a, m = self.be, self.dt, self.attn, self.mlp
        y, x = _LNRes.apply(x, self.norm1.weight, self.norm1.bias, self.eps, dt, be)
        o = _Attn.apply(_Lin.apply(y, a.qkv.weight, a.qkv.bias, None, dt, dt, be), self.heads, be)
        x = _LSRes.apply(x, _Lin.apply(o, a.proj.weight, a.proj.bias, None, dt, dt, be), self.ls1.gamma, be)
        y, x = _LNRes.apply(x, self.norm2.weight, self.norm2.bias, self.eps, dt, be)
        return _LSRes.apply(x, _Mlp.apply(y, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, None, dt, be), self.ls2.gamma, be)


class DinoVisionTransformer(nn.Module):
    """timm.create_model('vit_*_patch14_dinov2', num_classes=C, img_size=S) as autograd nodes over the kernels: forward(x [B, 3, S, S]) -> logits [B, C]; num_classes = 0:
    the normed class token [B, D] (global_pool 'token') or the normed tokens [B, 1 + (S / 14)^2, D] (global_pool '', what TimmWrapper asks for)."""

    def __init__(self, spec: Dinov2Spec, device=None, backend: Optional[_lib.Backend] = None, seed: Optional[int] = None, operand: str = "bf16"):
        super().__init__()
        if operand not in OPERANDS:
            raise ValueError(f"operand must be 'bf16' or 'fp16', got {operand!r}")
        if spec.img_size % spec.patch_size:
            raise ValueError(f"img_size must be a multiple of the patch size {spec.patch_size} (the stem does not crop a border)")
        if spec.dim % spec.heads or spec.dim // spec.heads not in (64, 80):
            raise ValueError("the attention kernels are built for head dims 64 and 80 (every served DINOv2 id has 64)")
        if spec.dim % 8 or spec.mlp_dim % 8:
            raise ValueError("dim and mlp_dim must be multiples of 8 (16-byte rows of 16-bit operands)")
        if spec.global_pool not in ("token", ""):
            raise ValueError("global_pool: 'token' (the family's default) or '' (the normed tokens, with num_classes=0)")
        self.spec, self.operand = spec, operand
        self.be = backend or _lib.load()
        dt = self.dt = OPERANDS[operand]
        dev = device if device is not None else ("cuda" if self.be.device_only else "cpu")
        if seed is not None:
            torch.manual_seed(seed)
        self.num_classes, self.num_features = spec.num_classes, spec.dim
        self.tokens = (spec.img_size // spec.patch_size) ** 2 + 1
        self.cls_token = nn.Parameter(torch.zeros(1, 1, spec.dim, device=dev))
        self.pos_embed = nn.Parameter(torch.zeros(1, self.tokens, spec.dim, device=dev))
        self.patch_embed = _Holder()
        self.patch_embed.proj = nn.Conv2d(spec.in_chans, spec.dim, spec.patch_size, spec.patch_size, device=dev)
        self.blocks = nn.Sequential(*[Block(spec, self.be, dt, dev) for _ in range(spec.depth)])
        self.norm = nn.LayerNorm(spec.dim, eps=spec.ln_eps, device=dev)
        self.head = nn.Linear(spec.dim, spec.num_classes, device=dev) if spec.num_classes > 0 else nn.Identity()
        self.reset_parameters()

    def reset_parameters(self):
        """timm's init (trunc_normal 0.02 pos_embed, normal 1e-6 cls_token, gamma = init_values, LayerNorm 1 / 0), then the reference's override (classify_model.py:70-81):
        N(0, 0.02) for every Conv2d / Linear weight, zeros for Linear biases; gamma stays at init_values"""
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        nn.init.normal_(self.cls_token, std=1e-6)
        for blk in self.blocks:
            for ls in (blk.ls1, blk.ls2):
                nn.init.constant_(ls.gamma, self.spec.init_values)
            for nrm in (blk.norm1, blk.norm2):
                nrm.reset_parameters()
        self.norm.reset_parameters()
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, mean=0, std=0.02)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, mean=0, std=0.02)
                nn.init.zeros_(m.bias)

    def _patch_rows(self, x: torch.Tensor) -> torch.Tensor:
        """[B, 3, S, S] -> the (c, ky, kx) patch rows [B (S / 14)^2, Kp], K = 588 zero-padded to Kp = 592; bf16 straight from the patchify kernel, fp16 through its f32 form"""
        s, be = self.spec, self.be
        B = x.shape[0]
        if self.dt == torch.bfloat16:
            return ops.patchify(x, s.patch_size, backend=be)
        K = s.in_chans * s.patch_size ** 2
        rows = B * (s.img_size // s.patch_size) ** 2
        pf = torch.empty((rows, K), dtype=torch.float32, device=x.device)
        be.check(be.lib.vdk_patchify_f32(be.ptr(x), B, s.in_chans, s.img_size, s.img_size, s.patch_size, be.ptr(pf), be.stream()), "vdk_patchify_f32")
        return ops.cast_16(torch.nn.functional.pad(pf, (0, -K % 8)), self.dt, backend=be)

    def forward_tokens(self, x: torch.Tensor) -> torch.Tensor:
        """the f32 residual stream [B, N, D] behind the last block (before `norm`)"""
        s, be, dt = self.spec, self.be, self.dt
        check_image(x, s.in_chans, s.img_size)
        B = x.shape[0]
        w = self.patch_embed.proj.weight.view(s.dim, -1)
        w = torch.nn.functional.pad(w, (0, -w.shape[1] % 8))
        tok = _Lin.apply(self._patch_rows(x.contiguous()), w, self.patch_embed.proj.bias, None, dt, dt, be).float().view(B, self.tokens - 1, s.dim)
        t = torch.cat((self.cls_token.expand(B, -1, -1), tok), dim=1) + self.pos_embed
        return self.blocks(t)

    def forward_features(self, x: torch.Tensor) -> torch.Tensor:
        return _LN.apply(self.forward_tokens(x), self.norm.weight, self.norm.bias, self.spec.ln_eps, torch.float32, self.be)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.spec.global_pool == "":
            return self.forward_features(x)
        # LayerNorm is per token: norm(x)[:, 0] == norm(x[:, 0]); only the class-token rows are normalised
        f = _LN.apply(self.forward_tokens(x)[:, 0], self.norm.weight, self.norm.bias, self.spec.ln_eps, torch.float32, self.be)
        if self.num_classes == 0:
            return f
        return _LinearFn.apply(f, self.head.weight, self.head.bias, self.be)


def create_model(name: str, pretrained: bool = False, num_classes: int = 1000, img_size: int = 518, device=None, backend=None, seed: Optional[int] = None,
                 operand: str = "bf16", drop_path_rate: float = 0.0, global_pool: Optional[str] = None, **kwargs) -> DinoVisionTransformer:
    """timm.create_model for the served DINOv2 ids (a `timm-` prefix and a `.tag` suffix are accepted).  `vit_giant_patch14_dinov2` (SwiGLU) and the `_reg4_` ids (register
    tokens) are not served: KeyError with the served list."""
    if kwargs:
        raise TypeError(f"dinov2.create_model: unsupported keyword arguments {sorted(kwargs)} (timm would act on them; this module does not build them)")
    arch = name[5:] if name.startswith("timm-") else name
    arch = arch.split(".")[0]
    if arch not in TIMM_DINOV2S:
        raise KeyError(f"'{name}': served DINOv2 ids are {sorted(TIMM_DINOV2S)} (LayerScale ViT-S/B/L/14, head dim 64); the giant id (SwiGLU) and the reg4 ids (register tokens) "
                       "are not built")
    if pretrained:
        raise RuntimeError("no network access: load a checkpoint with load_state_dict (timm's state_dict names)")
    if drop_path_rate != 0.0:
        raise NotImplementedError("drop_path_rate != 0 is not built for the DINOv2 ids (timm's default for the family is 0)")
    if img_size % 14:
        raise ValueError("the patch-14 family needs img_size % 14 == 0 (518 by default; the stem does not crop a border)")
    if global_pool not in (None, "token") and not (global_pool == "" and num_classes == 0):
        raise ValueError("global_pool: 'token' (the family's default) or '' together with num_classes=0 (the normed tokens [B, N, D])")
    spec = Dinov2Spec(img_size=img_size, num_classes=num_classes, global_pool="token" if global_pool is None else global_pool, **TIMM_DINOV2S[arch])
    return DinoVisionTransformer(spec, device=device, backend=backend, seed=seed, operand=operand)
