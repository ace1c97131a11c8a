"""BEiT / BEiT-v2 base and large at patch 16, 224 pixels (timm `beit_{base,large}_patch16_224`, `beitv2_{base,large}_patch16_224`) on the HIP kernels: the first id of the
`timm.list_models(pretrained=True)` examples in both of the reference's model READMEs (`beit_base_patch16_224.in22k_ft_in22k`).  Autograd-node form, modelled on
`dinov2.DinoVisionTransformer` and `swinv2.SwinTransformerV2`: a torch Module with timm's state_dict names whose arithmetic runs in autograd nodes over the library's kernels.
What the family adds to a LayerScale ViT is the relative position bias inside the attention over the whole 197-token sequence, served by csrc/attention_bias.hip
(vdk_attention_bias_fwd / vdk_attention_bias_bwd: softmax(scale q k^T + bias[h]) v with d(bias) in the backward, N <= 256, head dim 64).  A LayerScale + bias mode of the
native `vdk_vit_*` engine (and with it FusedTrainStep / FaceTrainStep / forward_precise) is the follow-up; this module trains under a plain torch optimizer (with a loss
scale for fp16 operands).

timm 0.9.16 `beit.py` semantics as restated here -- from knowledge of the pinned version, pinned against transformers.BeitModel through tests/beit_ref.py and
tests/test_beit_ref.py:
  * patch_embed.proj = Conv 16 x 16 stride 16 with bias; cls_token is prepended; there is NO absolute position embedding.
  * Block (LayerNorm eps 1e-6): x = x + gamma_1 * attn(norm1(x)); x = x + gamma_2 * mlp(norm2(x)); gamma_1, gamma_2 are parameters [dim] directly on the block, initialised
    to 0.1 (beit base / large) or 1e-5 (the beitv2 ids); MLP ratio 4, exact-erf GELU.
  * attn.qkv = Linear(C -> 3 C) without a bias parameter; the bias used is cat(q_bias, zeros, v_bias); q_bias and v_bias are parameters, k_bias a non-persistent zero
    buffer; attn.proj carries a bias; scale = 64^-0.5.
  * attn.relative_position_bias_table [(2 G - 1)^2 + 3, H] per block (G = grid edge, 14), zero at init; relative_position_index is a non-persistent buffer [N, N],
    N = G^2 + 1: patch to patch (dy + G - 1)(2 G - 1) + (dx + G - 1); row 0 (class query) = R - 3, column 0 (class key) = R - 2, entry (0, 0) = R - 1, R the table length;
    bias = table[index].view(N, N, H).permute(2, 0, 1).
  * head with global_pool = 'avg' (the default): `norm` is Identity, the mean of the PATCH tokens (class token excluded) goes through fc_norm, then head.  With
    num_classes = 0 and global_pool = '' (what TimmWrapper asks for): `norm` is a LayerNorm over all N tokens and the tokens [B, N, C] are returned; the state_dict then has
    norm.* and no fc_norm.*.
  * init: timm's (trunc_normal 0.02 cls_token, zero tables, gammas = init_values), then the reference's override: N(0, 0.02) for every Conv / Linear weight, zero Linear
    biases; gamma_*, q_bias, v_bias, the tables, cls_token and the LayerNorms are left alone.
Not served: the 384 / 512 ids (577 / 1025 tokens: the bias in the streaming attention kernels is a follow-up) and the shared relative position bias (no timm id of this
family uses it): KeyError with the served list.

Arithmetic: `operand` "bf16" | "fp16" is the format of every GEMM and attention operand; residual stream and master weights fp32.  A block is built from _nodes.py (_LNRes,
_Lin, _Mlp, _BiasGather), dinov2._LSRes (x + gamma * h with h kept in the operand format; vdk_ls_residual_fwd / _bwd) and _AttnBias below; the table gradient is
vdk_relpos_bias_table_grad on the kernel's d(bias).  The class-token cat, the patch-token mean and fc_norm's input are torch ops on the device; the head runs on the fp32 GEMM."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn

from . import _lib, ops
from ._abi import F16_
from ._engine import OPERANDS, _Holder, check_image
from ._nodes import _BiasGather, _LinearFn, _Lin, _LN, _LNRes, _Mlp
from .dinov2 import _LSRes

_DT = {torch.bfloat16: 0, torch.float16: F16_}      # VDK_BF16, VDK_F16

NEEDS_ENGINE = ("{what} needs a native engine; the BEiT models (beit_* / beitv2_*_patch16_224) are served as autograd nodes over the kernels and train under a plain torch "
                "optimizer over model.parameters() (with a loss scale for fp16 operands).  The LayerScale + bias mode of the native vdk_vit_* engine and its fused train step "
                "are a follow-up.")


@dataclass(frozen=True)
class BeitSpec:
    img_size: int = 224
    patch_size: int = 16
    in_chans: int = 3
    num_classes: int = 1000
    dim: int = 768
    depth: int = 12
    heads: int = 12
    ln_eps: float = 1e-6
    init_values: float = 0.1
    global_pool: str = "avg"        # 'avg' (the family's default) | '' (with num_classes = 0: the normed tokens)


TIMM_BEITS = {
    "beit_base_patch16_224": dict(dim=768, depth=12, heads=12, init_values=0.1),
    "beit_large_patch16_224": dict(dim=1024, depth=24, heads=16, init_values=0.1),
    "beitv2_base_patch16_224": dict(dim=768, depth=12, heads=12, init_values=1e-5),
    "beitv2_large_patch16_224": dict(dim=1024, depth=24, heads=16, init_values=1e-5),
}


def relative_position_index(G: int) -> torch.Tensor:
    """[N, N], N = G^2 + 1, into a table of R = (2 G - 1)^2 + 3 rows (see the module docstring)"""
    R = (2 * G - 1) ** 2 + 3
    coords = torch.stack(torch.meshgrid(torch.arange(G), torch.arange(G), indexing="ij")).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += G - 1
    rel[:, :, 1] += G - 1
    rel[:, :, 0] *= 2 * G - 1
    idx = torch.zeros(G * G + 1, G * G + 1, dtype=torch.long)
    idx[1:, 1:] = rel.sum(-1)
    idx[0, :] = R - 3
    idx[:, 0] = R - 2
    idx[0, 0] = R - 1
    return idx


def _uses_table(idx: torch.Tensor, R: int) -> torch.Tensor:
    """for the bias gather's backward: the positions q * N + k at which each of the R table entries is used, int32 [R, most uses of one entry] (-1 padded), ascending"""
    flat = idx.reshape(-1)
    order = torch.argsort(flat, stable=True)
    counts = torch.bincount(flat, minlength=R)
    uses = torch.full((R, int(counts.max())), -1, dtype=torch.int32)
    start = torch.cumsum(counts, 0) - counts
    rows = flat[order]
    uses[rows, torch.arange(flat.numel()) - start[rows]] = order.to(torch.int32)
    return uses


class _AttnBias(torch.autograd.Function):
    """softmax(q k^T / sqrt(64) + bias[h]) v on 16-bit qkv rows [B, N, 3 D] and an f32 bias [H, N, N] -> o [B, N, D] (csrc/attention_bias.hip); backward: dqkv and d(bias)"""

    @staticmethod
    def forward(ctx, qkv, bias, heads, be):
        qkv, bias = qkv.contiguous(), bias.detach().contiguous()
        B, N, D3 = qkv.shape
        D = D3 // 3
        hd = D // heads
        o = torch.empty((B, N, D), dtype=qkv.dtype, device=qkv.device)
        lse = torch.empty((B, heads, N), dtype=torch.float32, device=qkv.device)
        ws, n = ops._ws(be, be.lib.vdk_attention_bias_fwd_workspace_bytes, N, heads, device=qkv.device)
        be.check(be.lib.vdk_attention_bias_fwd(be.ptr(qkv), D3, be.ptr(o), D, be.ptr(lse), be.ptr(bias), B, N, heads, hd, hd ** -0.5, _DT[qkv.dtype], be.ptr(ws), n,
                                               be.stream()), "vdk_attention_bias_fwd")
        ctx.save_for_backward(qkv, o, lse, bias)
        ctx.heads, ctx.be = heads, be
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse, bias = ctx.saved_tensors
        be, heads = ctx.be, ctx.heads
        B, N, D3 = qkv.shape
        D = D3 // 3
        hd = D // heads
        do = do.contiguous()
        dqkv, dbias = torch.empty_like(qkv), torch.empty_like(bias)
        ws, n = ops._ws(be, be.lib.vdk_attention_bias_bwd_workspace_bytes, B, N, heads, device=qkv.device)
        be.check(be.lib.vdk_attention_bias_bwd(be.ptr(qkv), D3, be.ptr(o), be.ptr(do), D, be.ptr(lse), be.ptr(bias), be.ptr(dqkv), D3, be.ptr(dbias), B, N, heads, hd,
                                               hd ** -0.5, _DT[qkv.dtype], be.ptr(ws), n, be.stream()), "vdk_attention_bias_bwd")
        return dqkv, dbias, None, None


# ---- modules with timm's names -------------------------------------------------------------------------------------------------------------------------
class Attention(nn.Module):
    def __init__(self, dim: int, heads: int, grid: int, dev):
        super().__init__()
        R = (2 * grid - 1) ** 2 + 3
        self.qkv = nn.Linear(dim, 3 * dim, bias=False, device=dev)
        self.q_bias = nn.Parameter(torch.zeros(dim, device=dev))
        self.register_buffer("k_bias", torch.zeros(dim, device=dev), persistent=False)
        self.v_bias = nn.Parameter(torch.zeros(dim, device=dev))
        self.relative_position_bias_table = nn.Parameter(torch.zeros(R, heads, device=dev))
        idx = relative_position_index(grid)
        self.register_buffer("relative_position_index", idx.to(dev), persistent=False)
        self.register_buffer("_uses", _uses_table(idx, R).to(dev), persistent=False)
        self.proj = nn.Linear(dim, dim, device=dev)


class Mlp(nn.Module):
    def __init__(self, dim: int, hidden: int, dev):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden, device=dev)
        self.fc2 = nn.Linear(hidden, dim, device=dev)


class Block(nn.Module):
    def __init__(self, spec: BeitSpec, grid: int, be, dt, dev):
        super().__init__()
        self.heads, self.eps, self.be, self.dt = spec.heads, spec.ln_eps, be, dt
        self.norm1 = nn.LayerNorm(spec.dim, eps=spec.ln_eps, device=dev)
        self.attn = Attention(spec.dim, spec.heads, grid, dev)
        self.norm2 = nn.LayerNorm(spec.dim, eps=spec.ln_eps, device=dev)
        self.mlp = Mlp(spec.dim, 4 * spec.dim, dev)
        self.gamma_1 = nn.Parameter(spec.init_values * torch.ones(spec.dim, device=dev))
        self.gamma_2 = nn.Parameter(spec.init_values * torch.ones(spec.dim, device=dev))

    def forward(self, x):
        """the block on the f32 tokens [B, N, D]; each branch leaves its last GEMM in the operand format, as under the reference's autocast, and _LSRes widens it"""
        be, dt, a, m = self.be, self.dt, self.attn, self.mlp
        y, x = _LNRes.apply(x, self.norm1.weight, self.norm1.bias, self.eps, dt, be)
        qkv = _Lin.apply(y, a.qkv.weight, torch.cat((a.q_bias, a.k_bias, a.v_bias)), None, dt, dt, be)
        bias = _BiasGather.apply(a.relative_position_bias_table, a.relative_position_index, a._uses, be)
        o = _AttnBias.apply(qkv, bias, self.heads, be)
        x = _LSRes.apply(x, _Lin.apply(o, a.proj.weight, a.proj.bias, None, dt, dt, be), self.gamma_1, be)
        y, x = _LNRes.apply(x, self.norm2.weight, self.norm2.bias, self.eps, dt, be)
        return _LSRes.apply(x, _Mlp.apply(y, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, None, dt, be), self.gamma_2, be)


class Beit(nn.Module):
    """timm.create_model('beit_*_patch16_224', num_classes=C) as autograd nodes over the kernels: forward(x [B, 3, S, S]) -> logits [B, C]; num_classes = 0: the fc_norm'ed
    mean of the patch tokens [B, D] (global_pool 'avg') or the normed tokens [B, 1 + (S / 16)^2, D] (global_pool '', what TimmWrapper asks for)."""

    def __init__(self, spec: BeitSpec, device=None, backend: Optional[_lib.Backend] = None, seed: Optional[int] = None, operand: str = "bf16"):
        super().__init__()
        if operand not in OPERANDS:
            raise ValueError(f"operand must be 'bf16' or 'fp16', got {operand!r}")
        if spec.patch_size != 16 or spec.img_size % 16:
            raise ValueError("img_size must be a multiple of the patch size 16 (the stem does not crop a border)")
        grid = spec.img_size // 16
        if grid * grid + 1 > 256:
            raise ValueError(f"img_size {spec.img_size}: {grid * grid + 1} tokens; the biased attention kernels serve up to 256 (img_size <= 240)")
        if spec.dim % spec.heads or spec.dim // spec.heads != 64:
            raise ValueError("the biased attention kernels are built for head dim 64 (every served BEiT id has it)")
        if spec.global_pool not in ("avg", ""):
            raise ValueError("global_pool: 'avg' (the family's default) or '' (the normed tokens, with num_classes=0)")
        self.spec, self.operand = spec, operand
        self.be = backend or _lib.load()
        dt = self.dt = OPERANDS[operand]
        dev = device if device is not None else ("cuda" if self.be.device_only else "cpu")
        if seed is not None:
            torch.manual_seed(seed)
        self.num_classes, self.num_features = spec.num_classes, spec.dim
        self.tokens = grid * grid + 1
        self.cls_token = nn.Parameter(torch.zeros(1, 1, spec.dim, device=dev))
        self.patch_embed = _Holder()
        self.patch_embed.proj = nn.Conv2d(spec.in_chans, spec.dim, 16, 16, device=dev)
        self.blocks = nn.Sequential(*[Block(spec, grid, self.be, dt, dev) for _ in range(spec.depth)])
        if spec.global_pool == "avg":
            self.norm = nn.Identity()
            self.fc_norm = nn.LayerNorm(spec.dim, eps=spec.ln_eps, device=dev)
        else:
            self.norm = nn.LayerNorm(spec.dim, eps=spec.ln_eps, device=dev)
        self.head = nn.Linear(spec.dim, spec.num_classes, device=dev) if spec.num_classes > 0 else nn.Identity()
        nn.init.trunc_normal_(self.cls_token, std=0.02)
        self.reset_parameters()

    def reset_parameters(self):
        """the reference's override: N(0, 0.02) for every Conv2d / Linear weight, zeros for Linear biases.  gamma_*, q_bias, v_bias, the relative position tables, cls_token
        and the LayerNorms are left alone."""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, mean=0, std=0.02)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, mean=0, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def _patch_rows(self, x: torch.Tensor) -> torch.Tensor:
        """[B, 3, S, S] -> the (c, ky, kx) patch rows [B (S / 16)^2, 768]; bf16 straight from the patchify kernel, fp16 through its f32 form"""
        s, be = self.spec, self.be
        B = x.shape[0]
        if self.dt == torch.bfloat16:
            return ops.patchify(x, 16, backend=be)
        K = s.in_chans * 256
        pf = torch.empty((B * (self.tokens - 1), K), dtype=torch.float32, device=x.device)
        be.check(be.lib.vdk_patchify_f32(be.ptr(x), B, s.in_chans, s.img_size, s.img_size, 16, be.ptr(pf), be.stream()), "vdk_patchify_f32")
        return ops.cast_16(pf, self.dt, backend=be)

    def forward_tokens(self, x: torch.Tensor) -> torch.Tensor:
        """the f32 residual stream [B, N, D] behind the last block (before `norm`)"""
        s, be, dt = self.spec, self.be, self.dt
        check_image(x, s.in_chans, s.img_size)
        B = x.shape[0]
        w = self.patch_embed.proj.weight.view(s.dim, -1)
        tok = _Lin.apply(self._patch_rows(x.contiguous()), w, self.patch_embed.proj.bias, None, dt, dt, be).float().view(B, self.tokens - 1, s.dim)
        return self.blocks(torch.cat((self.cls_token.expand(B, -1, -1), tok), dim=1))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        s, be = self.spec, self.be
        t = self.forward_tokens(x)
        if s.global_pool == "":
            return _LN.apply(t, self.norm.weight, self.norm.bias, s.ln_eps, torch.float32, be)
        f = _LN.apply(t[:, 1:].mean(1), self.fc_norm.weight, self.fc_norm.bias, s.ln_eps, torch.float32, be)
        if self.num_classes == 0:
            return f
        return _LinearFn.apply(f, self.head.weight, self.head.bias, be)


def create_model(name: str, pretrained: bool = False, num_classes: int = 1000, img_size: int = 224, device=None, backend=None, seed: Optional[int] = None,
                 operand: str = "bf16", drop_path_rate: float = 0.0, global_pool: Optional[str] = None, **kwargs) -> Beit:
    """timm.create_model for the served BEiT ids (a `timm-` prefix and a `.tag` suffix are accepted).  The 384 / 512 ids are not served: KeyError with the served list."""
    if kwargs:
        raise TypeError(f"beit.create_model: unsupported keyword arguments {sorted(kwargs)} (timm would act on them; this module does not build them)")
    arch = name[5:] if name.startswith("timm-") else name
    arch = arch.split(".")[0]
    if arch not in TIMM_BEITS:
        raise KeyError(f"'{name}': served BEiT ids are {sorted(TIMM_BEITS)} (patch 16 at 224 pixels: 197 tokens, head dim 64); the 384 / 512 ids (577 / 1025 tokens) need the "
                       "relative position bias in the streaming attention kernels, a follow-up")
    if pretrained:
        raise RuntimeError("no network access: load a checkpoint with load_state_dict (timm's state_dict names)")
    if drop_path_rate != 0.0:
        raise NotImplementedError("drop_path_rate != 0 is not built for the BEiT ids (timm's default for the family is 0)")
    if img_size % 16 or (img_size // 16) ** 2 + 1 > 256:
        raise ValueError("the patch-16 family needs img_size % 16 == 0 and (img_size / 16)^2 + 1 <= 256 tokens (224 by default; the biased attention kernels hold the whole "
                         "sequence in one CU's LDS)")
    if global_pool not in (None, "avg") and not (global_pool == "" and num_classes == 0):
        raise ValueError("global_pool: 'avg' (the family's default) or '' together with num_classes=0 (the normed tokens [B, N, D])")
    spec = BeitSpec(img_size=img_size, num_classes=num_classes, global_pool="avg" if global_pool is None else global_pool, **TIMM_BEITS[arch])
    return Beit(spec, device=device, backend=backend, seed=seed, operand=operand)
