"""TEST INFRASTRUCTURE: a CPU restatement of timm 0.9.16's BEiT (beit.py) for the patch16 family, with the biased attention written out forward and backward.
`oracle.bf16ops`' precision switch makes the same code the fp32 oracle ("fp32") and the 16-bit-operand floor ("bf16_operands" / "fp16_operands").

Biased attention in a 16-bit mode is exactly the arithmetic csrc/attention_bias.hip states:
  * S = fp32(q . k) * scale + bias in fp32 from the stored 16-bit q and k; fp32 softmax with the exact maximum; P rounded once as the left operand of P v; o rounded once;
  * backward: P = exp(S - lse), dP = dO v^T, D = rowsum(dO o) on the rounded tensors, dS = P (dP - D) in fp32; d(bias) = sum over the batch of the UNROUNDED dS; dS is
    rounded as the operand of dq = scale dS k and dk = scale dS^T q, P as the operand of dv = P^T dO; dq, dk, dv rounded once.
In "fp32" mode every rounding is the identity.

The model (from knowledge of the pinned timm version; the points are listed in visiondk_amd/beit.py's docstring; pinned against transformers.BeitModel by
tests/test_beit_ref.py): no absolute position embedding, a relative position bias table per block with three extra entries for the class token, qkv without a bias parameter
(cat(q_bias, 0, v_bias)), gamma_1 / gamma_2 directly on the block, mean pooling of the patch tokens through fc_norm.  16-bit modes: every Linear through bf16ops.linear with
its output held in 16 bits (bf16ops.q), LayerNorm and the residual stream in fp32, `h * gamma` promoted to fp32 (csrc/layerscale_residual.hip), the table gather, the pooled
fc_norm and the head in fp32."""
from __future__ import annotations

import torch
import torch.nn as nn

from oracle import bf16ops
from oracle.vit_ref import Mlp


def _r(t):
    return t if bf16ops.mode() == "fp32" else bf16ops.rb(t)


def relative_position_index(G: int) -> torch.Tensor:
    """[N, N], N = G^2 + 1, into a table of R = (2 G - 1)^2 + 3 rows: patch to patch (dy + G - 1)(2 G - 1) + (dx + G - 1); row 0 (class query) R - 3, column 0 (class key)
    R - 2, entry (0, 0) R - 1"""
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


def gather_bias(table: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    """table [R, H] -> bias [H, N, N]"""
    n = index.shape[0]
    return table[index.view(-1)].view(n, n, -1).permute(2, 0, 1).contiguous()


def bias_attention_fwd(q, k, v, sc, bias):
    """q, k, v [B, H, N, hd] (values of the operand format), bias [H, N, N] -> o, and what the backward needs"""
    s = (q @ k.transpose(-2, -1)) * sc + bias
    lse = torch.logsumexp(s, -1, keepdim=True)
    p = torch.exp(s - lse)
    o = _r(_r(p) @ v)
    return o, {"p": p, "o": o, "lse": lse.squeeze(-1)}


def bias_attention_bwd(q, k, v, g, sc, saved):
    """-> dict dq, dk, dv (rounded once) and dbias [H, N, N] (the fp32 sum of the unrounded dS over the batch)"""
    p, o = saved["p"], saved["o"]
    dv = _r(_r(p).transpose(-2, -1) @ g)
    dp = g @ v.transpose(-2, -1)
    ds = p * (dp - (g * o).sum(-1, keepdim=True))
    dq = _r((_r(ds) @ k) * sc)
    dk = _r((_r(ds).transpose(-2, -1) @ q) * sc)
    return {"dq": dq, "dk": dk, "dv": dv, "dbias": ds.sum(0)}


class BiasAttention(torch.autograd.Function):
    """the two functions above as one autograd node: (q, k, v [B, H, N, hd], bias [H, N, N], scale) -> o"""

    @staticmethod
    def forward(ctx, q, k, v, bias, sc):
        o, saved = bias_attention_fwd(q, k, v, sc, bias)
        ctx.saved, ctx.sc = saved, sc
        ctx.save_for_backward(q, k, v)
        return o

    @staticmethod
    def backward(ctx, g):
        q, k, v = ctx.saved_tensors
        r = bias_attention_bwd(q, k, v, _r(g), ctx.sc, ctx.saved)
        return r["dq"], r["dk"], r["dv"], r["dbias"], None


# ---- the model -------------------------------------------------------------------------------------------------------------------------------------
class Attention(nn.Module):
    def __init__(self, dim, heads, grid):
        super().__init__()
        self.heads, self.scale = heads, (dim // heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=False)
        self.q_bias = nn.Parameter(torch.zeros(dim))
        self.register_buffer("k_bias", torch.zeros(dim), persistent=False)
        self.v_bias = nn.Parameter(torch.zeros(dim))
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * grid - 1) ** 2 + 3, heads))
        self.register_buffer("relative_position_index", relative_position_index(grid), persistent=False)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):
        B, n, C = x.shape
        qkv = bf16ops.q(bf16ops.linear(x, self.qkv.weight, torch.cat((self.q_bias, self.k_bias, self.v_bias))))
        q, k, v = qkv.reshape(B, n, 3, self.heads, -1).permute(2, 0, 3, 1, 4).unbind(0)
        o = BiasAttention.apply(q, k, v, gather_bias(self.relative_position_bias_table, self.relative_position_index), self.scale)
        return bf16ops.linear(o.transpose(1, 2).reshape(B, n, C), self.proj.weight, self.proj.bias)


class Block(nn.Module):
    def __init__(self, dim, heads, grid, eps, init_values):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=eps)
        self.attn = Attention(dim, heads, grid)
        self.norm2 = nn.LayerNorm(dim, eps=eps)
        self.mlp = Mlp(dim, 4 * dim)
        self.gamma_1 = nn.Parameter(init_values * torch.ones(dim))
        self.gamma_2 = nn.Parameter(init_values * torch.ones(dim))

    def forward(self, x):
        x = x + self.gamma_1 * bf16ops.q(self.attn(bf16ops.q(self.norm1(x))))
        return x + self.gamma_2 * bf16ops.q(self.mlp(bf16ops.q(self.norm2(x))))


class _PatchEmbed(nn.Module):
    def __init__(self, in_chans, dim):
        super().__init__()
        self.proj = nn.Conv2d(in_chans, dim, 16, 16)

    def forward(self, x):
        if bf16ops.mode() == "fp32":
            return self.proj(x).flatten(2).transpose(1, 2)
        B, Cc, S, _ = x.shape
        g = S // 16
        pt = x.reshape(B, Cc, g, 16, g, 16).permute(0, 2, 4, 1, 3, 5).reshape(B, g * g, Cc * 256)
        return bf16ops.q(bf16ops.linear(pt, self.proj.weight.reshape(self.proj.out_channels, -1), self.proj.bias))


class BeitRef(nn.Module):
    """beit_base_patch16_224: dim 768, depth 12, heads 12, init_values 0.1; global_pool 'avg' (timm's default for the family: mean of the patch tokens -> fc_norm -> head) or
    '' with num_classes = 0 (norm over every token, the tokens returned)"""

    def __init__(self, img_size=224, in_chans=3, num_classes=1000, dim=768, depth=12, heads=12, init_values=0.1, eps=1e-6, global_pool="avg"):
        super().__init__()
        assert global_pool in ("avg", "")
        self.num_classes, self.global_pool = num_classes, global_pool
        grid = img_size // 16
        self.patch_embed = _PatchEmbed(in_chans, dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, dim))
        self.blocks = nn.Sequential(*[Block(dim, heads, grid, eps, init_values) for _ in range(depth)])
        if global_pool == "avg":
            self.norm = nn.Identity()
            self.fc_norm = nn.LayerNorm(dim, eps=eps)
        else:
            self.norm = nn.LayerNorm(dim, eps=eps)
        self.head = nn.Linear(dim, num_classes) if num_classes > 0 else nn.Identity()
        nn.init.trunc_normal_(self.cls_token, std=0.02)          # timm's init ...
        for m in self.modules():                                  # ... then the reference's reset_parameters
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, mean=0, std=0.02)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, mean=0, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def forward_tokens(self, x):
        t = self.patch_embed(x)
        return self.blocks(torch.cat([self.cls_token.expand(t.shape[0], -1, -1), t], dim=1))

    def forward(self, x):
        t = self.norm(self.forward_tokens(x))
        if self.global_pool == "":
            return t
        return self.head(self.fc_norm(t[:, 1:].mean(1)))
