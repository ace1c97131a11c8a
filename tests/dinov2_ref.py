"""TEST INFRASTRUCTURE: a CPU restatement of timm 0.9.16's DINOv2 ViTs (`vit_{small,base,large}_patch14_dinov2`: vision_transformer.py with init_values = 1e-5), built from
oracle/vit_ref.py's pieces.  `oracle.bf16ops`' precision switch makes the same code the fp32 oracle ("fp32") and the 16-bit-operand floor ("bf16_operands" / "fp16_operands").

What the family adds to oracle.vit_ref.VisionTransformerRef is LayerScale on the residual stream: x = x + ls1(attn(norm1 x)), x = x + ls2(mlp(norm2 x)), ls(h) = h * gamma.
In a 16-bit mode this is the reference's autocast arithmetic, and that of csrc/layerscale_residual.hip: the branch's last Linear (attn.proj / mlp.fc2) leaves h in the operand
format (bf16ops.q: value rounded going forward, gradient rounded coming back), `h * gamma` promotes to fp32 and the add is fp32; on the way back gamma * dy is rounded ONCE (q's
backward) and dgamma = sum dy * h is an fp32 sum over the stored 16-bit h.  The patch embedding's output is held in 16 bits as well (the cat with the fp32 class token widens
it); the final norm and the head are fp32 in every mode (visiondk_amd.dinov2 runs the head on the fp32 GEMM).  In "fp32" mode every rounding is the identity.
state_dict names equal timm's; pinned against transformers.Dinov2Model by tests/test_dinov2_ref.py."""
from __future__ import annotations

import torch
import torch.nn as nn

from oracle import bf16ops
from oracle.vit_ref import Attention, Mlp, PatchEmbed


class LayerScale(nn.Module):
    def __init__(self, dim, init_values=1e-5):
        super().__init__()
        self.gamma = nn.Parameter(init_values * torch.ones(dim))

    def forward(self, h):
        return h * self.gamma


class Block(nn.Module):
    def __init__(self, dim, heads, mlp_dim, eps, init_values):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=eps)
        self.attn = Attention(dim, heads)
        self.ls1 = LayerScale(dim, init_values)
        self.norm2 = nn.LayerNorm(dim, eps=eps)
        self.mlp = Mlp(dim, mlp_dim)
        self.ls2 = LayerScale(dim, init_values)

    def forward(self, x):
        x = x + self.ls1(bf16ops.q(self.attn(bf16ops.q(self.norm1(x)))))
        return x + self.ls2(bf16ops.q(self.mlp(bf16ops.q(self.norm2(x)))))


class Dinov2Ref(nn.Module):
    """vit_large_patch14_dinov2: dim 1024, depth 24, heads 16, mlp 4096, img_size 518 (1370 tokens)"""

    def __init__(self, img_size=518, patch_size=14, in_chans=3, num_classes=1000, dim=1024, depth=24, heads=16, mlp_dim=4096, eps=1e-6, init_values=1e-5, global_pool="token"):
        super().__init__()
        self.num_classes, self.global_pool = num_classes, global_pool
        n = (img_size // patch_size) ** 2 + 1
        self.patch_embed = PatchEmbed(patch_size, in_chans, dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, n, dim))
        self.blocks = nn.Sequential(*[Block(dim, heads, mlp_dim, eps, init_values) for _ in range(depth)])
        self.norm = nn.LayerNorm(dim, eps=eps)
        self.head = nn.Linear(dim, num_classes) if num_classes > 0 else nn.Identity()
        nn.init.trunc_normal_(self.pos_embed, std=0.02)      # timm's init ...
        nn.init.normal_(self.cls_token, std=1e-6)
        for m in self.modules():                             # ... then the reference's reset_parameters
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, mean=0, std=0.02)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, mean=0, std=0.02)
                nn.init.zeros_(m.bias)

    def _embed(self, x):
        if bf16ops.mode() == "fp32":
            return self.patch_embed.proj(x).flatten(2).transpose(1, 2)
        p = self.patch_embed.proj
        k = p.kernel_size[0]
        B, Cc, H, W = x.shape
        pt = x.reshape(B, Cc, H // k, k, W // k, k).permute(0, 2, 4, 1, 3, 5).reshape(B, (H // k) * (W // k), Cc * k * k)
        return bf16ops.q(bf16ops.linear(pt, p.weight.reshape(p.out_channels, -1), p.bias))

    def forward_tokens(self, x):
        t = self._embed(x)
        t = torch.cat([self.cls_token.expand(t.shape[0], -1, -1), t], dim=1) + self.pos_embed
        return self.blocks(t)

    def forward_features(self, x):
        return self.norm(self.forward_tokens(x))

    def forward(self, x):
        f = self.forward_features(x)
        if self.global_pool == "":
            return f
        return self.head(f[:, 0])
