"""TEST INFRASTRUCTURE: a CPU restatement of timm 0.9.16's SwinV2 (swin_transformer_v2.py) for the window8_256 family, with the cosine window attention written out
forward and backward.  `oracle.bf16ops`' precision switch makes the same code the fp32 oracle ("fp32") and the 16-bit-operand floor ("bf16_operands" / "fp16_operands").

Cosine attention in a 16-bit mode is exactly the arithmetic of csrc/window_attention_cos.hip:
  * the norms |q_i|, |k_j| are fp32 sums over the stored 16-bit values; qn = q / max(|q|, 1e-12) and kn are ROUNDED to the operand format (what autocast does to the fp32
    output of F.normalize ahead of the matmul);
  * S = tau_h (qn kn^T) + bias (+ mask) in fp32, fp32 softmax, P rounded once as the operand of P v, o rounded;
  * backward: D from the rounded o, dS = P (dP - D) in fp32 and rounded as the operand of d(qn) = tau dS kn and d(kn) = tau dS^T qn; the Jacobian of the normalisation in
    fp32, dq = (d(qn) - u (u . d(qn))) / max(|q|, 1e-12) with u the fp32 unit vector, before the ONE rounding of dq and dk; d(bias) and d(tau) from the unrounded dS.
In "fp32" mode every rounding is the identity."""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from oracle import bf16ops
from oracle.swin_ref import shifted_window_mask, window_partition, window_reverse

EPS = 1e-12                       # F.normalize
LOGIT_MAX = math.log(100.0)       # timm clamps logit_scale at ln(1 / 0.01)


def _r(t):
    return t if bf16ops.mode() == "fp32" else bf16ops.rb(t)


def tau_of(logit_scale):
    """exp(clamp(logit_scale, max = ln 100)), any shape"""
    return torch.exp(torch.clamp(logit_scale, max=LOGIT_MAX))


def cos_attention_fwd(q, k, v, tau, lb):
    """q, k, v [W, H, N, hd] (values of the operand format), tau [H], lb [W | 1, H, N, N] (bias + mask).  -> o, and what the backward needs"""
    qd = q.norm(dim=-1, keepdim=True).clamp_min(EPS)
    kd = k.norm(dim=-1, keepdim=True).clamp_min(EPS)
    qn, kn = _r(q / qd), _r(k / kd)
    cos = qn @ kn.transpose(-2, -1)
    s = cos * tau.view(1, -1, 1, 1) + lb
    lse = torch.logsumexp(s, -1, keepdim=True)
    p = torch.exp(s - lse)
    o = _r(_r(p) @ v)
    return o, {"qd": qd, "kd": kd, "qn": qn, "kn": kn, "cos": cos, "p": p, "o": o, "lse": lse.squeeze(-1)}


def cos_attention_bwd(q, k, v, g, tau, saved):
    """-> dict dq, dk, dv (rounded once), dbias [H, N, N] and dtau [H] (fp32 sums of the unrounded dS over the windows)"""
    qd, kd, qn, kn, cos, p, o = (saved[n] for n in ("qd", "kd", "qn", "kn", "cos", "p", "o"))
    t = tau.view(1, -1, 1, 1)
    dv = _r(_r(p).transpose(-2, -1) @ g)
    dp = g @ v.transpose(-2, -1)
    ds = p * (dp - (g * o).sum(-1, keepdim=True))
    dqn = (_r(ds) @ kn) * t
    dkn = (_r(ds).transpose(-2, -1) @ qn) * t
    uq, uk = q / qd, k / kd
    dq = _r((dqn - uq * (uq * dqn).sum(-1, keepdim=True)) / qd)
    dk = _r((dkn - uk * (uk * dkn).sum(-1, keepdim=True)) / kd)
    return {"dq": dq, "dk": dk, "dv": dv, "dbias": ds.sum(0), "dtau": (ds * cos).sum((0, 2, 3)), "dtau_abs": (ds.abs() * cos.abs()).sum((0, 2, 3))}


class CosAttention(torch.autograd.Function):
    """the two functions above as one autograd node: (q, k, v, tau [H], bias [H, N, N], mask-per-window [W | 1, 1, N, N] or None) -> o.  `holder` (any object or None):
    the backward leaves `holder.dtau_abs` = sum |dS| |qn . kn| per head there, the non-cancelling scale of d(tau) = sum dS (qn . kn) (sum_j dS_ij = 0: the terms cancel)"""

    @staticmethod
    def forward(ctx, q, k, v, tau, bias, maskw, holder=None):
        lb = bias[None] if maskw is None else bias[None] + maskw
        o, saved = cos_attention_fwd(q, k, v, tau, lb)
        ctx.saved, ctx.holder = saved, holder
        ctx.save_for_backward(q, k, v, tau)
        return o

    @staticmethod
    def backward(ctx, g):
        q, k, v, tau = ctx.saved_tensors
        r = cos_attention_bwd(q, k, v, _r(g), tau, ctx.saved)
        if ctx.holder is not None:
            ctx.holder.dtau_abs = r["dtau_abs"].detach()
        return r["dq"], r["dk"], r["dv"], r["dtau"], r["dbias"], None, None


# ---- the model -------------------------------------------------------------------------------------------------------------------------------------
# timm 0.9.16 swin_transformer_v2.py for the window8_256 family, with timm's state_dict names (the points are listed in visiondk_amd/swinv2.py's docstring; pinned
# against transformers.Swinv2Model by tests/test_swinv2_ref.py).  16-bit modes: every Linear through bf16ops.linear, its output held in 16 bits where autocast holds it
# (bf16ops.q), LayerNorm and the residual stream in fp32, GELU through bf16ops.gelu; the parameter side (cpb_mlp, 16 sigmoid, exp(clamp)) and the pooled head in fp32.
WS = 8


def coords_table(ws=WS):
    r = torch.arange(-(ws - 1), ws, dtype=torch.float32)
    t = torch.stack(torch.meshgrid([r, r], indexing="ij")).permute(1, 2, 0).contiguous().unsqueeze(0)          # [1, 2 ws - 1, 2 ws - 1, 2]
    t[:, :, :, 0] /= ws - 1
    t[:, :, :, 1] /= ws - 1
    t *= 8
    return torch.sign(t) * torch.log2(torch.abs(t) + 1.0) / math.log2(8)


def relative_position_index(ws=WS):
    coords = torch.stack(torch.meshgrid([torch.arange(ws), torch.arange(ws)], indexing="ij")).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += ws - 1
    rel[:, :, 1] += ws - 1
    rel[:, :, 0] *= 2 * ws - 1
    return rel.sum(-1)


class WindowAttentionV2(nn.Module):
    def __init__(self, dim, heads, ws=WS):
        super().__init__()
        self.heads, self.ws = heads, ws
        self.logit_scale = nn.Parameter(torch.log(10 * torch.ones((heads, 1, 1))))
        self.cpb_mlp = nn.Sequential(nn.Linear(2, 512, bias=True), nn.ReLU(inplace=True), nn.Linear(512, heads, bias=False))
        self.register_buffer("relative_coords_table", coords_table(ws), persistent=False)
        self.register_buffer("relative_position_index", relative_position_index(ws), persistent=False)
        self.qkv = nn.Linear(dim, dim * 3, bias=False)
        self.q_bias = nn.Parameter(torch.zeros(dim))
        self.register_buffer("k_bias", torch.zeros(dim), persistent=False)
        self.v_bias = nn.Parameter(torch.zeros(dim))
        self.proj = nn.Linear(dim, dim)

    def logit_scale_grad_scale(self):
        """after a backward: tau sum |dS| |qn . kn| per head (0 where the clamp stops the gradient), shaped like logit_scale -- what went into d(logit_scale), in the way
        tests/rowbound.py scales an output row by the absolute-value products that went into it"""
        ls = self.logit_scale.detach().view(-1)
        return (self.dtau_abs * tau_of(ls) * (ls <= LOGIT_MAX)).view_as(self.logit_scale)

    def bias(self):
        n = self.ws * self.ws
        t = self.cpb_mlp(self.relative_coords_table).view(-1, self.heads)
        return 16 * torch.sigmoid(t[self.relative_position_index.view(-1)].view(n, n, -1).permute(2, 0, 1).contiguous())

    def forward(self, x, mask=None):
        B_, n, C = x.shape
        qkv = bf16ops.q(bf16ops.linear(x, self.qkv.weight, torch.cat((self.q_bias, self.k_bias, self.v_bias))))
        q, k, v = qkv.reshape(B_, n, 3, self.heads, -1).permute(2, 0, 3, 1, 4).unbind(0)
        maskw = None if mask is None else mask.repeat(B_ // mask.shape[0], 1, 1).unsqueeze(1)
        o = CosAttention.apply(q, k, v, tau_of(self.logit_scale.view(-1)), self.bias(), maskw, self)
        return bf16ops.q(bf16ops.linear(o.transpose(1, 2).reshape(B_, n, C), self.proj.weight, self.proj.bias))


class MlpV2(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.fc1 = nn.Linear(dim, 4 * dim)
        self.fc2 = nn.Linear(4 * dim, dim)

    def forward(self, x):
        return bf16ops.q(bf16ops.linear(bf16ops.gelu(bf16ops.linear(x, self.fc1.weight, self.fc1.bias)), self.fc2.weight, self.fc2.bias))


class SwinV2Block(nn.Module):
    def __init__(self, dim, res, heads, ws, shift):
        super().__init__()
        if res <= ws:
            ws, shift = res, 0
        self.res, self.ws, self.shift = res, ws, shift
        self.attn = WindowAttentionV2(dim, heads, ws)
        self.norm1 = nn.LayerNorm(dim)
        self.mlp = MlpV2(dim)
        self.norm2 = nn.LayerNorm(dim)
        self.register_buffer("attn_mask", shifted_window_mask(res, res, ws, shift) if shift > 0 else None, persistent=False)
        self.drop = None                       # None, or (f1 [B], f2 [B]): timm's per-sample drop-path factors, handed in by the test

    def _attn(self, x):
        B, H, W, C = x.shape
        h = torch.roll(x, (-self.shift, -self.shift), (1, 2)) if self.shift else x
        w = self.attn(window_partition(h, self.ws).view(-1, self.ws * self.ws, C), self.attn_mask)
        h = window_reverse(w.view(-1, self.ws, self.ws, C), self.ws, H, W)
        return torch.roll(h, (self.shift, self.shift), (1, 2)) if self.shift else h

    def forward(self, x):                      # [B, H, W, C]
        f1, f2 = (1.0, 1.0) if self.drop is None else (f.view(-1, 1, 1, 1) for f in self.drop)
        x = x + self.norm1(self._attn(x)) * f1
        return x + self.norm2(self.mlp(x)) * f2


class PatchMergingV2(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = nn.LayerNorm(2 * dim)

    def forward(self, x):
        B, H, W, C = x.shape
        x = x.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 4, 2, 5).flatten(3)
        return self.norm(bf16ops.q(bf16ops.linear(x, self.reduction.weight)))


class SwinV2Stage(nn.Module):
    def __init__(self, dim_in, dim, res, depth, heads, ws, downsample):
        super().__init__()
        self.downsample = PatchMergingV2(dim_in) if downsample else nn.Identity()
        self.blocks = nn.Sequential(*[SwinV2Block(dim, res, heads, ws, 0 if j % 2 == 0 else ws // 2) for j in range(depth)])

    def forward(self, x):
        return self.blocks(self.downsample(x))


class _PatchEmbed(nn.Module):
    def __init__(self, in_chans, dim):
        super().__init__()
        self.proj = nn.Conv2d(in_chans, dim, 4, 4)
        self.norm = nn.LayerNorm(dim)

    def forward(self, x):
        if bf16ops.mode() == "fp32":
            return self.norm(self.proj(x).permute(0, 2, 3, 1))
        B, Cin, S, _ = x.shape
        g = S // 4
        pt = x.reshape(B, Cin, g, 4, g, 4).permute(0, 2, 4, 1, 3, 5).reshape(B, g, g, Cin * 16)
        return self.norm(bf16ops.q(bf16ops.linear(pt, self.proj.weight.view(self.proj.weight.shape[0], -1), self.proj.bias)))


class _Head(nn.Module):
    def __init__(self, dim, num_classes):
        super().__init__()
        self.fc = nn.Linear(dim, num_classes) if num_classes > 0 else nn.Identity()

    def forward(self, x):
        return self.fc(x.mean((1, 2)))


class SwinV2Ref(nn.Module):
    """swinv2_base_window8_256: embed_dim 128, depths (2, 2, 18, 2), heads (4, 8, 16, 32)"""

    def __init__(self, img_size=256, in_chans=3, num_classes=1000, embed_dim=128, depths=(2, 2, 18, 2), heads=(4, 8, 16, 32), window=WS):
        super().__init__()
        self.num_classes = num_classes
        self.patch_embed = _PatchEmbed(in_chans, embed_dim)
        res = img_size // 4
        layers, dim_in = [], embed_dim
        for i, (d, h) in enumerate(zip(depths, heads)):
            dim = embed_dim * 2 ** i
            if i > 0:
                res //= 2
            layers.append(SwinV2Stage(dim_in, dim, res, d, h, window, downsample=i > 0))
            dim_in = dim
        self.layers = nn.Sequential(*layers)
        self.norm = nn.LayerNorm(dim_in)
        self.head = _Head(dim_in, num_classes)
        self.num_features = dim_in
        for stage in self.layers:                # timm's _init_respostnorm
            for blk in stage.blocks:
                for nrm in (blk.norm1, blk.norm2):
                    nn.init.zeros_(nrm.weight)
                    nn.init.zeros_(nrm.bias)
        for m in self.modules():                 # the reference's reset_parameters
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, mean=0, std=0.02)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, mean=0, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def set_drop_path(self, factors):
        """factors [2 * blocks, B] (row 2 k: block k's attention branch, 2 k + 1: its MLP branch; entries 0 or 1 / keep_prob), or None"""
        k = 0
        for stage in self.layers:
            for blk in stage.blocks:
                blk.drop = None if factors is None else (factors[2 * k], factors[2 * k + 1])
                k += 1

    def forward_features(self, x):
        return self.norm(self.layers(self.patch_embed(x)))

    def forward(self, x):
        x = self.forward_features(x)
        return self.head(x) if self.num_classes > 0 else x
