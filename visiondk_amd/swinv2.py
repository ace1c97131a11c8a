"""SwinV2 (timm `swinv2_*_window8_256`) on the HIP kernels: the family the reference's configs list as a one-line alternative to their default Swin backbone
(`timm-swinv2_base_window8_256.ms_in1k`).  Autograd-node form, modelled on `swin.SwinTransformerAutograd`: a torch Module with timm's state_dict names whose arithmetic
runs in autograd nodes over the library's kernels.  A native `vdk_swinv2_*` engine (and with it FusedTrainStep / FaceTrainStep / forward_precise) and a fused
"LayerNorm + residual" epilogue are follow-ups; this module trains under a plain torch optimizer (with a loss scale for fp16 operands).

timm 0.9.16 semantics as restated here (swin_transformer_v2.py; pinned against transformers.Swinv2Model through tests/swinv2_ref.py, tests/test_swinv2_ref.py):
  * patch_embed.proj = Conv 4 x 4 stride 4, then patch_embed.norm; features are NHWC.
  * stage i > 0 STARTS with `downsample`: the 2 x 2 gather reshape(B, H/2, 2, W/2, 2, C).permute(0, 1, 3, 4, 2, 5).flatten(3), then `reduction` Linear(4C -> 2C, no
    bias), then `norm` LayerNorm(2C) -- the reverse of v1's norm-then-reduce.
  * block (residual-post-norm): x = x + drop_path(norm1(attn(x))); x = x + drop_path(norm2(mlp(x))).  LayerNorm eps 1e-5, MLP ratio 4, exact-erf GELU.
  * odd blocks of a stage shift by 4; a map no larger than the window makes the window the map and the shift 0 (the last stage, 8 x 8).  The shift mask is 0 / -100, added once.
  * attn.qkv = Linear(C -> 3C) without a bias parameter; the bias used is cat(q_bias, zeros, v_bias); q_bias and v_bias are parameters, k_bias is a non-persistent zero buffer.
  * attn.logit_scale: parameter [H, 1, 1], initialised to ln 10, used as exp(clamp(., max = ln 100)) on the cosine of L2-normalised q and k (F.normalize, eps 1e-12).
  * attn.cpb_mlp: Linear(2 -> 512, bias) - ReLU - Linear(512 -> H, no bias) over the coordinate table [1, 15, 15, 2] = meshgrid(arange(-7, 8), arange(-7, 8)) / 7 * 8
    mapped through sign(x) log2(|x| + 1) / 3 (a non-persistent buffer, like relative_position_index);
    bias = 16 sigmoid(cpb_mlp(table).view(225, H)[index].view(64, 64, H).permute(2, 0, 1)).
  * after the stages `norm` and `head.fc` (global average pool); num_classes = 0 returns the normed NHWC map [B, 8, 8, C].
  * init: timm's own, then `_init_respostnorm`: norm1 / norm2 weight AND bias of every block are 0, so every block is the identity at initialisation.  The reference's
    reset_parameters re-draws every Conv / Linear weight N(0, 0.02) and zeroes Linear biases (both cpb_mlp Linears included); it leaves LayerNorms, q_bias, v_bias and
    logit_scale alone.

Arithmetic: `operand` "bf16" | "fp16" is the format of every GEMM and attention operand; residual stream and master weights fp32; every Linear on the 16-bit MFMA GEMM
(bias / GELU epilogues, weight gradients in TN form; outputs held in the operand format wherever autocast holds them); LayerNorm through ops.layernorm_*; attention through vdk_wa_cos_fwd / bwd on qkv rows kept in image order (rowidx).
The batch-independent parameter side stays in fp32 torch ops on the device: the cpb_mlp on its 225 rows, 16 sigmoid, exp(clamp) and its chain rule; the gather's backward is
vdk_relpos_bias_table_grad (fixed order).  The two residual adds per block and the widening of a 16-bit GEMM output for the fp32 LayerNorm are torch ops."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence

import torch
import torch.nn as nn

from . import _lib, ops
from ._engine import OPERANDS, _Holder, check_image
from ._nodes import _BiasGather, _cast, _LinearFn, _Lin, _LN, _Mlp, _Pool
from .swin import _init_conv_linear, _merge2x2, _rel_index, _shift_mask, _stem_patches, _uses_table, _window_rows

WS = 8
N = WS * WS
LOGIT_MAX = math.log(100.0)       # timm clamps logit_scale at ln(1 / 0.01)
_OPF = {torch.bfloat16: 0, torch.float16: 1}


@dataclass(frozen=True)
class SwinV2Spec:
    img_size: int = 256
    in_chans: int = 3
    num_classes: int = 1000
    embed_dim: int = 128
    depths: Sequence[int] = (2, 2, 18, 2)
    heads: Sequence[int] = (4, 8, 16, 32)
    ln_eps: float = 1e-5


TIMM_SWINV2S = {
    "swinv2_tiny_window8_256": dict(embed_dim=96, depths=(2, 2, 6, 2), heads=(3, 6, 12, 24)),
    "swinv2_small_window8_256": dict(embed_dim=96, depths=(2, 2, 18, 2), heads=(3, 6, 12, 24)),
    "swinv2_base_window8_256": dict(embed_dim=128, depths=(2, 2, 18, 2), heads=(4, 8, 16, 32)),
}


def tau_of(logit_scale: torch.Tensor) -> torch.Tensor:
    """the per-head logit multiplier the kernels take: exp(clamp(logit_scale, max = ln 100))"""
    return torch.exp(torch.clamp(logit_scale, max=LOGIT_MAX))


def logit_scale_grad(dtau: torch.Tensor, logit_scale: torch.Tensor) -> torch.Tensor:
    """chain rule from the kernel's d(tau) to d(logit_scale): tau where the clamp passes (logit_scale <= ln 100, the boundary included, as torch.clamp does), else 0"""
    ls = logit_scale.reshape(dtau.shape)
    return (dtau * tau_of(ls) * (ls <= LOGIT_MAX).to(dtau.dtype)).reshape(logit_scale.shape)


def coords_table(ws: int = WS) -> torch.Tensor:
    """[1, 2 ws - 1, 2 ws - 1, 2]: log-spaced relative coordinates (pretrained_window_size = 0)"""
    r = torch.arange(-(ws - 1), ws, dtype=torch.float32)
    t = torch.stack(torch.meshgrid(r, r, indexing="ij")).permute(1, 2, 0).contiguous().unsqueeze(0)
    t = t / (ws - 1) * 8
    return torch.sign(t) * torch.log2(t.abs() + 1.0) / math.log2(8)


def rel_index(ws: int = WS) -> torch.Tensor:
    return _rel_index(ws)


# ---- the attention node (the model-independent nodes: _nodes.py) -----------------------------------------------------------------------------------
class _CosAttn(torch.autograd.Function):
    """the attention step of timm's SwinV2 WindowAttention on 16-bit qkv rows (csrc/window_attention_cos.hip); rowidx (int32 [T], a permutation) = the tensor row of every
    (window, token): qkv and o stay in image order.  logit_scale f32 [H]: tau = exp(clamp) goes to the kernel, d(tau) comes back through logit_scale_grad."""

    @staticmethod
    def forward(ctx, qkv, logit_scale, bias, mask, heads, be, rowidx):
        T, C3 = qkv.shape
        Cc = C3 // 3
        windows = T // N
        o = torch.empty((T, Cc), dtype=qkv.dtype, device=qkv.device)
        lse = torch.empty((windows, heads, N), dtype=torch.float32, device=qkv.device)
        biasc, tau = bias.detach().contiguous(), tau_of(logit_scale.detach()).contiguous()
        nW = 0 if mask is None else mask.shape[0]
        ws, n = ops._ws(be, be.lib.vdk_wa_cos_fwd_workspace_bytes, nW, heads, device=qkv.device)
        be.check(be.lib.vdk_wa_cos_fwd(be.ptr(qkv), C3, be.ptr(o), Cc, be.ptr(lse), be.ptr(tau), be.ptr(biasc), be.ptr(mask), nW, windows, heads, be.ptr(rowidx),
                                       _OPF[qkv.dtype], be.ptr(ws), n, be.stream()), "vdk_wa_cos_fwd")
        ctx.save_for_backward(qkv, o, lse, biasc, tau, logit_scale)
        ctx.mask, ctx.heads, ctx.be, ctx.rowidx = mask, heads, be, rowidx
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse, biasc, tau, logit_scale = ctx.saved_tensors
        be, heads, mask = ctx.be, ctx.heads, ctx.mask
        T, C3 = qkv.shape
        Cc = C3 // 3
        windows = T // N
        nW = 0 if mask is None else mask.shape[0]
        do = _cast(be, do.contiguous(), qkv.dtype)
        dqkv = torch.empty_like(qkv)
        dbias = torch.empty((heads, N, N), dtype=torch.float32, device=qkv.device)
        dtau = torch.empty((heads,), dtype=torch.float32, device=qkv.device)
        ws, n = ops._ws(be, be.lib.vdk_wa_cos_bwd_workspace_bytes, windows, nW, heads, device=qkv.device)
        be.check(be.lib.vdk_wa_cos_bwd(be.ptr(qkv), C3, be.ptr(o), be.ptr(do), Cc, be.ptr(lse), be.ptr(tau), be.ptr(biasc), be.ptr(mask), nW, windows, heads, be.ptr(ctx.rowidx),
                                       be.ptr(dqkv), C3, be.ptr(dbias), be.ptr(dtau), _OPF[qkv.dtype], be.ptr(ws), n, be.stream()), "vdk_wa_cos_bwd")
        return dqkv, logit_scale_grad(dtau, logit_scale), dbias, None, None, None, None


# ---- modules with timm's names -------------------------------------------------------------------------------------------------------------------
class WindowAttention(nn.Module):
    def __init__(self, dim: int, heads: int, dev):
        super().__init__()
        self.heads = heads
        self.logit_scale = nn.Parameter(torch.log(10 * torch.ones((heads, 1, 1), device=dev)))
        self.cpb_mlp = nn.Sequential(nn.Linear(2, 512, bias=True, device=dev), nn.ReLU(inplace=True), nn.Linear(512, heads, bias=False, device=dev))
        self.register_buffer("relative_coords_table", coords_table().to(dev), persistent=False)
        idx = rel_index()
        self.register_buffer("relative_position_index", idx.to(dev), persistent=False)
        self.register_buffer("_uses", _uses_table(idx, WS).to(dev), persistent=False)
        self.qkv = nn.Linear(dim, 3 * dim, bias=False, device=dev)
        self.q_bias = nn.Parameter(torch.zeros(dim, device=dev))
        self.register_buffer("k_bias", torch.zeros(dim, device=dev), persistent=False)
        self.v_bias = nn.Parameter(torch.zeros(dim, device=dev))
        self.proj = nn.Linear(dim, dim, device=dev)

    def bias(self, be) -> torch.Tensor:
        """16 sigmoid(cpb_mlp(table)[index]) as [H, 64, 64]: fp32 torch ops on 225 rows, the gather's backward in a fixed order"""
        t = self.cpb_mlp(self.relative_coords_table).view(-1, self.heads)
        return 16.0 * torch.sigmoid(_BiasGather.apply(t, self.relative_position_index, self._uses, be))


class Mlp(nn.Module):
    def __init__(self, dim: int, dev):
        super().__init__()
        self.fc1 = nn.Linear(dim, 4 * dim, device=dev)
        self.fc2 = nn.Linear(4 * dim, dim, device=dev)


class SwinV2Block(nn.Module):
    def __init__(self, dim: int, res: int, heads: int, shift: int, eps: float, be, dt, dev):
        super().__init__()
        if res < WS or res % WS:
            raise ValueError("feature maps must be multiples of the 8 x 8 window (img_size % 256 == 0 for the window8_256 family)")
        if res == WS:
            shift = 0
        self.res, self.shift, self.eps, self.be, self.heads, self.dt = res, shift, eps, be, heads, dt
        self.attn = WindowAttention(dim, heads, dev)
        self.norm1 = nn.LayerNorm(dim, eps=eps, device=dev)
        self.mlp = Mlp(dim, dev)
        self.norm2 = nn.LayerNorm(dim, eps=eps, device=dev)
        self.register_buffer("attn_mask", _shift_mask(res, res, WS, shift).to(dev) if shift else None, persistent=False)
        self._perm = {}

    def _perms(self, B: int, dev):
        if B not in self._perm:      # (one batch size kept)
            self._perm = {B: _window_rows(self.res, self.shift, WS, B).to(dev)}
        return self._perm[B]

    def rows(self, x, B: int, f1=None, f2=None):
        """the block on the f32 token rows [B * H * W, C] in image order; f1, f2: per-row drop-path factors [rows, 1] or None.  Each branch leaves its last GEMM in the
        operand format, as under the reference's autocast, and is widened (a torch copy, like the residual adds) for the fp32 LayerNorm.  Measured on the tiny model of
        tests/test_swinv2.py: with fp32 GEMM outputs feeding the post-norms the fp16 logit_scale gradients sat 3.6 - 4.5 x the 16-bit restatement's own deviation from fp32,
        with the rounding in place every gradient is within 1.7 x."""
        be, a, dt = self.be, self.attn, self.dt
        qkv = _Lin.apply(x, a.qkv.weight, torch.cat((a.q_bias, a.k_bias, a.v_bias)), None, dt, dt, be)
        o = _CosAttn.apply(qkv, a.logit_scale.view(-1), a.bias(be), self.attn_mask, self.heads, be, self._perms(B, x.device))
        h = _LN.apply(_Lin.apply(o, a.proj.weight, a.proj.bias, None, dt, dt, be).float(), self.norm1.weight, self.norm1.bias, self.eps, torch.float32, be)
        x = x + (h if f1 is None else h * f1)
        m = self.mlp
        h = _LN.apply(_Mlp.apply(x, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, None, dt, be).float(), self.norm2.weight, self.norm2.bias, self.eps, torch.float32, be)
        return x + (h if f2 is None else h * f2)


class PatchMerging(nn.Module):
    def __init__(self, dim: int, eps: float, be, dt, dev):
        super().__init__()
        self.eps, self.be, self.dt = eps, be, dt
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False, device=dev)
        self.norm = nn.LayerNorm(2 * dim, eps=eps, device=dev)

    def forward(self, x):
        y = _Lin.apply(_merge2x2(x), self.reduction.weight, None, None, self.dt, self.dt, self.be).float()
        return _LN.apply(y, self.norm.weight, self.norm.bias, self.eps, torch.float32, self.be)


class SwinV2Stage(nn.Module):
    def __init__(self, dim_in: int, dim: int, res: int, depth: int, heads: int, downsample: bool, eps: float, be, dt, dev):
        super().__init__()
        self.downsample = PatchMerging(dim_in, eps, be, dt, dev) if downsample else nn.Identity()
        self.blocks = nn.Sequential(*[SwinV2Block(dim, res, heads, 0 if j % 2 == 0 else WS // 2, eps, be, dt, dev) for j in range(depth)])


class SwinTransformerV2(nn.Module):
    """timm.create_model('swinv2_*_window8_256', num_classes=C) as autograd nodes over the kernels: forward(x [B, 3, S, S]) -> logits [B, C]; num_classes = 0:
    forward_features, the normed NHWC map [B, S/32, S/32, C_last].  train() mode applies stochastic depth (`drop_path_rate`, timm's default for the family is 0.1):
    per-sample factors drawn on the device by draw_drop_path, or handed in as forward(x, drop_path=factors)."""

    def __init__(self, spec: SwinV2Spec, device=None, backend: Optional[_lib.Backend] = None, seed: Optional[int] = None, operand: str = "bf16", drop_path_rate: float = 0.0):
        super().__init__()
        if operand not in OPERANDS:
            raise ValueError(f"operand must be 'bf16' or 'fp16', got {operand!r}")
        self.spec, self.operand, self.drop_path_rate = spec, operand, float(drop_path_rate)
        self.be = backend or _lib.load()
        dt = self.dt = OPERANDS[operand]
        dev = device if device is not None else ("cuda" if self.be.device_only else "cpu")
        if seed is not None:
            torch.manual_seed(seed)
        self.num_classes = spec.num_classes
        self.patch_embed = _Holder()
        self.patch_embed.proj = nn.Conv2d(spec.in_chans, spec.embed_dim, 4, 4, device=dev)
        self.patch_embed.norm = nn.LayerNorm(spec.embed_dim, eps=spec.ln_eps, device=dev)
        res = spec.img_size // 4
        layers, dim_in = [], spec.embed_dim
        for i, (d, h) in enumerate(zip(spec.depths, spec.heads)):
            dim = spec.embed_dim * 2 ** i
            if dim // h != 32 or dim % h:
                raise ValueError("the cosine window attention kernels are built for head dim 32 (every timm swinv2_*_window8_256)")
            if i > 0:
                res //= 2
            layers.append(SwinV2Stage(dim_in, dim, res, d, h, i > 0, spec.ln_eps, self.be, dt, dev))
            dim_in = dim
        self.layers = nn.Sequential(*layers)
        self.norm = nn.LayerNorm(dim_in, eps=spec.ln_eps, device=dev)
        self.num_features = dim_in
        self.head = _Holder()
        self.head.fc = nn.Linear(dim_in, spec.num_classes, device=dev) if spec.num_classes > 0 else nn.Identity()
        self.reset_parameters()

    def reset_parameters(self):
        """timm's init with `_init_respostnorm` (norm1 / norm2 weight and bias of every block 0), then the reference's override (classify_model.py:70-81): N(0, 0.02) for
        every Conv2d / Linear weight, zeros for Linear biases -- the cpb_mlp Linears included; LayerNorms, q_bias, v_bias and logit_scale are left alone"""
        for stage in self.layers:
            for blk in stage.blocks:
                for nrm in (blk.norm1, blk.norm2):
                    nn.init.zeros_(nrm.weight)
                    nn.init.zeros_(nrm.bias)
        _init_conv_linear(self)

    def draw_drop_path(self, batch: int) -> Optional[torch.Tensor]:
        """factors f32 [2 * blocks, batch] = Bernoulli(keep) / keep per (branch, sample), as timm's drop_path(); block j's rate is linspace(0, drop_path_rate, blocks)[j],
        the same for its two branches.  None when drop_path_rate == 0."""
        if self.drop_path_rate <= 0.0:
            return None
        dev = self.norm.weight.device
        keep = (1.0 - torch.linspace(0, self.drop_path_rate, sum(self.spec.depths), device=dev).repeat_interleave(2)).unsqueeze(1)
        return torch.where(torch.rand((keep.shape[0], batch), device=dev) < keep, 1.0 / keep, torch.zeros((), device=dev)).contiguous()

    def forward_features(self, x: torch.Tensor, drop_path: Optional[torch.Tensor] = None) -> torch.Tensor:
        s, be, dt = self.spec, self.be, self.dt
        check_image(x, s.in_chans, s.img_size)
        B = x.shape[0]
        if self.training:
            if drop_path is None:
                drop_path = self.draw_drop_path(B)
        elif drop_path is not None:
            raise ValueError("drop-path factors are for train() mode; eval() never drops a path")
        if drop_path is not None and tuple(drop_path.shape) != (2 * sum(s.depths), B):
            raise ValueError(f"drop_path must be [{2 * sum(s.depths)}, {B}]")
        g = s.img_size // 4
        pe = self.patch_embed
        y = _Lin.apply(_stem_patches(x), pe.proj.weight.view(s.embed_dim, -1), pe.proj.bias, None, dt, dt, be).float()
        y = _LN.apply(y.view(B, g, g, s.embed_dim), pe.norm.weight, pe.norm.bias, s.ln_eps, torch.float32, be)
        k = 0
        for stage in self.layers:
            y = stage.downsample(y)
            _, H, W, Cc = y.shape
            t = y.reshape(-1, Cc)
            for blk in stage.blocks:
                f1 = f2 = None
                if drop_path is not None:
                    f1, f2 = (drop_path[2 * k + j].to(torch.float32).repeat_interleave(H * W).unsqueeze(1) for j in (0, 1))
                t = blk.rows(t, B, f1, f2)
                k += 1
            y = t.view(B, H, W, Cc)
        return _LN.apply(y, self.norm.weight, self.norm.bias, s.ln_eps, torch.float32, be)

    def forward(self, x: torch.Tensor, drop_path: Optional[torch.Tensor] = None) -> torch.Tensor:
        f = self.forward_features(x, drop_path)
        if self.num_classes == 0:
            return f
        return _LinearFn.apply(_Pool.apply(f, self.be), self.head.fc.weight, self.head.fc.bias, self.be)


def create_model(name: str, pretrained: bool = False, num_classes: int = 1000, img_size: int = 256, device=None, backend=None, seed: Optional[int] = None,
                 operand: str = "bf16", drop_path_rate: float = 0.1, global_pool: Optional[str] = None, **kwargs) -> SwinTransformerV2:
    """timm.create_model for the served SwinV2 ids (a `timm-` prefix and a `.tag` suffix are accepted).  The window-16 ids (256-token windows) and
    `window12to16_192to256` (a non-zero pretrained window size) are not served: KeyError with the served list."""
    if kwargs:
        raise TypeError(f"swinv2.create_model: unsupported keyword arguments {sorted(kwargs)} (timm would act on them; this module does not build them)")
    arch = name[5:] if name.startswith("timm-") else name
    arch = arch.split(".")[0]
    if arch not in TIMM_SWINV2S:
        raise KeyError(f"'{name}': served SwinV2 ids are {sorted(TIMM_SWINV2S)} (8 x 8 windows, head dim 32); window16 / window12to16 ids are not built")
    if pretrained:
        raise RuntimeError("no network access: load a checkpoint with load_state_dict (timm's state_dict names)")
    if global_pool not in (None, "avg") and not (global_pool == "" and num_classes == 0):
        raise ValueError("global_pool: 'avg' (the family's default) or '' together with num_classes=0 (the NHWC feature map)")
    if img_size % 256:
        raise ValueError("the window8_256 family needs img_size % 256 == 0 (64 x 64 ... 8 x 8 maps of 8 x 8 windows)")
    spec = SwinV2Spec(img_size=img_size, num_classes=num_classes, **TIMM_SWINV2S[arch])
    return SwinTransformerV2(spec, device=device, backend=backend, seed=seed, operand=operand, drop_path_rate=drop_path_rate)
