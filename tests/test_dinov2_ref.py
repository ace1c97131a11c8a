"""The CPU restatement of timm's DINOv2 ViTs (tests/dinov2_ref.py) pinned at fp32 against the independent transformers.Dinov2Model, and its state_dict names against timm's."""
import pytest
import torch

from tests.dinov2_ref import Dinov2Ref

TINY = dict(img_size=70, dim=128, depth=2, heads=2, mlp_dim=512)          # 5 x 5 patches + the class token = 26 tokens


def _hf_state_from_ref(ref, depth):
    """timm names -> transformers names: blocks.i.ls1.gamma -> encoder.layer.i.layer_scale1.lambda1, qkv split into query / key / value, attn.proj -> attention.output.dense"""
    sd, out = ref.state_dict(), {}
    out["embeddings.cls_token"], out["embeddings.position_embeddings"] = sd["cls_token"], sd["pos_embed"]
    out["embeddings.patch_embeddings.projection.weight"], out["embeddings.patch_embeddings.projection.bias"] = sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"]
    out["layernorm.weight"], out["layernorm.bias"] = sd["norm.weight"], sd["norm.bias"]
    for i in range(depth):
        t, h = f"blocks.{i}.", f"encoder.layer.{i}."
        D = sd[t + "ls1.gamma"].numel()
        for leaf in ("weight", "bias"):
            w = sd[t + "attn.qkv." + leaf]
            for k, name in enumerate(("query", "key", "value")):
                out[h + f"attention.attention.{name}.{leaf}"] = w[k * D:(k + 1) * D]
            for a, b in (("attn.proj", "attention.output.dense"), ("norm1", "norm1"), ("norm2", "norm2"), ("mlp.fc1", "mlp.fc1"), ("mlp.fc2", "mlp.fc2")):
                out[h + b + "." + leaf] = sd[t + a + "." + leaf]
        out[h + "layer_scale1.lambda1"], out[h + "layer_scale2.lambda1"] = sd[t + "ls1.gamma"], sd[t + "ls2.gamma"]
    return out


def _trained_like(ref, seed=0):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if "norm" in n:
                p.copy_(torch.randn(p.shape, generator=g) * 0.3 + (1.0 if n.endswith("weight") else 0.0))
            elif n.endswith(".gamma"):
                p.copy_((0.05 + 0.95 * torch.rand(p.shape, generator=g)) * (torch.randint(0, 2, p.shape, generator=g) * 2.0 - 1.0))
            elif n == "cls_token":
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
            elif p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=g) * 0.1)


def test_dinov2_restatement_matches_transformers():
    """fp32, random LayerNorms and biases, gammas in +-[0.05, 1], at the config's own image size (transformers' position interpolation is then the identity).  With every
    gamma replaced by 1 in the restatement alone the same comparison is off by far more than 1e-3: the pin sees the parameter."""
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(0)
    ref = Dinov2Ref(num_classes=0, global_pool="", **TINY).eval()
    _trained_like(ref)
    cfg = transformers.Dinov2Config(image_size=70, patch_size=14, num_channels=3, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, mlp_ratio=4, hidden_act="gelu",
                                    hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, drop_path_rate=0.0, layer_norm_eps=1e-6, qkv_bias=True, use_swiglu_ffn=False,
                                    layerscale_value=1.0)
    hf = transformers.Dinov2Model(cfg).eval()
    missing, unexpected = hf.load_state_dict(_hf_state_from_ref(ref, TINY["depth"]), strict=False)
    assert not unexpected, unexpected
    assert all("mask_token" in m for m in missing), missing          # (masked-image pre-training only; unused without bool_masked_pos)
    x = torch.randn(2, 3, 70, 70)
    rel = lambda a, b: float((a - b).norm() / b.norm())
    with torch.no_grad():
        out = hf(pixel_values=x)
        y = ref(x)                                                   # [B, 26, 128], normed
        assert tuple(y.shape) == (2, 26, 128) == tuple(out.last_hidden_state.shape)
        e_tok, e_pool = rel(y, out.last_hidden_state), rel(y[:, 0], out.pooler_output)
        print(f"dinov2 restatement vs transformers: last_hidden_state {e_tok:.2e}, pooler_output {e_pool:.2e}")
        assert e_tok <= 1e-5 and e_pool <= 1e-5
        for blk in ref.blocks:
            blk.ls1.gamma.fill_(1.0); blk.ls2.gamma.fill_(1.0)
        y1 = ref(x)
        o_tok, o_pool = rel(y1, out.last_hidden_state), rel(y1[:, 0], out.pooler_output)
        print(f"dinov2 restatement with gamma = 1 vs transformers: last_hidden_state {o_tok:.2e}, pooler_output {o_pool:.2e}")
        assert o_tok > 1e-3 and o_pool > 1e-3


def test_dinov2_large_names_and_shapes():
    """timm 0.9.16's state_dict of vit_large_patch14_dinov2 (img_size 518: 37 x 37 patches + the class token = 1370 positions; no register tokens, no fc_norm)"""
    with torch.device("meta"):
        ref = Dinov2Ref(num_classes=37)
    got = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    D, M = 1024, 4096
    want = {"cls_token": (1, 1, D), "pos_embed": (1, 1370, D), "patch_embed.proj.weight": (D, 3, 14, 14), "patch_embed.proj.bias": (D,), "norm.weight": (D,), "norm.bias": (D,),
            "head.weight": (37, D), "head.bias": (37,)}
    for i in range(24):
        b = f"blocks.{i}."
        want.update({b + "norm1.weight": (D,), b + "norm1.bias": (D,), b + "attn.qkv.weight": (3 * D, D), b + "attn.qkv.bias": (3 * D,), b + "attn.proj.weight": (D, D),
                     b + "attn.proj.bias": (D,), b + "ls1.gamma": (D,), b + "norm2.weight": (D,), b + "norm2.bias": (D,), b + "mlp.fc1.weight": (M, D), b + "mlp.fc1.bias": (M,),
                     b + "mlp.fc2.weight": (D, M), b + "mlp.fc2.bias": (D,), b + "ls2.gamma": (D,)})
    assert got == want, (sorted(set(got) ^ set(want))[:8], [k for k in want if k in got and got[k] != want[k]][:8])
    small = Dinov2Ref(num_classes=3, img_size=28, dim=64, depth=1, heads=1, mlp_dim=128)
    assert float(small.blocks[0].ls1.gamma.detach()[0]) == pytest.approx(1e-5, rel=1e-6) and float(small.blocks[0].ls2.gamma.detach().min()) == pytest.approx(1e-5, rel=1e-6)
