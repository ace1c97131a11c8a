"""The CPU restatement of timm's SwinV2 (tests/swinv2_ref.py) pinned against the independent transformers.Swinv2Model, and its state_dict names against timm's."""
import pytest
import torch

from tests.swinv2_ref import SwinV2Ref

TINY = dict(img_size=64, embed_dim=32, depths=(2, 2), heads=(1, 2))


def _hf_state_from_ref(ref, depths):
    """timm names -> transformers names.  qkv.weight and q_bias / v_bias split into query / key / value (key has no bias); cpb_mlp -> continuous_position_bias_mlp; norm1 /
    norm2 -> layernorm_before / layernorm_after (residual-post-norm: applied AFTER the branch in both); timm stage i + 1 STARTS with the downsample that transformers' stage
    i ENDS with."""
    sd, out = ref.state_dict(), {}
    out["embeddings.patch_embeddings.projection.weight"] = sd["patch_embed.proj.weight"]
    out["embeddings.patch_embeddings.projection.bias"] = sd["patch_embed.proj.bias"]
    out["embeddings.norm.weight"], out["embeddings.norm.bias"] = sd["patch_embed.norm.weight"], sd["patch_embed.norm.bias"]
    out["layernorm.weight"], out["layernorm.bias"] = sd["norm.weight"], sd["norm.bias"]
    for i, d in enumerate(depths):
        if i > 0:
            for leaf in ("reduction.weight", "norm.weight", "norm.bias"):
                out[f"encoder.layers.{i - 1}.downsample.{leaf}"] = sd[f"layers.{i}.downsample.{leaf}"]
        for j in range(d):
            t, h = f"layers.{i}.blocks.{j}.", f"encoder.layers.{i}.blocks.{j}."
            C = sd[t + "attn.q_bias"].numel()
            w = sd[t + "attn.qkv.weight"]
            out[h + "attention.self.query.weight"], out[h + "attention.self.key.weight"], out[h + "attention.self.value.weight"] = w[:C], w[C:2 * C], w[2 * C:]
            out[h + "attention.self.query.bias"], out[h + "attention.self.value.bias"] = sd[t + "attn.q_bias"], sd[t + "attn.v_bias"]
            out[h + "attention.self.logit_scale"] = sd[t + "attn.logit_scale"]
            for leaf in ("0.weight", "0.bias", "2.weight"):
                out[h + "attention.self.continuous_position_bias_mlp." + leaf] = sd[t + "attn.cpb_mlp." + leaf]
            for a, b in (("attn.proj", "attention.output.dense"), ("norm1", "layernorm_before"), ("mlp.fc1", "intermediate.dense"), ("mlp.fc2", "output.dense"),
                         ("norm2", "layernorm_after")):
                out[h + b + ".weight"], out[h + b + ".bias"] = sd[t + a + ".weight"], sd[t + a + ".bias"]
    return out


def test_swinv2_restatement_matches_transformers():
    """fp32, random non-zero LayerNorms (at the family's init every block is the identity), non-zero q_bias / v_bias, logit_scale spread with one head above the clamp.
    transformers adds the shift mask TWICE in the shifted block (-200 instead of -100: once in the layer, once in the attention); at this size exp(-100) relative to
    the row's other logits is already below fp32 resolution, so the outputs agree."""
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(0)
    ref = SwinV2Ref(num_classes=0, **TINY).eval()
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if "norm" in n:
                p.copy_(torch.randn_like(p) * 0.3 + (1.0 if n.endswith("weight") else 0.0))
            elif n.endswith("q_bias") or n.endswith("v_bias"):
                p.copy_(torch.randn_like(p) * 0.2)
            elif n.endswith("logit_scale"):
                p.copy_(torch.rand_like(p) * 1.8 + 1.6)
            elif "cpb_mlp" in n:
                p.copy_(torch.randn_like(p) * (1.0 if ".0." in n else 0.1))
            elif p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
        ref.layers[1].blocks[0].attn.logit_scale[1] = 5.0                       # > ln 100: clamped in both
    cfg = transformers.Swinv2Config(image_size=64, patch_size=4, num_channels=3, embed_dim=32, depths=[2, 2], num_heads=[1, 2], window_size=8, pretrained_window_sizes=[0, 0],
                                    mlp_ratio=4.0, qkv_bias=True, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, drop_path_rate=0.0, hidden_act="gelu",
                                    use_absolute_embeddings=False, layer_norm_eps=1e-5)
    hf = transformers.Swinv2Model(cfg, add_pooling_layer=True).eval()
    missing, unexpected = hf.load_state_dict(_hf_state_from_ref(ref, TINY["depths"]), strict=False)
    assert not unexpected, unexpected
    assert all(any(s in m for s in ("relative_position_index", "relative_coords_table", "attn_mask")) for m in missing), missing       # buffers only
    x = torch.randn(2, 3, 64, 64)
    with torch.no_grad():
        y = ref(x)                                   # [B, h, w, C]
        out = hf(pixel_values=x)
    B, h, w, C = y.shape
    rel = lambda a, b: float((a - b).norm() / b.norm())
    e_map, e_pool = rel(y.reshape(B, h * w, C), out.last_hidden_state), rel(y.mean((1, 2)), out.pooler_output)
    print(f"swinv2 restatement vs transformers: last_hidden_state {e_map:.2e}, pooled {e_pool:.2e}")
    assert e_map <= 1e-5 and e_pool <= 1e-5


def test_swinv2_base_names_and_shapes():
    """timm 0.9.16's state_dict of swinv2_base_window8_256: no k_bias, relative_coords_table, relative_position_index or attn_mask keys"""
    ref = SwinV2Ref(num_classes=37)
    got = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    want = {"patch_embed.proj.weight": (128, 3, 4, 4), "patch_embed.proj.bias": (128,), "patch_embed.norm.weight": (128,), "patch_embed.norm.bias": (128,),
            "norm.weight": (1024,), "norm.bias": (1024,), "head.fc.weight": (37, 1024), "head.fc.bias": (37,)}
    for i, (d, H) in enumerate(zip((2, 2, 18, 2), (4, 8, 16, 32))):
        C = 128 * 2 ** i
        if i > 0:
            want.update({f"layers.{i}.downsample.reduction.weight": (C, 2 * C), f"layers.{i}.downsample.norm.weight": (C,), f"layers.{i}.downsample.norm.bias": (C,)})
        for j in range(d):
            b = f"layers.{i}.blocks.{j}."
            want.update({b + "attn.logit_scale": (H, 1, 1), b + "attn.cpb_mlp.0.weight": (512, 2), b + "attn.cpb_mlp.0.bias": (512,), b + "attn.cpb_mlp.2.weight": (H, 512),
                         b + "attn.qkv.weight": (3 * C, C), b + "attn.q_bias": (C,), b + "attn.v_bias": (C,), b + "attn.proj.weight": (C, C), b + "attn.proj.bias": (C,),
                         b + "norm1.weight": (C,), b + "norm1.bias": (C,), b + "mlp.fc1.weight": (4 * C, C), b + "mlp.fc1.bias": (4 * C,), b + "mlp.fc2.weight": (C, 4 * C),
                         b + "mlp.fc2.bias": (C,), b + "norm2.weight": (C,), b + "norm2.bias": (C,)})
    assert got == want, (sorted(set(got) ^ set(want))[:8], [k for k in want if k in got and got[k] != want[k]][:8])
    assert not any(s in k for k in got for s in ("k_bias", "relative_coords_table", "relative_position_index", "attn_mask"))
    assert float(ref.layers[0].blocks[0].attn.logit_scale.detach()[0]) == pytest.approx(2.302585, abs=1e-5)
    assert all(float(p.detach().abs().max()) == 0.0 for n, p in ref.named_parameters() if ".norm1." in n or ".norm2." in n)                 # _init_respostnorm
    assert float(ref.layers[0].blocks[0].attn.relative_coords_table.abs().max()) == pytest.approx(3.169925 / 3.0, abs=1e-6)         # log2(7 / 7 * 8 + 1) / 3
