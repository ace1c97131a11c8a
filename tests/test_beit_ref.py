"""The CPU restatement of timm's BEiT (tests/beit_ref.py) pinned at fp32 against the independent transformers.BeitModel on both head paths, its relative position index
against transformers' generator, its state_dict names against timm's, and the biased attention node against plain autograd.

On the parent commit tests/beit_ref.py does not exist: the module's import fails and every test here with it."""
import pytest
import torch

from oracle import bf16ops
from tests import beit_ref
from tests.beit_ref import BeitRef

TINY = dict(img_size=96, dim=128, depth=2, heads=2)          # 6 x 6 patches + the class token = 37 tokens


def _hf_state_from_ref(ref, depth, mean_pool):
    """timm names -> transformers names: qkv split into q_proj / k_proj / v_proj (no k bias), attn.proj -> attention.o_proj, gamma_1 / gamma_2 -> lambda_1 / lambda_2,
    fc_norm -> pooler.layernorm (mean pooling) or norm -> layernorm (tokens)"""
    sd, out = ref.state_dict(), {}
    out["embeddings.cls_token"] = sd["cls_token"]
    out["embeddings.patch_embeddings.projection.weight"], out["embeddings.patch_embeddings.projection.bias"] = sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"]
    src, dst = ("fc_norm", "pooler.layernorm") if mean_pool else ("norm", "layernorm")
    out[dst + ".weight"], out[dst + ".bias"] = sd[src + ".weight"], sd[src + ".bias"]
    for i in range(depth):
        t, h = f"blocks.{i}.", f"layers.{i}."
        D = sd[t + "gamma_1"].numel()
        w = sd[t + "attn.qkv.weight"]
        for k, name in enumerate(("q_proj", "k_proj", "v_proj")):
            out[h + f"attention.{name}.weight"] = w[k * D:(k + 1) * D]
        out[h + "attention.q_proj.bias"], out[h + "attention.v_proj.bias"] = sd[t + "attn.q_bias"], sd[t + "attn.v_bias"]
        out[h + "relative_position_bias.relative_position_bias_table"] = sd[t + "attn.relative_position_bias_table"]
        for a, b in (("attn.proj", "attention.o_proj"), ("norm1", "layernorm_before"), ("norm2", "layernorm_after"), ("mlp.fc1", "mlp.fc1"), ("mlp.fc2", "mlp.fc2")):
            for leaf in ("weight", "bias"):
                out[h + b + "." + leaf] = sd[t + a + "." + leaf]
        out[h + "lambda_1"], out[h + "lambda_2"] = sd[t + "gamma_1"], sd[t + "gamma_2"]
    return out


def trained_like(model, seed=0):
    """weights as a trained checkpoint has them: LayerNorms and biases random, a non-zero table, gammas of order 0.1 - 1 with a random sign"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda p, s: (torch.randn(p.shape, generator=g) * s).to(p.device)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "norm" in n:
                p.copy_(rn(p, 0.3) + (1.0 if n.endswith("weight") else 0.0))
            elif "gamma_" in n:
                p.copy_(((0.1 + 0.9 * torch.rand(p.shape, generator=g)) * (torch.randint(0, 2, p.shape, generator=g) * 2.0 - 1.0)).to(p.device))
            elif n.endswith("relative_position_bias_table"):
                p.copy_(rn(p, 1.0))
            elif n == "cls_token":
                p.copy_(rn(p, 0.02))
            elif p.dim() == 1:
                p.copy_(rn(p, 0.1))


def _hf(transformers, mean_pool):
    cfg = transformers.BeitConfig(image_size=96, patch_size=16, num_channels=3, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512,
                                  hidden_act="gelu", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, drop_path_rate=0.0, use_relative_position_bias=True,
                                  use_shared_relative_position_bias=False, use_absolute_position_embeddings=False, use_mask_token=False, layer_scale_init_value=0.1,
                                  layer_norm_eps=1e-6, use_mean_pooling=mean_pool, attn_implementation="eager")
    return transformers.BeitModel(cfg).eval()


@pytest.mark.parametrize("mean_pool", [True, False], ids=["mean-pool", "tokens"])
def test_beit_restatement_matches_transformers(mean_pool):
    """fp32, random LayerNorms, q / v biases and tables, gammas in +-[0.1, 1].  Mean-pool path: fc_norm(mean of the patch tokens) against transformers' pooler_output;
    token path: norm over all tokens against last_hidden_state.  With every table zeroed in the restatement alone the same comparison is off by far more than 1e-3: the
    pin sees the bias."""
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(0)
    ref = BeitRef(num_classes=0, global_pool="avg" if mean_pool else "", **TINY).eval()
    trained_like(ref)
    hf = _hf(transformers, mean_pool)
    missing, unexpected = hf.load_state_dict(_hf_state_from_ref(ref, TINY["depth"], mean_pool), strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    x = torch.randn(2, 3, 96, 96)
    rel = lambda a, b: float((a - b).norm() / b.norm())
    with torch.no_grad():
        out = hf(pixel_values=x)
        want = out.pooler_output if mean_pool else out.last_hidden_state
        y = ref(x)
        assert tuple(y.shape) == tuple(want.shape) == ((2, 128) if mean_pool else (2, 37, 128))
        e = rel(y, want)
        print(f"beit restatement vs transformers ({'pooler_output' if mean_pool else 'last_hidden_state'}): {e:.2e}")
        assert e <= 1e-5
        for blk in ref.blocks:
            blk.attn.relative_position_bias_table.zero_()
        e0 = rel(ref(x), want)
        print(f"beit restatement with zero tables vs transformers: {e0:.2e}")
        assert e0 > 1e-3


def test_relative_position_index_matches_transformers():
    transformers = pytest.importorskip("transformers")
    from transformers.models.beit.modeling_beit import BeitRelativePositionBias
    assert torch.equal(BeitRelativePositionBias.generate_relative_position_index((6, 6)), beit_ref.relative_position_index(6))
    idx = beit_ref.relative_position_index(14)
    R = 27 * 27 + 3
    assert idx.shape == (197, 197) and int(idx.max()) == R - 1 and bool((idx[0, 1:] == R - 3).all()) and bool((idx[1:, 0] == R - 2).all()) and int(idx[0, 0]) == R - 1
    assert int(idx[1, 1]) == 13 * 27 + 13 and int(idx[1, 2]) == 13 * 27 + 12 and int(idx[1, 15]) == 12 * 27 + 13


def test_beit_base_names_and_shapes():
    """timm 0.9.16's state_dict of beit_base_patch16_224: no pos_embed, no qkv.bias, gamma_1 / gamma_2 on the block, one table of 732 rows per block, fc_norm and no norm
    with mean pooling; norm and no fc_norm on the token path"""
    with torch.device("meta"):
        ref = BeitRef(num_classes=37)
        tok = BeitRef(num_classes=0, global_pool="")
    got = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    D, M = 768, 3072
    want = {"cls_token": (1, 1, D), "patch_embed.proj.weight": (D, 3, 16, 16), "patch_embed.proj.bias": (D,), "fc_norm.weight": (D,), "fc_norm.bias": (D,),
            "head.weight": (37, D), "head.bias": (37,)}
    for i in range(12):
        b = f"blocks.{i}."
        want.update({b + "gamma_1": (D,), b + "gamma_2": (D,), b + "norm1.weight": (D,), b + "norm1.bias": (D,), b + "attn.q_bias": (D,), b + "attn.v_bias": (D,),
                     b + "attn.relative_position_bias_table": (732, 12), b + "attn.qkv.weight": (3 * D, D), b + "attn.proj.weight": (D, D), b + "attn.proj.bias": (D,),
                     b + "norm2.weight": (D,), b + "norm2.bias": (D,), b + "mlp.fc1.weight": (M, D), b + "mlp.fc1.bias": (M,), b + "mlp.fc2.weight": (D, M), b + "mlp.fc2.bias": (D,)})
    assert got == want, (sorted(set(got) ^ set(want))[:8], [k for k in want if k in got and got[k] != want[k]][:8])
    keys = set(tok.state_dict())
    assert "norm.weight" in keys and "norm.bias" in keys and not any(k.startswith(("fc_norm", "head")) for k in keys)
    small = BeitRef(num_classes=3, img_size=32, dim=64, depth=1, heads=1, init_values=1e-5)
    assert float(small.blocks[0].gamma_1.detach()[0]) == pytest.approx(1e-5, rel=1e-6) and float(small.blocks[0].attn.relative_position_bias_table.detach().abs().max()) == 0.0


def test_bias_attention_node_matches_autograd_in_fp32():
    """BiasAttention's hand-written backward (dq, dk, dv, d(bias)) against torch autograd through softmax(sc q k^T + bias) v, float64"""
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(2, 2, 37, 16, generator=g, dtype=torch.float64, requires_grad=True) for _ in range(3))
    bias = torch.randn(2, 37, 37, generator=g, dtype=torch.float64, requires_grad=True)
    dout = torch.randn(2, 2, 37, 16, generator=g, dtype=torch.float64)
    assert bf16ops.mode() == "fp32"
    beit_ref.BiasAttention.apply(q, k, v, bias, 0.25).backward(dout)
    got = [t.grad.clone() for t in (q, k, v, bias)]
    for t in (q, k, v, bias):
        t.grad = None
    (torch.softmax(0.25 * (q @ k.transpose(-2, -1)) + bias, -1) @ v).backward(dout)
    for a, t, name in zip(got, (q, k, v, bias), ("dq", "dk", "dv", "dbias")):
        assert float((a - t.grad).abs().max()) <= 1e-12 * max(1.0, float(t.grad.abs().max())), name
