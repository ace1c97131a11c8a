"""The ViT engine at head dim 72 (SigLIP SO400M/14: width 1152 = 16 heads x 72, MLP 4304, patch 14 on 224 px -> 256 tokens, no class token, global_pool='map') against
the fp32 oracle, on a small model of the same shape family: dim 144 = 2 heads x 72, MLP 528 = 16 * 33 (4304's divisibility: a multiple of 16 and of nothing larger),
patch 14 on 28 px (4 tokens) and, one block deep, on 224 px (256 tokens: the model's own sequence length)."""
import dataclasses

import pytest
import torch

from oracle.vit_ref import SiglipVisionTransformerRef, VisionTransformerRef, train_step_reference
from visiondk_amd import face, vit

SPEC = vit.VitSpec(img_size=28, patch_size=14, num_classes=10, dim=144, depth=2, heads=2, mlp_dim=528, class_token=False)      # hd 72, 4 tokens
SPEC256 = dataclasses.replace(SPEC, img_size=224, depth=1)                                                                       # hd 72, 256 tokens
SPECS = {"4tok": SPEC, "256tok": SPEC256}
ID = "vit_so400m_patch14_siglip_224"


def _rel(a, b):
    return ((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-30)).item()


def _map_ref(spec, seed=0):
    """the weight perturbation of tests/test_siglip.py's _pair: non-trivial biases / norms, block weights x 3 and pooling-head weights x 4 -> activations of O(1)"""
    torch.manual_seed(seed)
    ref = SiglipVisionTransformerRef(spec.img_size, spec.patch_size, 3, spec.num_classes, spec.dim, spec.depth, spec.heads, spec.mlp_dim)
    with torch.no_grad():
        for p in ref.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
        for blk in ref.blocks:
            for lin in (blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2):
                lin.weight.mul_(3.0)
        for lin in (ref.attn_pool.q, ref.attn_pool.kv, ref.attn_pool.proj, ref.attn_pool.mlp.fc1, ref.attn_pool.mlp.fc2):
            lin.weight.mul_(4.0)
    return ref


def _map_pair(be, dev, spec=SPEC, seed=0, operand="bf16"):
    ref = _map_ref(spec, seed)
    model = vit.VisionTransformerMap(spec, device=dev, backend=be, seed=1, operand=operand)
    model.load_state_dict({k: v.to(dev) for k, v in ref.state_dict().items()}, strict=True)
    return ref, model


@pytest.mark.parametrize("operand", ["bf16", "fp16"])
@pytest.mark.parametrize("which", ["4tok", "256tok"])
def test_hd72_map_forward_backward_vs_oracle(be, dev, which, operand):
    """VisionTransformerMap logits and EVERY gradient against SiglipVisionTransformerRef with the bounds of tests/test_siglip.py: bf16 2e-2 / 6e-2, fp16 under a loss
    scale of 1024 2.5e-3 / 8e-3"""
    spec = SPECS[which]
    ref, model = _map_pair(be, dev, spec, operand=operand)
    torch.manual_seed(3)
    B = 4 if which == "4tok" else 2
    x = torch.randn(B, 3, spec.img_size, spec.img_size); y = torch.randint(0, 10, (B,))
    S = 1024.0 if operand == "fp16" else 1.0
    lr = ref(x); torch.nn.functional.cross_entropy(lr, y).backward()
    lo = model(x.to(dev)); (torch.nn.functional.cross_entropy(lo, y.to(dev)) * S).backward()
    got = dict(model.named_parameters())
    for n, _ in ref.named_parameters():
        assert got[n].grad is not None, n
    worst = max(((_rel(got[n].grad / S, p.grad), n) for n, p in ref.named_parameters()))
    print(which, operand, "logits", _rel(lo.detach(), lr.detach()), "worst grad", worst)
    tol_l, tol_g = (2e-2, 6e-2) if operand == "bf16" else (2.5e-3, 8e-3)
    assert _rel(lo.detach(), lr.detach()) < tol_l
    assert worst[0] < tol_g, worst


def test_hd72_map_train_step_fp16_vs_reference_step(be, dev):
    """three MapTrainStep steps on fp16 operands under the loss scale against the fp32 reference step: the update bound of tests/test_siglip.py (8e-2 on each tensor's
    update, 1e-2 on the loss); no step is skipped"""
    ref, model = _map_pair(be, dev, seed=3, operand="fp16")
    hyp = dict(lr=0.05, momentum=0.9, weight_decay=5e-4)
    step = vit.MapTrainStep(model, label_smoothing=0.1, max_norm=10.0, ema=True, init_scale=1024.0, **hyp)
    init_sd = {n: p.detach().clone() for n, p in ref.named_parameters()}
    bufs = None
    torch.manual_seed(11)
    for it in range(3):
        x = torch.randn(4, 3, 28, 28); y = torch.randint(0, 10, (4,))
        _, loss_ref, _, _, bufs = train_step_reference(ref, x, y, label_smoothing=0.1, max_norm=10.0, momentum_bufs=bufs, updates=it, **hyp)
        step.step(x.to(dev), y.to(dev))
        assert abs(step.loss_value() - loss_ref.item()) < 1e-2 * abs(loss_ref.item()), (it, step.loss_value(), loss_ref.item())
    assert step.skipped_steps() == 0 and step.loss_scale() == 1024.0
    got = dict(model.named_parameters())
    for n, p in ref.named_parameters():      # the UPDATE each tensor received over the 3 steps
        assert _rel(got[n].detach().cpu() - init_sd[n], p.detach() - init_sd[n]) < 8e-2, n


def test_hd72_class_token_classifier_vs_oracle(be, dev):
    """a class-token classifier at dim 144 / 2 heads: vdk_attention_cls_serves answers false for 72, so the last block runs the full attention (the fallback from the
    class-query path).  bf16 bounds of tests/test_vit.py: logits 2e-2, loss 5e-3, every gradient 6e-2"""
    spec = dataclasses.replace(SPEC, class_token=True)
    torch.manual_seed(0)
    ref = VisionTransformerRef(spec.img_size, spec.patch_size, 3, spec.num_classes, spec.dim, spec.depth, spec.heads, spec.mlp_dim, eps=spec.ln_eps)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.05)
        ref.cls_token.add_(torch.randn_like(ref.cls_token) * 0.02)
        for blk in ref.blocks:
            for lin in (blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2):
                lin.weight.mul_(4.0)
    model = vit.VisionTransformer(spec, device=dev, backend=be, seed=1)
    model.load_state_dict(ref.state_dict(), strict=True)
    torch.manual_seed(5)
    x = torch.randn(3, 3, 28, 28); y = torch.randint(0, 10, (3,))
    logits_ref = ref(x); loss_ref = torch.nn.functional.cross_entropy(logits_ref, y, label_smoothing=0.05); loss_ref.backward()
    logits = model(x.to(dev)); loss = torch.nn.functional.cross_entropy(logits, y.to(dev), label_smoothing=0.05); loss.backward()
    errs = sorted((_rel(p.grad, pr.grad), n) for (n, p), (nr, pr) in zip(model.named_parameters(), ref.named_parameters()))
    print("class-token hd72: logits", _rel(logits, logits_ref), "worst grad", errs[-1])
    assert [n for n, _ in model.named_parameters()] == [n for n, _ in ref.named_parameters()]
    assert _rel(logits, logits_ref) < 2e-2
    assert abs(loss.item() - loss_ref.item()) < 5e-3 * abs(loss_ref.item())
    assert errs[-1][0] < 6e-2, errs[-1]


def _feature_pair(be, dev, spec, seed):
    fspec = dataclasses.replace(spec, num_classes=0)
    ref = _map_ref(dataclasses.replace(spec, num_classes=10), seed)
    model = vit.VisionTransformer(fspec, device=dev, backend=be, seed=1)
    model.load_state_dict({k: v for k, v in ref.state_dict().items() if not k.startswith(("head.", "attn_pool."))}, strict=True)
    return ref, model


def test_hd72_feature_mode_tokens(be, dev):
    """num_classes=0, global_pool='' (what the face / CBIR wrapper asks for): final-normed tokens [B, 4, 144] within the forward bound"""
    ref, model = _feature_pair(be, dev, SPEC, 4)
    torch.manual_seed(7)
    x = torch.randn(3, 3, 28, 28)
    with torch.no_grad():
        want = ref.forward_features(x)
        got = model(x.to(dev))
    assert tuple(got.shape) == (3, 4, 144)
    print("feature tokens", _rel(got, want))
    assert _rel(got, want) < 2e-2


@pytest.mark.parametrize("which", ["4tok", "256tok"])
def test_hd72_precise_forward_vs_oracle(be, dev, which):
    """forward_precise (fp32-MFMA contractions: q k^T over 72 columns, scale 72 ** -0.5, P V into 72 columns) on the patch-14 stem, read as it lies (588 = 4 * 147): the
    1e-4 bound of tests/test_vit_hd80.py"""
    spec = SPECS[which]
    ref, model = _feature_pair(be, dev, spec, 2)
    torch.manual_seed(6)
    x = torch.randn(2, 3, spec.img_size, spec.img_size)
    with torch.no_grad():
        want = ref.forward_features(x)
        got = model.forward_precise(x.to(dev))
    print(which, "precise tokens", _rel(got, want))
    assert got.shape == want.shape and _rel(got, want) < 1e-4


def test_so400m_id_resolves(be, dev):
    """`timm-vit_so400m_patch14_siglip_224` is a valid id for the classifier factory and for face.get_model's backbone.  The full model is 428 M parameters, too large to
    allocate here: the id table entry, and the models built around the id with the depth overridden to one block"""
    s = vit.spec_from_timm_name(ID, 0)
    assert (s.dim, s.depth, s.heads, s.mlp_dim, s.patch_size, s.class_token, s.img_size, s.ln_eps) == (1152, 27, 16, 4304, 14, False, 224, 1e-6)
    full = vit.TIMM_VITS[ID]
    vit.TIMM_VITS[ID] = dict(full, depth=1)
    try:
        m = vit.create_model(ID, num_classes=5, device=dev, backend=be)
        assert isinstance(m, vit.VisionTransformerMap) and m.engine.tokens == 256 and m.attn_pool.head_dim == 72 and m.attn_pool.scale == 72 ** -0.5
        del m
        cfg = {"task": "cbir", "image_size": 224, "backbone": {"timm-" + ID + ".webli": {"image_size": 224, "feat_dim": 64, "pretrained": False}},
               "head": {"arcface": {"feat_dim": 64, "num_class": 40, "margin_arc": 0.35, "margin_am": 0.0, "scale": 32}}}
        wrap = face.get_model(cfg, None, 0, backend=be, device=dev)
        bb = wrap.model.trainingwrapper["backbone"]
        assert bb.model.engine.tokens == 256 and bb.model.spec.dim == 1152 and bb.model.spec.heads == 16 and not bb.model.spec.class_token
        assert bb.output_layer[2].in_features == 256 * 1152
    finally:
        vit.TIMM_VITS[ID] = full


def test_oracle_at_head_dim_72_matches_transformers():
    """CPU only: oracle/vit_ref.SiglipVisionTransformerRef at hidden 144 / 2 heads / intermediate 528 against transformers.SiglipVisionModel (last_hidden_state and
    pooler_output, <= 1e-5), through the timm <- HF weight map of tests/test_oracle_vit.py::test_siglip_map_pool_ref_matches_transformers.  That map lives inside the test
    function there (it cannot be imported), so it is restated here for this width."""
    from transformers import SiglipVisionConfig, SiglipVisionModel
    torch.manual_seed(0)
    D, depth, heads, img, ps, mlp = 144, 2, 2, 28, 14, 528
    ref = SiglipVisionTransformerRef(img, ps, 3, 0, D, depth, heads, mlp_dim=mlp).eval()
    with torch.no_grad():
        for p in ref.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
    cfg = SiglipVisionConfig(hidden_size=D, intermediate_size=mlp, num_hidden_layers=depth, num_attention_heads=heads, image_size=img, patch_size=ps,
                             hidden_act="gelu", layer_norm_eps=1e-6, attention_dropout=0.0)
    hf = SiglipVisionModel(cfg).eval()
    sd, hsd = ref.state_dict(), hf.state_dict()
    pre = "vision_model." if any(k.startswith("vision_model.") for k in hsd) else ""

    def put(name, value):
        assert hsd[pre + name].shape == value.shape, (name, hsd[pre + name].shape, value.shape)
        hsd[pre + name] = value.clone()

    put("embeddings.patch_embedding.weight", sd["patch_embed.proj.weight"]); put("embeddings.patch_embedding.bias", sd["patch_embed.proj.bias"])
    put("embeddings.position_embedding.weight", sd["pos_embed"][0])
    for i in range(depth):
        w, b = sd[f"blocks.{i}.attn.qkv.weight"], sd[f"blocks.{i}.attn.qkv.bias"]
        for j, nm in enumerate(["q_proj", "k_proj", "v_proj"]):
            put(f"encoder.layers.{i}.self_attn.{nm}.weight", w[j * D:(j + 1) * D]); put(f"encoder.layers.{i}.self_attn.{nm}.bias", b[j * D:(j + 1) * D])
        for kind in ("weight", "bias"):
            put(f"encoder.layers.{i}.self_attn.out_proj.{kind}", sd[f"blocks.{i}.attn.proj.{kind}"])
            put(f"encoder.layers.{i}.layer_norm1.{kind}", sd[f"blocks.{i}.norm1.{kind}"]); put(f"encoder.layers.{i}.layer_norm2.{kind}", sd[f"blocks.{i}.norm2.{kind}"])
            put(f"encoder.layers.{i}.mlp.fc1.{kind}", sd[f"blocks.{i}.mlp.fc1.{kind}"]); put(f"encoder.layers.{i}.mlp.fc2.{kind}", sd[f"blocks.{i}.mlp.fc2.{kind}"])
    for kind in ("weight", "bias"):
        put(f"post_layernorm.{kind}", sd[f"norm.{kind}"])
        put(f"head.layernorm.{kind}", sd[f"attn_pool.norm.{kind}"])
        put(f"head.attention.out_proj.{kind}", sd[f"attn_pool.proj.{kind}"])
        put(f"head.mlp.fc1.{kind}", sd[f"attn_pool.mlp.fc1.{kind}"]); put(f"head.mlp.fc2.{kind}", sd[f"attn_pool.mlp.fc2.{kind}"])
    put("head.probe", sd["attn_pool.latent"])
    put("head.attention.in_proj_weight", torch.cat([sd["attn_pool.q.weight"], sd["attn_pool.kv.weight"]], 0))
    put("head.attention.in_proj_bias", torch.cat([sd["attn_pool.q.bias"], sd["attn_pool.kv.bias"]], 0))
    hf.load_state_dict(hsd)
    x = torch.randn(3, 3, img, img)
    with torch.no_grad():
        feats = ref.forward_features(x)
        pooled = ref.attn_pool(feats)
        out = hf(pixel_values=x)
    assert _rel(feats, out.last_hidden_state) <= 1e-5 and _rel(pooled, out.pooler_output) <= 1e-5
