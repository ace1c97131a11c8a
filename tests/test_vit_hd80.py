"""The ViT engine at head dim 80 (ViT-H/14 CLIP: width 1280 = 16 heads x 80, pre_norm, LayerNorm eps 1e-5, patch 14) against the fp32 oracle, on a small model of the
same shape family: dim 320 = 4 heads x 80, patch 14 on 28 px (5 tokens) and, one block deep, on 224 px (257 tokens: the model's own sequence length)."""
import dataclasses

import pytest
import torch

from oracle.vit_ref import VisionTransformerRef, train_step_reference
from visiondk_amd import face, vit

SPEC = vit.VitSpec(img_size=28, patch_size=14, num_classes=10, dim=320, depth=2, heads=4, mlp_dim=640, ln_eps=1e-5, pre_norm=True)      # hd 80, 5 tokens
SPEC257 = dataclasses.replace(SPEC, img_size=224, depth=1)                                                                                  # hd 80, 257 tokens
SPECS = {"5tok": SPEC, "257tok": SPEC257}


def _rel(a, b):
    return ((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-30)).item()


def _ref(spec, seed):
    """the weight perturbation of tests/test_vit.py's _pair: non-trivial biases / norms / cls so every gradient path is exercised, block weights x 4 -> activations of O(1)"""
    torch.manual_seed(seed)
    ref = VisionTransformerRef(spec.img_size, spec.patch_size, 3, max(spec.num_classes, 1), spec.dim, spec.depth, spec.heads, spec.mlp_dim, eps=spec.ln_eps, pre_norm=spec.pre_norm)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.05)
        ref.cls_token.add_(torch.randn_like(ref.cls_token) * 0.02)
        for blk in ref.blocks:
            for lin in (blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2):
                lin.weight.mul_(4.0)
    return ref


def _pair(be, dev, spec=SPEC, seed=0, operand="bf16"):
    ref = _ref(spec, seed)
    model = vit.VisionTransformer(spec, device=dev, backend=be, seed=1, operand=operand)
    model.load_state_dict(ref.state_dict(), strict=True)
    return ref, model


@pytest.mark.parametrize("operand", ["bf16", "fp16"])
@pytest.mark.parametrize("which", ["5tok", "257tok"])
def test_hd80_forward_backward_vs_oracle(be, dev, which, operand):
    """bf16: the bounds of tests/test_vit.py (logits 2e-2, loss 5e-3, every gradient 6e-2).  fp16 under a loss scale: the bounds tests/test_fp16_operands.py holds its small
    ViT to (logits 1e-3, loss 1e-4, every gradient 5e-3)."""
    spec = SPECS[which]
    ref, model = _pair(be, dev, spec, operand=operand)
    torch.manual_seed(5)
    B = 3 if which == "5tok" else 2
    x = torch.randn(B, 3, spec.img_size, spec.img_size); y = torch.randint(0, 10, (B,))
    S = 1024.0 if operand == "fp16" else 1.0
    logits_ref = ref(x)
    loss_ref = torch.nn.functional.cross_entropy(logits_ref, y, label_smoothing=0.05)
    loss_ref.backward()
    logits = model(x.to(dev))
    loss = torch.nn.functional.cross_entropy(logits, y.to(dev), label_smoothing=0.05)
    (loss * S).backward()
    tol_l, tol_loss, tol_g = (2e-2, 5e-3, 6e-2) if operand == "bf16" else (1e-3, 1e-4, 5e-3)
    errs = sorted((_rel(p.grad / S, pr.grad), n) for (n, p), (nr, pr) in zip(model.named_parameters(), ref.named_parameters()))
    print(which, operand, "logits", _rel(logits, logits_ref), "loss", abs(loss.item() - loss_ref.item()) / abs(loss_ref.item()), "worst grad", errs[-1])
    assert [n for n, _ in model.named_parameters()] == [n for n, _ in ref.named_parameters()]
    assert _rel(logits, logits_ref) < tol_l
    assert abs(loss.item() - loss_ref.item()) < tol_loss * abs(loss_ref.item())
    assert errs[-1][0] < tol_g, errs[-1]


def test_hd80_fused_step_fp16_vs_reference_step(be, dev):
    """three FusedTrainStep steps on fp16 operands under the loss scale against the fp32 reference step: the bounds of tests/test_vit.py::test_fused_step_vs_reference_step"""
    ref, model = _pair(be, dev, seed=3, operand="fp16")
    hyp = dict(lr=0.01, momentum=0.937, weight_decay=5e-4)
    step = vit.FusedTrainStep(model, label_smoothing=0.05, max_norm=10.0, ema=True, init_scale=1024.0, **hyp)
    ema_ref = {n: p.detach().clone() for n, p in ref.named_parameters()}
    init_sd = {n: p.detach().clone() for n, p in ref.named_parameters()}
    bufs = None
    torch.manual_seed(11)
    for it in range(3):
        x = torch.randn(4, 3, 28, 28); y = torch.randint(0, 10, (4,))
        _, loss_ref, _, _, bufs = train_step_reference(ref, x, y, label_smoothing=0.05, max_norm=10.0, momentum_bufs=bufs, ema=ema_ref, updates=it, **hyp)
        step.step(x.to(dev), y.to(dev))
        assert abs(step.loss_value() - loss_ref.item()) < 1e-2 * abs(loss_ref.item()), (it, step.loss_value(), loss_ref.item())
    assert step.skipped_steps() == 0 and step.loss_scale() == 1024.0
    sd = model.state_dict()
    for n, p in ref.named_parameters():      # the UPDATE each tensor received over the 3 steps
        assert _rel(sd[n].cpu() - init_sd[n], p.detach() - init_sd[n]) < 8e-2, n
    for n in ema_ref:
        assert _rel(model.engine.view(step.ema, n).cpu() - init_sd[n], ema_ref[n] - init_sd[n]) < 8e-2, n


def _precise_case(be, dev, spec):
    ref, model = _pair(be, dev, spec, seed=2)
    torch.manual_seed(6)
    x = torch.randn(2, 3, spec.img_size, spec.img_size)
    with torch.no_grad():
        want = ref(x)
        got = model.forward_precise(x.to(dev))
    print(spec.img_size, spec.patch_size, "precise logits", _rel(got, want))
    assert got.shape == want.shape and _rel(got, want) < 1e-4


# the same two models on patch 8 (16 px -> 5 tokens, 128 px -> 257 tokens): in_chans * 8 * 8 = 192 is a multiple of 8, the stem every other precise test uses
SPECS_P8 = {"5tok": dataclasses.replace(SPEC, img_size=16, patch_size=8), "257tok": dataclasses.replace(SPEC257, img_size=128, patch_size=8)}


@pytest.mark.parametrize("which", ["5tok", "257tok"])
def test_hd80_precise_forward_vs_oracle_patch8(be, dev, which):
    """forward_precise (fp32-MFMA contractions: q k^T over 80 columns, scale 80 ** -0.5, P V into 80 columns) at head dim 80: the bound of
    tests/test_precise.py::test_vit_logits_precise.  Measured on the CPU emulation: 1.1e-6 / 1.0e-6."""
    _precise_case(be, dev, SPECS_P8[which])


@pytest.mark.parametrize("which", ["5tok", "257tok"])
def test_hd80_precise_forward_vs_oracle(be, dev, which):
    """The same check on the patch-14 specs, i.e. on the real model's stem: in_chans * 14 * 14 = 588 is a multiple of 4 but not of 8.  At head dim 80 the fp32 path
    reads the patch rows and the [D, 588] weight as they lie (vdk_gemm_f32_nt needs K % 4); at head dim 64 it still refuses such a stem, which
    tests/test_vit.py::test_patch14_padded_operand_copies_vs_oracle pins.  Measured on the CPU emulation: 1.06e-6 (5 tokens) / 1.01e-6 (257 tokens)."""
    _precise_case(be, dev, SPECS[which])


def test_hd80_feature_mode_tokens(be, dev):
    """num_classes=0, global_pool='' (what the face / CBIR wrapper asks for): final-normed tokens [B, 5, 320] within the forward bound"""
    fspec = dataclasses.replace(SPEC, num_classes=0)
    ref = _ref(fspec, 4)
    model = vit.VisionTransformer(fspec, device=dev, backend=be, seed=1)
    model.load_state_dict({k: v for k, v in ref.state_dict().items() if not k.startswith("head.")}, strict=True)
    torch.manual_seed(7)
    x = torch.randn(3, 3, 28, 28)
    with torch.no_grad():
        want = ref.forward_features(x)
        got = model(x.to(dev))
    assert tuple(got.shape) == (3, 5, 320)
    print("feature tokens", _rel(got, want))
    assert _rel(got, want) < 2e-2


def test_vit_huge_id_resolves(be, dev):
    """`timm-vit_huge_patch14_clip_224` is a valid id for the classifier factory and for face.get_model's backbone.  The full model is 632 M parameters, too large to
    allocate here: the id table entry, and the wrapper built around the id with the depth overridden to one block"""
    s = vit.spec_from_timm_name("vit_huge_patch14_clip_224", 0)
    assert (s.dim, s.depth, s.heads, s.mlp_dim, s.patch_size, s.pre_norm, s.ln_eps, s.img_size) == (1280, 32, 16, 5120, 14, True, 1e-5, 224)
    full = vit.TIMM_VITS["vit_huge_patch14_clip_224"]
    vit.TIMM_VITS["vit_huge_patch14_clip_224"] = dict(full, depth=1)
    try:
        cfg = {"task": "cbir", "image_size": 224, "backbone": {"timm-vit_huge_patch14_clip_224.laion2b_ft_in12k_in1k": {"image_size": 224, "feat_dim": 64, "pretrained": False}},
               "head": {"arcface": {"feat_dim": 64, "num_class": 40, "margin_arc": 0.35, "margin_am": 0.0, "scale": 32}}}
        wrap = face.get_model(cfg, None, 0, backend=be, device=dev)
        bb = wrap.model.trainingwrapper["backbone"]
        assert bb.model.engine.tokens == 257 and bb.model.spec.dim == 1280 and bb.model.spec.heads == 16 and bb.model.spec.pre_norm
        assert bb.output_layer[2].in_features == 257 * 1280
    finally:
        vit.TIMM_VITS["vit_huge_patch14_clip_224"] = full
