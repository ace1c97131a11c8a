"""ViT-H/14 CLIP at its real width and sequence length on the device: dim 1280 = 16 heads x 80, MLP 5120, patch 14 on 224 px (257 tokens), pre_norm, LayerNorm eps 1e-5,
1000 classes, fp16 operands -- against the fp32 oracle on the CPU.  Eight of the model's 32 blocks keep the oracle's CPU evaluation to seconds; the 32-block figure is
what `python tools/vit_huge_record.py parity` measures."""
import pytest
import torch

NORTH_STAR_LOGITS, NORTH_STAR_GRAD = 1e-3, 5e-3      # the project's stated tolerance (tests/test_fp16_operands.py), asserted literally


def _rel(a, b):
    return ((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-30)).item()


@pytest.mark.gpu
def test_vit_huge_patch14_width_fp16_operands_within_the_stated_tolerance(hip):
    from oracle.parity import vit_pair
    from visiondk_amd import vit
    tv = vit.TIMM_VITS["vit_huge_patch14_clip_224"]
    assert (tv["dim"], tv["heads"], tv["mlp_dim"], tv["patch_size"], tv["pre_norm"], tv["ln_eps"]) == (1280, 16, 5120, 14, True, 1e-5)      # the id table is what is tested
    ref, model = vit_pair(hip, "cuda:0", 224, tv["patch_size"], tv["dim"], 8, tv["heads"], tv["mlp_dim"], 1000, seed=2, operand="fp16", pre_norm=True, eps=tv["ln_eps"])
    assert model.engine.tokens == 257
    torch.manual_seed(6)
    x = torch.randn(2, 3, 224, 224); y = torch.randint(0, 1000, (2,))
    S = 1024.0
    lo = model(x.cuda()); lr = ref(x)
    (torch.nn.functional.cross_entropy(lo, y.cuda(), label_smoothing=0.05) * S).backward()
    torch.nn.functional.cross_entropy(lr, y, label_smoothing=0.05).backward()
    errs = sorted((_rel(p.grad / S, pr.grad), n) for (n, p), (_, pr) in zip(model.named_parameters(), ref.named_parameters()))
    print("vit_huge width, 8 blocks: logits", _rel(lo, lr), "worst gradients", errs[-3:], "median", errs[len(errs) // 2])
    assert _rel(lo, lr) <= NORTH_STAR_LOGITS and errs[-1][0] <= NORTH_STAR_GRAD, (_rel(lo, lr), errs[-1])
