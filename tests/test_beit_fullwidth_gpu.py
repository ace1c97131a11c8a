"""beit_base_patch16_224 at full width (dim 768, 12 heads, 197 tokens: the 7-tile instantiation of csrc/attention_bias.hip, twelve heads per image) on the device, 2 of its
12 blocks, fp16 operands, 2 images, against the fp32 restatement on the CPU: logits and the worst and the median parameter gradient at 1.5 x the fp16-operand restatement's
own deviation, computed here on the same weights and inputs (tests/test_dinov2_fullwidth_gpu.py's rule).  Weights as a trained checkpoint has them: non-zero tables.

On the parent commit visiondk_amd.beit and tests/beit_ref.py do not exist: the module's import fails and the test with it."""
import pytest
import torch

from oracle import bf16ops
from tests.beit_ref import BeitRef
from tests.test_beit import _rel
from tests.test_beit_ref import trained_like
from visiondk_amd import beit

SCALE = 1024.0
WIDTH = dict(img_size=224, num_classes=37, dim=768, depth=2, heads=12)


@pytest.mark.gpu
def test_beit_base_width_224_fp16_forward_backward_vs_restatement(hip):
    model = beit.Beit(beit.BeitSpec(**WIDTH), device="cuda:0", backend=hip, operand="fp16", seed=0)
    trained_like(model, seed=3)
    ref = BeitRef(**WIDTH)
    ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()}, strict=True)
    g = torch.Generator().manual_seed(1)
    x, t = torch.randn(2, 3, 224, 224, generator=g), torch.tensor([3, 30])

    def run(mode, scale):
        ref.zero_grad()
        with bf16ops.precision(mode):
            y = ref(x)
            (torch.nn.functional.cross_entropy(y, t) * scale).backward()
        return y.detach().clone(), {n: p.grad.detach().clone() / scale for n, p in ref.named_parameters()}

    y32, g32 = run("fp32", 1.0)
    y16, g16 = run("fp16_operands", SCALE)
    model.eval()
    y = model(x.cuda())
    (torch.nn.functional.cross_entropy(y, t.cuda()) * SCALE).backward()
    torch.cuda.synchronize()
    got = {n: p.grad.detach().cpu() / SCALE for n, p in model.named_parameters()}
    assert set(got) == set(g32)
    errs = sorted((_rel(got[n], g32[n]), n) for n in g32)
    floor = sorted((_rel(g16[n], g32[n]), n) for n in g32)
    res = {"logits": _rel(y.detach().cpu(), y32), "logits_floor": _rel(y16, y32), "worst_grad": errs[-1], "worst_grad_floor": floor[-1],
           "median_grad": errs[len(errs) // 2], "median_grad_floor": floor[len(floor) // 2]}
    print(res)
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    assert res["logits"] <= 1.5 * res["logits_floor"], res
    assert res["worst_grad"][0] <= 1.5 * res["worst_grad_floor"][0], res
    assert res["median_grad"][0] <= 1.5 * res["median_grad_floor"][0], res                     # (the worst alone would let every other gradient drift)
