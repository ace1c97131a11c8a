"""vit_large_patch14_dinov2 at full width (dim 1024, 16 heads, mlp 4096) and img_size 518 (1370 tokens: the streaming attention kernels, K = 588 patches) on the device, 4 of
the 24 blocks, fp16 operands, 2 images, against the fp32 restatement on the CPU: logits and the worst and the median parameter gradient at 1.5 x the fp16-operand
restatement's own deviation, computed here on the same weights and inputs (tests/test_swinv2_fullsize_gpu.py's rule).  The CPU restatement dominates the run time."""
import pytest
import torch

from oracle import bf16ops
from tests.dinov2_ref import Dinov2Ref
from tests.test_dinov2 import _rel, _trained_like
from visiondk_amd import dinov2

SCALE = 1024.0
WIDTH = dict(img_size=518, num_classes=37, dim=1024, depth=4, heads=16, mlp_dim=4096)


@pytest.mark.gpu
def test_dinov2_large_width_518_fp16_forward_backward_vs_restatement(hip):
    model = dinov2.DinoVisionTransformer(dinov2.Dinov2Spec(**WIDTH), device="cuda:0", backend=hip, operand="fp16", seed=0)
    _trained_like(model, seed=3, keep=None)
    ref = Dinov2Ref(**WIDTH)
    ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()}, strict=True)
    g = torch.Generator().manual_seed(1)
    x, t = torch.randn(2, 3, 518, 518, generator=g), torch.tensor([3, 30])

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
    print(f"north_star literal (logits 1e-3, gradients 5e-3): logits {'met' if res['logits'] <= 1e-3 else 'NOT met'}, worst gradient "
          f"{'met' if res['worst_grad'][0] <= 5e-3 else 'NOT met'} (not asserted until a recorded 24-block run shows margin)")
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    assert res["logits"] <= 1.5 * res["logits_floor"], res
    assert res["worst_grad"][0] <= 1.5 * res["worst_grad_floor"][0], res
    assert res["median_grad"][0] <= 1.5 * res["median_grad_floor"][0], res                     # (the worst alone would let every other gradient drift)
