"""swinv2_base_window8_256 at full width and depth on the device (fp16 operands, 2 images) against the fp32 restatement on the CPU: logits and the worst parameter
and the median parameter gradient, and every block's logit_scale gradient by name in units of what went into it, at 1.5 x the fp16-operand restatement's own deviation,
computed here on the same weights and inputs.  The CPU restatement dominates the run time."""
import math

import pytest
import torch

from oracle import bf16ops
from tests.swinv2_ref import SwinV2Ref
from tests.test_swinv2 import _rel, _trained_like
from visiondk_amd import swinv2

SCALE = 1024.0


@pytest.mark.gpu
def test_swinv2_base_full_size_fp16_forward_backward_vs_restatement(hip):
    model = swinv2.create_model("swinv2_base_window8_256", num_classes=37, device="cuda:0", backend=hip, operand="fp16", drop_path_rate=0.0, seed=0)
    _trained_like(model, seed=3)
    with torch.no_grad():
        model.layers[1].blocks[0].attn.logit_scale[1] = math.log(10.0)          # (_trained_like's clamped head belongs to the tiny model; here every head is live)
    ref = SwinV2Ref(num_classes=37)
    ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()}, strict=True)
    g = torch.Generator().manual_seed(1)
    x, t = torch.randn(2, 3, 256, 256, generator=g), torch.tensor([3, 30])

    def run(mode, scale):
        ref.zero_grad()
        with bf16ops.precision(mode):
            y = ref(x)
            (torch.nn.functional.cross_entropy(y, t) * scale).backward()
        return y.detach().clone(), {n: p.grad.detach().clone() / scale for n, p in ref.named_parameters()}

    y32, g32 = run("fp32", 1.0)
    units = {n + ".logit_scale": m.logit_scale_grad_scale() for n, m in ref.named_modules() if hasattr(m, "logit_scale_grad_scale")}      # of the fp32 run (loss scale 1)
    y16, g16 = run("fp16_operands", SCALE)
    model.eval()
    y = model(x.cuda())
    (torch.nn.functional.cross_entropy(y, t.cuda()) * SCALE).backward()
    torch.cuda.synchronize()
    got = {n: p.grad.detach().cpu() / SCALE for n, p in model.named_parameters()}
    # logit_scale gradients, by name, in units of what went into them (tests/test_swinv2.py): each block against 1.5 x the restatement's worst block
    in_units = lambda g, n: float((g[n] - g32[n]).double().norm() / units[n].double().norm())
    ls_e, ls_f = {n: in_units(got, n) for n in units}, {n: in_units(g16, n) for n in units}
    names = [n for n in g32 if n not in units]
    errs = sorted((_rel(got[n], g32[n]), n) for n in names)
    floor = sorted((_rel(g16[n], g32[n]), n) for n in names)
    res = {"logits": _rel(y.detach().cpu(), y32), "logits_floor": _rel(y16, y32), "worst_grad": errs[-1], "worst_grad_floor": floor[-1],
           "median_grad": errs[len(errs) // 2], "median_grad_floor": floor[len(floor) // 2],
           "worst_logit_scale_in_units": max((e, n) for n, e in ls_e.items()), "worst_logit_scale_in_units_floor": max((e, n) for n, e in ls_f.items())}
    print(res)
    print(f"north_star literal (logits 1e-3, gradients 5e-3): logits {'met' if res['logits'] <= 1e-3 else 'NOT met'}, worst gradient "
          f"{'met' if res['worst_grad'][0] <= 5e-3 else 'NOT met'} (not asserted until a recorded run shows margin)")
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    assert res["logits"] <= 1.5 * res["logits_floor"], res
    assert res["worst_grad"][0] <= 1.5 * res["worst_grad_floor"][0], res
    assert res["median_grad"][0] <= 1.5 * res["median_grad_floor"][0], res                     # (the worst alone would let every other gradient drift)
    for n, e in ls_e.items():
        assert e <= 1.5 * res["worst_logit_scale_in_units_floor"][0], (n, e, res)
