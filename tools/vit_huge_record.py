"""ViT-H/14 CLIP (`vit_huge_patch14_clip_224`: 32 blocks of width 1280 = 16 heads x 80, 257 tokens) at full size, for the record.
    python tools/vit_huge_record.py parity            # batch 2, fp16 operands, logits and every parameter gradient against the fp32 oracle on the CPU
    python tools/vit_huge_record.py step [--batch 64] [--steps 10] [--operand fp16]      # one FusedTrainStep's time (device events, after warm-up)
Each mode prints one JSON line.  The kernel-trace share of attention comes from a separate profiler run of the `step` mode (tools/rocpd_stats.py)."""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from visiondk_amd import vit  # noqa: E402

NAME = "vit_huge_patch14_clip_224"


def _rel(a, b):
    return ((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-30)).item()


def parity(args):
    from oracle.parity import vit_pair
    tv = vit.TIMM_VITS[NAME]
    t0 = time.time()
    ref, model = vit_pair(None, "cuda:0", 224, tv["patch_size"], tv["dim"], args.depth or tv["depth"], tv["heads"], tv["mlp_dim"], 1000, seed=2, operand="fp16", pre_norm=True, eps=tv["ln_eps"])
    torch.manual_seed(6)
    x = torch.randn(2, 3, 224, 224); y = torch.randint(0, 1000, (2,))
    S = 1024.0
    lo = model(x.cuda())
    (torch.nn.functional.cross_entropy(lo, y.cuda(), label_smoothing=0.05) * S).backward()
    lr = ref(x)
    torch.nn.functional.cross_entropy(lr, y, label_smoothing=0.05).backward()
    errs = sorted((_rel(p.grad / S, pr.grad), n) for (n, p), (_, pr) in zip(model.named_parameters(), ref.named_parameters()))
    lg = _rel(lo, lr)
    print(json.dumps({"model": NAME, "depth": args.depth or tv["depth"], "batch": 2, "operand": "fp16", "logits_rel": lg, "worst_grad_rel": errs[-1][0], "worst_grad": errs[-1][1],
                      "median_grad_rel": errs[len(errs) // 2][0], "meets_1e-3_5e-3": bool(lg <= 1e-3 and errs[-1][0] <= 5e-3), "seconds": time.time() - t0}))


def step(args):
    model = vit.create_model(NAME, num_classes=1000, device="cuda:0", operand=args.operand)
    st = vit.FusedTrainStep(model, lr=0.01, label_smoothing=0.05, ema=False)
    torch.manual_seed(0)
    x = torch.randn(args.batch, 3, 224, 224, device="cuda"); y = torch.randint(0, 1000, (args.batch,), device="cuda")
    for _ in range(3):
        st.step(x, y)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
        st.step(x, y)
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / args.steps
    print(json.dumps({"model": NAME, "batch": args.batch, "operand": args.operand, "steps": args.steps, "step_ms": ms, "img_per_s": args.batch / ms * 1e3, "loss": st.loss_value()}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("parity", "step"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--depth", type=int, default=0, help="parity: fewer blocks than the model's 32")
    ap.add_argument("--operand", default="fp16", choices=("fp16", "bf16"))
    a = ap.parse_args()
    {"parity": parity, "step": step}[a.mode](a)
