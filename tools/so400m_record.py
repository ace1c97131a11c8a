"""SigLIP SO400M/14 (`vit_so400m_patch14_siglip_224`: 27 blocks of width 1152 = 16 heads x 72, MLP 4304, 256 tokens, attention-pool head) at full size, for the record.
    python tools/so400m_record.py parity [--depth K]      # batch 2, fp16 operands, logits and every parameter gradient against the fp32 oracle on the CPU
    python tools/so400m_record.py step [--batch 64] [--steps 10] [--operand fp16]      # one MapTrainStep's time (device events, after warm-up)
Each mode prints one JSON line."""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from visiondk_amd import vit  # noqa: E402

NAME = "vit_so400m_patch14_siglip_224"


def _rel(a, b):
    return ((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-30)).item()


def map_pair(be, dev, depth, classes=1000, seed=2, operand="fp16"):
    """the fp32 oracle of the model at `depth` blocks in the reference's initialisation, every bias / norm path carrying signal (oracle/parity.py's vit_pair for the
    class_token=False + global_pool='map' family), and the engine model on the same weights"""
    from oracle.vit_ref import SiglipVisionTransformerRef
    tv = vit.TIMM_VITS[NAME]
    torch.manual_seed(seed)
    ref = SiglipVisionTransformerRef(224, tv["patch_size"], 3, classes, tv["dim"], depth, tv["heads"], tv["mlp_dim"])
    with torch.no_grad():
        for p in ref.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.05)
    spec = vit.VitSpec(img_size=224, patch_size=tv["patch_size"], num_classes=classes, dim=tv["dim"], depth=depth, heads=tv["heads"], mlp_dim=tv["mlp_dim"], class_token=False)
    model = vit.VisionTransformerMap(spec, device=dev, backend=be, seed=1, operand=operand)
    model.load_state_dict({k: v.to(dev) for k, v in ref.state_dict().items()}, strict=True)
    return ref, model


def fwd_bwd_errors(ref, model, dev, seed=6, loss_scale=1024.0):
    """-> (logits error, sorted [(gradient error, parameter name)]) of one batch-2 forward + backward under the loss scale against the oracle"""
    torch.manual_seed(seed)
    x = torch.randn(2, 3, 224, 224); y = torch.randint(0, ref.head.out_features, (2,))
    lo = model(x.to(dev))
    (torch.nn.functional.cross_entropy(lo, y.to(dev), label_smoothing=0.05) * loss_scale).backward()
    lr = ref(x)
    torch.nn.functional.cross_entropy(lr, y, label_smoothing=0.05).backward()
    got = dict(model.named_parameters())
    errs = sorted((_rel(got[n].grad / loss_scale, p.grad), n) for n, p in ref.named_parameters())
    return _rel(lo, lr), errs


def parity(args):
    depth = args.depth or vit.TIMM_VITS[NAME]["depth"]
    t0 = time.time()
    ref, model = map_pair(None, "cuda:0", depth)
    lg, errs = fwd_bwd_errors(ref, model, "cuda:0")
    print(json.dumps({"model": NAME, "depth": depth, "batch": 2, "operand": "fp16", "logits_rel": lg, "worst_grad_rel": errs[-1][0], "worst_grad": errs[-1][1],
                      "median_grad_rel": errs[len(errs) // 2][0], "meets_1e-3_5e-3": bool(lg <= 1e-3 and errs[-1][0] <= 5e-3), "seconds": time.time() - t0}))


def step(args):
    model = vit.create_model(NAME, num_classes=1000, device="cuda:0", operand=args.operand)
    st = vit.MapTrainStep(model, lr=0.01, label_smoothing=0.05, ema=False)
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
    print(json.dumps({"model": NAME, "batch": args.batch, "operand": args.operand, "steps": args.steps, "step_ms": ms, "img_per_s": args.batch / ms * 1e3, "loss": st.loss_value(),
                      "skipped_steps": st.skipped_steps()}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("parity", "step"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--depth", type=int, default=0, help="parity: fewer blocks than the model's 27")
    ap.add_argument("--operand", default="fp16", choices=("fp16", "bf16"))
    a = ap.parse_args()
    {"parity": parity, "step": step}[a.mode](a)
