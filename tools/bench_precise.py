"""Throughput and parity of the PRECISE (fp32-MFMA) forward beside the 16-bit training-path forward of the same engine: images/s of both, and the distance of both
from a CPU fp32 torch reference (4 images).  One JSON line.
usage: python tools/bench_precise.py [model id = vit_base_patch16_224 | swin_base_patch4_window7_224] [batch = 128] [timed calls = 3] [--no-parity]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from visiondk_amd import swin, vit

args = [a for a in sys.argv[1:] if not a.startswith("--")]
name = args[0] if len(args) > 0 else "vit_base_patch16_224"
B = int(args[1]) if len(args) > 1 else 128
calls = int(args[2]) if len(args) > 2 else 3
dev = torch.device("cuda:0")
if name in swin.TIMM_SWINS:
    from oracle.swin_ref import SwinTransformerRef as Ref
    model = swin.create_model(name, num_classes=1000, device=dev, seed=0, drop_path_rate=0.0)
    gflop = {"swin_base_patch4_window7_224": 15.47}.get(name)          # forward GFLOP per image (tools/bench_swin.py)
    ref_kw = dict(embed_dim=model.spec.embed_dim, depths=model.spec.depths, heads=model.spec.heads)
    fwd16 = lambda: model.engine.forward(x, training=False)
elif name in vit.TIMM_VITS:
    from oracle.vit_ref import VisionTransformerRef as Ref
    model = vit.create_model(name, num_classes=1000, device=dev)
    gflop = {"vit_base_patch16_224": 35.13}.get(name)
    ref_kw = None
    fwd16 = lambda: model.engine.forward(x)
else:
    raise SystemExit(f"unknown model id {name!r}")
model.eval()
g = torch.Generator(device="cpu"); g.manual_seed(0)
x = torch.randn(B, 3, 224, 224, generator=g).to(dev)
res = {"model": name, "batch": B, "operand": model.engine.operand}
for key, fn in (("forward_16bit", fwd16), ("forward_precise", lambda: model.engine.forward_precise(x))):
    fn(); torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    dt = (time.time() - t0) / calls
    res[key] = {"ms": dt * 1e3, "images_per_sec": B / dt}
    if gflop:
        res[key]["model_tflops"] = gflop * 1e9 * B / dt / 1e12
res["precise_over_16bit_time"] = res["forward_precise"]["ms"] / res["forward_16bit"]["ms"]
if "--no-parity" not in sys.argv:
    if ref_kw is None and name != "vit_base_patch16_224":
        raise SystemExit("parity: the ViT oracle of this tool is built at the B/16 shape (pass --no-parity)")
    ref = Ref(**ref_kw) if ref_kw else Ref()
    ref.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    ref.eval()
    with torch.no_grad():
        exp = ref(x[:4].cpu())
        rel = lambda a: ((a.double().cpu() - exp.double()).norm() / exp.double().norm()).item()
        res["rel_from_cpu_fp32_reference_4_images"] = {"forward_precise": rel(model.forward_precise(x[:4])), "forward_16bit": rel(model(x[:4]).detach())}
print(json.dumps(res))
