"""DINOv2 ViT-L/14 (`vit_large_patch14_dinov2`: dim 1024, 24 blocks, 16 heads, img_size 518 = 1370 tokens, LayerScale) at full size, for the record.
    python tools/dinov2_record.py parity [--depth 24]          # batch 2, fp16 operands, logits and every parameter gradient against the fp32 restatement on the CPU
    python tools/dinov2_record.py ls                            # per-launch time of the two LayerScale residual kernels at 16 x 1370 and 64 x 1370 rows, C = 1024, against their
                                                                # byte counts and beside ops.cast_16 on the same tensor (same process, device events, medians of alternating windows)
    python tools/dinov2_record.py step [--steps 3]              # forward + backward of the module at the largest batch of {64, 32, 16} that fits, and the share of the two kernels
Each mode prints JSON lines (profiles/dinov2_l14.jsonl)."""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from visiondk_amd import _lib, dinov2, ops  # noqa: E402

NAME = "vit_large_patch14_dinov2"
TOKENS = 1370


def _rel(a, b):
    return ((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-30)).item()


def parity(args):
    from oracle import bf16ops
    from tests.dinov2_ref import Dinov2Ref
    from tests.test_dinov2 import _trained_like
    t0 = time.time()
    kw = dict(dinov2.TIMM_DINOV2S[NAME], img_size=518, num_classes=37, depth=args.depth)
    model = dinov2.DinoVisionTransformer(dinov2.Dinov2Spec(**kw), device="cuda:0", operand="fp16", seed=0)
    _trained_like(model, seed=3, keep=None)
    ref = Dinov2Ref(**kw)
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
    y16, g16 = run("fp16_operands", 1024.0)
    y = model.eval()(x.cuda())
    (torch.nn.functional.cross_entropy(y, t.cuda()) * 1024.0).backward()
    torch.cuda.synchronize()
    got = {n: p.grad.detach().cpu() / 1024.0 for n, p in model.named_parameters()}
    errs = sorted((_rel(got[n], g32[n]), n) for n in g32)
    floor = sorted((_rel(g16[n], g32[n]), n) for n in g32)
    print(json.dumps({"mode": "parity", "model": NAME, "depth": args.depth, "img_size": 518, "batch": 2, "operand": "fp16", "logits_rel": _rel(y, y32),
                      "logits_rel_restatement16": _rel(y16, y32), "worst_grad_rel": errs[-1][0], "worst_grad": errs[-1][1], "worst_grad_rel_restatement16": floor[-1][0],
                      "median_grad_rel": errs[len(errs) // 2][0], "median_grad_rel_restatement16": floor[len(floor) // 2][0],
                      "meets_1e-3_5e-3": bool(_rel(y, y32) <= 1e-3 and errs[-1][0] <= 5e-3), "seconds": time.time() - t0}))


def _events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us per launch


def _ls_case(be, rows, Cc, dt=torch.float16):
    """-> {name: launcher} on random data: the two kernels, and ops.cast_16 on the same [rows, C] f32 tensor (6 B / element: the library's plain streaming kernel)"""
    dev, p = "cuda", be.ptr
    x, dy = torch.randn(rows, Cc, device=dev), torch.randn(rows, Cc, device=dev)
    h = torch.randn(rows, Cc, device=dev).to(dt)
    y, dh = torch.empty_like(x), torch.empty_like(h)
    gamma, dg = torch.rand(Cc, device=dev), torch.empty(Cc, device=dev)
    need = C.c_size_t(0)
    be.check(be.lib.vdk_ls_residual_bwd_workspace_bytes(rows, Cc, C.byref(need)), "ws")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    out16 = torch.empty_like(h)
    cast = be.lib.vdk_cast_f32_f16 if dt == torch.float16 else be.lib.vdk_cast_f32_bf16
    opf = 1 if dt == torch.float16 else 0
    return {"fwd": lambda: be.check(be.lib.vdk_ls_residual_fwd(p(x), Cc, p(h), Cc, p(gamma), p(y), Cc, rows, Cc, opf, be.stream()), "fwd"),
            "bwd": lambda: be.check(be.lib.vdk_ls_residual_bwd(p(dy), Cc, p(h), Cc, p(gamma), p(dh), Cc, p(dg), rows, Cc, opf, p(ws), need.value, be.stream()), "bwd"),
            "cast_16": lambda: be.check(cast(p(x), p(out16), x.numel(), be.stream()), "cast")}, (x, dy, h, y, dh, gamma, dg, ws, out16)


BYTES = {"fwd": 10, "bwd": 8, "cast_16": 6}          # per element: x 4 + h 2 + y 4; dy 4 + h 2 + dh 2; in 4 + out 2


def ls(args):
    be = _lib.load()
    for B in (16, 64):
        rows, Cc = B * TOKENS, 1024
        fns, keep = _ls_case(be, rows, Cc)
        for f in fns.values():                                              # warm-up: code objects loaded
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(args.rounds):                                        # alternating windows, so that the three kernels see the same machine
            for k, f in fns.items():
                t[k].append(_events(f, args.reps))
        out = {"mode": "ls", "rows": rows, "C": Cc, "operand": "fp16", "reps": args.reps, "rounds": args.rounds,
               "note": "back-to-back launches on one set of tensors: at 16 x 1370 rows the working set (<= 224 MB) can stay in the 256 MB last-level cache"}
        for k, v in t.items():
            med = statistics.median(v)
            out[f"{k}_us"], out[f"{k}_us_min"], out[f"{k}_us_max"] = med, min(v), max(v)
            out[f"{k}_TBps"] = BYTES[k] * rows * Cc / med / 1e6
        out["fwd_over_cast"], out["bwd_over_cast"] = out["fwd_us"] / out["cast_16_us"], out["bwd_us"] / out["cast_16_us"]
        print(json.dumps(out), flush=True)


def step(args):
    be = _lib.load()
    torch.manual_seed(0)
    for batch in (64, 32, 16):
        model = None
        try:
            model = dinov2.create_model(NAME, num_classes=1000, img_size=518, device="cuda:0", operand=args.operand).train()
            x = torch.randn(batch, 3, 518, 518, device="cuda"); y = torch.randint(0, 1000, (batch,), device="cuda")

            def one():
                model.zero_grad(set_to_none=True)
                (torch.nn.functional.cross_entropy(model(x), y) * 1024.0).backward()

            for _ in range(2):
                one()
            torch.cuda.synchronize()
            ms = _events(one, args.steps) / 1e3
        except torch.OutOfMemoryError:
            del model
            torch.cuda.empty_cache()
            print(json.dumps({"mode": "step", "batch": batch, "fits": False}), flush=True)
            continue
        # the two kernels at this batch's row count, timed alone: 2 forward + 2 backward launches per block
        fns, keep = _ls_case(be, batch * TOKENS, 1024, torch.float16 if args.operand == "fp16" else torch.bfloat16)
        for f in fns.values():
            f()
        torch.cuda.synchronize()
        us = {k: statistics.median(_events(f, 50) for _ in range(3)) for k, f in fns.items()}
        ls_ms = 2 * 24 * (us["fwd"] + us["bwd"]) / 1e3
        print(json.dumps({"mode": "step", "model": NAME, "what": "forward + backward of the autograd-node module (no optimizer)", "img_size": 518, "batch": batch, "fits": True,
                          "operand": args.operand, "steps": args.steps, "fwd_bwd_ms": ms, "img_per_s": batch / ms * 1e3, "ls_fwd_us": us["fwd"], "ls_bwd_us": us["bwd"],
                          "ls_kernels_ms_per_step": ls_ms, "ls_share_of_step": ls_ms / ms}), flush=True)
        return


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("parity", "ls", "step"))
    ap.add_argument("--depth", type=int, default=24, help="parity: blocks (24 = the model)")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=100, help="ls: launches per timed window")
    ap.add_argument("--rounds", type=int, default=7, help="ls: alternating windows per kernel")
    ap.add_argument("--operand", default="fp16", choices=("fp16", "bf16"))
    a = ap.parse_args()
    {"parity": parity, "ls": ls, "step": step}[a.mode](a)
