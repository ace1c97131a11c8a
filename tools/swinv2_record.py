"""SwinV2 window8_256 (`swinv2_base_window8_256`: depths 2-2-18-2, heads 4-8-16-32, 64-token windows, cosine attention) at full size, for the record.
    python tools/swinv2_record.py parity                        # batch 2, fp16 operands, logits and every parameter gradient against the fp32 restatement on the CPU
    python tools/swinv2_record.py attn [--batch 64]             # per-launch time of the cosine forward / backward at swinv2_base's four stage geometries beside the 49-token
                                                                # kernels at swin_base's, same process, device events, alternating
    python tools/swinv2_record.py step [--batch 64] [--steps 5] # forward + backward of the module
Each mode prints JSON lines (profiles/swinv2_w8.jsonl)."""
import argparse
import ctypes as C
import json
import math
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from visiondk_amd import _lib, swinv2  # noqa: E402

NAME = "swinv2_base_window8_256"


def _rel(a, b):
    return ((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-30)).item()


def parity(args):
    from oracle import bf16ops
    from tests.swinv2_ref import SwinV2Ref
    from tests.test_swinv2 import _trained_like
    t0 = time.time()
    model = swinv2.create_model(NAME, num_classes=37, device="cuda:0", operand="fp16", drop_path_rate=0.0, seed=0)
    _trained_like(model, seed=3)
    with torch.no_grad():
        model.layers[1].blocks[0].attn.logit_scale[1] = math.log(10.0)
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
    units = {n + ".logit_scale": m.logit_scale_grad_scale() for n, m in ref.named_modules() if hasattr(m, "logit_scale_grad_scale")}
    y16, g16 = run("fp16_operands", 1024.0)
    y = model.eval()(x.cuda())
    (torch.nn.functional.cross_entropy(y, t.cuda()) * 1024.0).backward()
    torch.cuda.synchronize()
    got = {n: p.grad.detach().cpu() / 1024.0 for n, p in model.named_parameters()}
    # every parameter but the logit_scales relative to itself; a logit_scale gradient (one cancelling sum per head) in units of what went into it, tests/test_swinv2.py
    errs = sorted((_rel(got[n], g32[n]), n) for n in g32 if n not in units)
    floor = sorted((_rel(g16[n], g32[n]), n) for n in g32 if n not in units)
    in_units = lambda g, n: float((g[n] - g32[n]).double().norm() / units[n].double().norm())
    ls = max((in_units(got, n), n) for n in units)
    print(json.dumps({"mode": "parity", "model": NAME, "batch": 2, "operand": "fp16", "logits_rel": _rel(y, y32), "logits_rel_restatement16": _rel(y16, y32),
                      "worst_grad_rel": errs[-1][0], "worst_grad": errs[-1][1], "worst_grad_rel_restatement16": floor[-1][0], "median_grad_rel": errs[len(errs) // 2][0],
                      "median_grad_rel_restatement16": floor[len(floor) // 2][0], "grad_rel_covers": "every parameter except the logit_scales",
                      "worst_logit_scale_in_units": ls[0], "worst_logit_scale": ls[1], "worst_logit_scale_in_units_restatement16": max(in_units(g16, n) for n in units),
                      "worst_logit_scale_rel_to_itself": max(_rel(got[n], g32[n]) for n in units),
                      "meets_1e-3_5e-3": bool(_rel(y, y32) <= 1e-3 and errs[-1][0] <= 5e-3), "seconds": time.time() - t0}))


def _events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us per launch


def _attn_case(be, N, windows, H, nW, cos, dt=torch.float16):
    """-> (forward launcher, backward launcher) of one stage geometry on random data; rows in image order behind a random row index, a mask where the stage has one"""
    dev, Cc, T = "cuda", 32 * H, windows * N
    p = be.ptr
    qkv, do = torch.randn(T, 3 * Cc, device=dev).to(dt), torch.randn(T, Cc, device=dev).to(dt)
    o, dqkv, lse = torch.empty(T, Cc, device=dev, dtype=dt), torch.empty(T, 3 * Cc, device=dev, dtype=dt), torch.empty(windows, H, N, device=dev)
    bias, dbias = torch.randn(H, N, N, device=dev), torch.empty(H, N, N, device=dev)
    mask = torch.where(torch.rand(nW, N, N, device=dev) < 0.3, -100.0, 0.0).contiguous() if nW else None
    rowidx = torch.randperm(T, device=dev).to(torch.int32)
    tau, dtau = torch.full((H,), 10.0, device=dev), torch.empty(H, device=dev)
    need = C.c_size_t(0)
    lib = be.lib
    if cos:
        be.check(lib.vdk_wa_cos_bwd_workspace_bytes(windows, nW, H, C.byref(need)), "ws")
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        fwd = lambda: be.check(lib.vdk_wa_cos_fwd(p(qkv), 3 * Cc, p(o), Cc, p(lse), p(tau), p(bias), p(mask), nW, windows, H, p(rowidx), 1, p(ws), ws.numel(), be.stream()), "fwd")
        bwd = lambda: be.check(lib.vdk_wa_cos_bwd(p(qkv), 3 * Cc, p(o), p(do), Cc, p(lse), p(tau), p(bias), p(mask), nW, windows, H, p(rowidx), p(dqkv), 3 * Cc, p(dbias), p(dtau),
                                                  1, p(ws), ws.numel(), be.stream()), "bwd")
    else:                          # the public 49-token entries are bf16
        qkv, do, o, dqkv = (t.to(torch.bfloat16) for t in (qkv, do, o, dqkv))
        be.check(lib.vdk_window_attention_bwd_workspace_bytes(windows, nW, H, C.byref(need)), "ws")
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        sc = 32 ** -0.5
        fwd = lambda: be.check(lib.vdk_window_attention_fwd(p(qkv), 3 * Cc, p(o), Cc, p(lse), p(bias), p(mask), nW, windows, H, N, 32, sc, p(rowidx), p(ws), ws.numel(),
                                                            be.stream()), "fwd")
        bwd = lambda: be.check(lib.vdk_window_attention_bwd(p(qkv), 3 * Cc, p(o), p(do), Cc, p(lse), p(bias), p(mask), nW, windows, H, N, 32, sc, p(rowidx), p(dqkv), 3 * Cc,
                                                            p(dbias), p(ws), ws.numel(), be.stream()), "bwd")
    return fwd, bwd, (qkv, do, o, dqkv, lse, bias, dbias, mask, rowidx, tau, dtau, ws)


def attn(args):
    be = _lib.load()
    B = args.batch
    for stage, H in enumerate((4, 8, 16, 32)):
        res2, res1 = 64 >> stage, 56 >> stage                              # swinv2_base at 256: maps 64 .. 8 of 8 x 8 windows; swin_base at 224: maps 56 .. 7 of 7 x 7
        cases = {"cos64": _attn_case(be, 64, B * (res2 // 8) ** 2, H, (res2 // 8) ** 2 if res2 > 8 else 0, True),
                 "v1_49": _attn_case(be, 49, B * (res1 // 7) ** 2, H, (res1 // 7) ** 2 if res1 > 7 else 0, False)}
        for f, b, _ in cases.values():                                      # warm-up: code objects loaded, every shape seen
            for _ in range(3):
                f(); b()
        torch.cuda.synchronize()
        t = {k: {"fwd": [], "bwd": []} for k in cases}
        for _ in range(args.rounds):                                        # alternating, so that both families see the same machine
            for k, (f, b, _) in cases.items():
                t[k]["fwd"].append(_events(f, args.reps)); t[k]["bwd"].append(_events(b, args.reps))
        out = {"mode": "attn", "stage": stage, "batch": B, "heads": H, "reps": args.reps, "rounds": args.rounds}
        for k, n_tok, res, ws in (("cos64", 64, res2, 8), ("v1_49", 49, res1, 7)):
            items = B * (res // ws) ** 2 * H
            for d in ("fwd", "bwd"):
                best, worst = min(t[k][d]), max(t[k][d])
                out[f"{k}_{d}_us"], out[f"{k}_{d}_us_max"], out[f"{k}_{d}_ns_per_item"] = best, worst, best * 1e3 / items
            out[f"{k}_items"] = items
        print(json.dumps(out), flush=True)


def step(args):
    model = swinv2.create_model(NAME, num_classes=1000, device="cuda:0", operand=args.operand, drop_path_rate=0.1).train()
    torch.manual_seed(0)
    x = torch.randn(args.batch, 3, 256, 256, device="cuda"); y = torch.randint(0, 1000, (args.batch,), device="cuda")

    def one():
        model.zero_grad(set_to_none=True)
        (torch.nn.functional.cross_entropy(model(x), y) * 1024.0).backward()

    for _ in range(2):
        one()
    torch.cuda.synchronize()
    ms = _events(one, args.steps) / 1e3
    print(json.dumps({"mode": "step", "model": NAME, "what": "forward + backward of the autograd-node module (no optimizer)", "batch": args.batch, "operand": args.operand,
                      "steps": args.steps, "fwd_bwd_ms": ms, "img_per_s": args.batch / ms * 1e3}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("parity", "attn", "step"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200, help="attn: launches per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="attn: alternating windows per kernel family")
    ap.add_argument("--operand", default="fp16", choices=("fp16", "bf16"))
    a = ap.parse_args()
    {"parity": parity, "attn": attn, "step": step}[a.mode](a)
