"""BEiT-B/16 (`beit_base_patch16_224`: dim 768, 12 blocks, 12 heads, 197 tokens, relative position bias) at full size, for the record.  To be run on the MI355X.
    python tools/beit_record.py attn                          # time per launch of vdk_attention_bias_fwd / _bwd at B = 256, H = 12, N = 197, fp16, and in the same process the
                                                              # unbiased vdk_attention_fwd_dt / _bwd_dt at that shape (device events, medians of alternating windows)
    python tools/beit_record.py parity [--depth 12]           # batch 2, fp16 operands, logits and every parameter gradient against the fp32 restatement on the CPU
    python tools/beit_record.py step [--steps 3]              # forward + backward of the module at batch 64
Each mode prints JSON lines (profiles/beit_b16.jsonl).  No ratio is asserted anywhere: `attn` reports both times beside the byte ratios per item, which are derived ceilings
(forward 2.5: a 155 KB bias tile beside 101 KB of q, k, v, o; backward 3.3 with the per-workgroup d(bias) slab)."""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from visiondk_amd import _abi, _lib, beit  # noqa: E402

NAME = "beit_base_patch16_224"


def _rel(a, b):
    return ((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-30)).item()


def _events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us per launch


def attn(args):
    be = _lib.load()
    p, dev = be.ptr, "cuda"
    B, N, H, hd = args.batch, 197, 12, 64
    D, sc, dt = H * hd, hd ** -0.5, _abi.F16_
    g = torch.Generator(device="cpu").manual_seed(0)
    qkv = torch.randn(B, N, 3 * D, generator=g).to(torch.float16).to(dev)
    dout = torch.randn(B, N, D, generator=g).to(torch.float16).to(dev)
    bias = torch.randn(H, N, N, generator=g).to(dev)
    o, ob = torch.empty_like(dout), torch.empty_like(dout)
    lse, lseb = torch.empty(B, H, N, device=dev), torch.empty(B, H, N, device=dev)
    dqkv, dqkvb, dvec, dbias = torch.empty_like(qkv), torch.empty_like(qkv), torch.empty(B, H, N, device=dev), torch.empty_like(bias)
    nf, nb = C.c_size_t(0), C.c_size_t(0)
    be.check(be.lib.vdk_attention_bias_fwd_workspace_bytes(N, H, C.byref(nf)), "ws")
    be.check(be.lib.vdk_attention_bias_bwd_workspace_bytes(B, N, H, C.byref(nb)), "ws")
    wf, wb = torch.empty(nf.value, dtype=torch.uint8, device=dev), torch.empty(nb.value, dtype=torch.uint8, device=dev)
    fns = {
        "fwd": lambda: be.check(be.lib.vdk_attention_fwd_dt(p(qkv), 3 * D, p(o), D, p(lse), B, N, H, hd, sc, dt, be.stream()), "fwd"),
        "bias_fwd": lambda: be.check(be.lib.vdk_attention_bias_fwd(p(qkv), 3 * D, p(ob), D, p(lseb), p(bias), B, N, H, hd, sc, dt, p(wf), nf.value, be.stream()), "bias fwd"),
        "bwd": lambda: be.check(be.lib.vdk_attention_bwd_dt(p(qkv), 3 * D, p(o), p(dout), D, p(lse), p(dqkv), 3 * D, p(dvec), B, N, H, hd, sc, dt, be.stream()), "bwd"),
        "bias_bwd": lambda: be.check(be.lib.vdk_attention_bias_bwd(p(qkv), 3 * D, p(ob), p(dout), D, p(lseb), p(bias), p(dqkvb), 3 * D, p(dbias), B, N, H, hd, sc, dt, p(wb),
                                                                   nb.value, be.stream()), "bias bwd"),
    }
    for f in fns.values():                                              # warm-up: code objects loaded, every shape of the timed windows
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(args.rounds):                                        # alternating windows, so that the four see the same machine
        for k, f in fns.items():
            t[k].append(_events(f, args.reps))
    out = {"mode": "attn", "B": B, "N": N, "H": H, "head_dim": hd, "operand": "fp16", "reps": args.reps, "rounds": args.rounds, "fwd_workspace_bytes": nf.value,
           "bwd_workspace_bytes": nb.value, "bias_entries_include": "the prep kernel per call; the backward also its d(bias) reduction",
           "byte_ratio_ceiling_fwd": 2.5, "byte_ratio_ceiling_bwd": 3.3}
    for k, v in t.items():
        out[f"{k}_us"], out[f"{k}_us_min"], out[f"{k}_us_max"] = statistics.median(v), min(v), max(v)
    out["fwd_ratio"], out["bwd_ratio"] = out["bias_fwd_us"] / out["fwd_us"], out["bias_bwd_us"] / out["bwd_us"]
    print(json.dumps(out), flush=True)


def parity(args):
    from oracle import bf16ops
    from tests.beit_ref import BeitRef
    from tests.test_beit_ref import trained_like
    t0 = time.time()
    kw = dict(beit.TIMM_BEITS[NAME], img_size=224, num_classes=37, depth=args.depth)
    model = beit.Beit(beit.BeitSpec(**kw), device="cuda:0", operand="fp16", seed=0)
    trained_like(model, seed=3)
    ref = BeitRef(**kw)
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
    y16, g16 = run("fp16_operands", 1024.0)
    y = model.eval()(x.cuda())
    (torch.nn.functional.cross_entropy(y, t.cuda()) * 1024.0).backward()
    torch.cuda.synchronize()
    got = {n: p.grad.detach().cpu() / 1024.0 for n, p in model.named_parameters()}
    errs = sorted((_rel(got[n], g32[n]), n) for n in g32)
    floor = sorted((_rel(g16[n], g32[n]), n) for n in g32)
    tables = [n for n in g32 if n.endswith("relative_position_bias_table")]
    print(json.dumps({"mode": "parity", "model": NAME, "depth": args.depth, "img_size": 224, "batch": 2, "operand": "fp16", "logits_rel": _rel(y, y32),
                      "logits_rel_restatement16": _rel(y16, y32), "worst_grad_rel": errs[-1][0], "worst_grad": errs[-1][1], "worst_grad_rel_restatement16": floor[-1][0],
                      "median_grad_rel": errs[len(errs) // 2][0], "median_grad_rel_restatement16": floor[len(floor) // 2][0],
                      "worst_table_grad_rel": max(_rel(got[n], g32[n]) for n in tables), "worst_table_grad_rel_restatement16": max(_rel(g16[n], g32[n]) for n in tables),
                      "seconds": time.time() - t0}))


def step(args):
    torch.manual_seed(0)
    batch = args.batch_step
    model = beit.create_model(NAME, num_classes=1000, device="cuda:0", operand=args.operand).train()
    x = torch.randn(batch, 3, 224, 224, device="cuda"); y = torch.randint(0, 1000, (batch,), device="cuda")

    def one():
        model.zero_grad(set_to_none=True)
        (torch.nn.functional.cross_entropy(model(x), y) * 1024.0).backward()

    for _ in range(2):
        one()
    torch.cuda.synchronize()
    ms = statistics.median(_events(one, args.steps) / 1e3 for _ in range(3))
    print(json.dumps({"mode": "step", "model": NAME, "what": "forward + backward of the autograd-node module (no optimizer)", "img_size": 224, "batch": batch,
                      "operand": args.operand, "steps": args.steps, "fwd_bwd_ms": ms, "img_per_s": batch / ms * 1e3}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("parity", "step", "attn"))
    ap.add_argument("--depth", type=int, default=12, help="parity: blocks (12 = the model)")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256, help="attn: batch items")
    ap.add_argument("--batch-step", type=int, default=64, help="step: images")
    ap.add_argument("--reps", type=int, default=50, help="attn: launches per timed window")
    ap.add_argument("--rounds", type=int, default=7, help="attn: alternating windows per entry")
    ap.add_argument("--operand", default="fp16", choices=("fp16", "bf16"))
    a = ap.parse_args()
    {"parity": parity, "step": step, "attn": attn}[a.mode](a)
