"""A/B timing of the attention kernels at the bench's geometry (ViT-B/16, batch 256: B*H = 3072 items of N = 197 tokens, head_dim 64).
    python tools/bench_attention.py [B N H] [--head-dim 64|72|80] [--dtype bf16|fp16]
head_dim 64 (default): per-call times of forward / backward for the short-sequence kernels (csrc/attention_small.hip) and the flash-style ones (csrc/attention.hip),
with the HBM floor of each (every operand / result once at 8 TB/s and at the 6.3 TB/s a copy kernel reaches).
head_dim 80: the streaming kernels of csrc/attention_hd.hip against their yardstick, the 64-wide streaming kernels of csrc/attention_long.hip forced at the same B, N, H
(VDK_ATTN_LONG_MIN=1), in one process, alternating rounds; FLOPs = 4 B H N^2 hd forward, 2.5 x that backward, so equal time per FLOP is parity (ratio 1.0).
head_dim 72: the 72-wide instance of csrc/attention_hd.hip, which the public entries refuse: called by raw ABI through the debug entries of csrc/vdk_internal.h, with
the 80-wide instance (same entries) and the 64-wide streaming kernels as further arms of the same alternating rounds.  The 72-wide kernels issue the MFMAs of the
80-wide ones and move 10 % fewer bytes: "vs_hd80" is their time over the 80-wide kernels' (<= 1 expected)."""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from visiondk_amd import _lib, ops  # noqa: E402


def _time(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def _raw_hd(be, a, H):
    """the arm's forward / backward through vdk_debug_attention_hd_* on preallocated results (no allocation inside the timed calls)"""
    qkv, dout, d = a["qkv"], a["dout"], a["d"]
    B, N, _ = qkv.shape
    D = H * d
    dt = 2 if qkv.dtype == torch.float16 else 0
    o = torch.empty((B, N, D), dtype=qkv.dtype, device="cuda"); lse = torch.empty((B, H, N), dtype=torch.float32, device="cuda")
    dqkv = torch.empty_like(qkv); dvec = torch.empty_like(lse)
    a["o"], a["lse"], a["keep"] = o, lse, (dqkv, dvec)
    p = lambda t: t.data_ptr()

    def fwd():
        be.check(be.lib.vdk_debug_attention_hd_fwd(p(qkv), 3 * D, p(o), D, p(lse), B, N, H, d, d ** -0.5, dt, be.stream()), "attention hd fwd")

    def bwd():
        be.check(be.lib.vdk_debug_attention_hd_bwd(p(qkv), 3 * D, p(o), p(dout), D, p(lse), p(dqkv), 3 * D, p(dvec), B, N, H, d, d ** -0.5, dt, be.stream()), "attention hd bwd")
    return fwd, bwd


def bench_hd(be, B, N, H, hd, dtype, rounds=7, iters=200):
    """-> {"hd80": {...}, "hd64_streaming": {...}, "time_per_flop_ratio": {...}} (hd 72: "hd72", "hd80" side by side and "vs_hd80" as well): medians over `rounds`
    alternating rounds of `iters` calls each"""
    arms = {}
    spec = ((f"hd{hd}", hd, None, False), ("hd64_streaming", 64, "1", False)) if hd == 80 else (("hd72", 72, None, True), ("hd80", 80, None, True), ("hd64_streaming", 64, "1", False))
    for name, d, env, raw in spec:
        torch.manual_seed(0)
        qkv = torch.randn(B, N, 3 * H * d, device="cuda").to(dtype)
        dout = torch.randn(B, N, H * d, device="cuda").to(dtype)
        arms[name] = dict(qkv=qkv, dout=dout, env=env, d=d, fwd=[], bwd=[])
        if raw:
            arms[name]["raw"] = _raw_hd(be, arms[name], H)

    def run(a, what):
        if a["env"] is not None:
            os.environ["VDK_ATTN_LONG_MIN"] = a["env"]
        try:
            if "raw" in a:
                f, b = a["raw"]
                if what == "prep":
                    f(); b(); torch.cuda.synchronize()
                else:
                    a[what].append(_time(f if what == "fwd" else b, iters))
            elif what == "prep":
                a["o"], a["lse"] = ops.attention_fwd(a["qkv"], H, backend=be)
                ops.attention_bwd(a["qkv"], a["o"], a["dout"], a["lse"], H, backend=be)
                torch.cuda.synchronize()
            elif what == "fwd":
                a["fwd"].append(_time(lambda: ops.attention_fwd(a["qkv"], H, backend=be), iters))
            else:
                a["bwd"].append(_time(lambda: ops.attention_bwd(a["qkv"], a["o"], a["dout"], a["lse"], H, backend=be), iters))
        finally:
            os.environ.pop("VDK_ATTN_LONG_MIN", None)

    for a in arms.values():
        run(a, "prep")
    for r in range(rounds + 1):                       # round 0 is the warm-up of every shape and is dropped
        for a in arms.values():
            run(a, "fwd"); run(a, "bwd")
    out = {}
    for name, a in arms.items():
        fl = 4.0 * B * H * N * N * a["d"]
        f, b = statistics.median(a["fwd"][1:]), statistics.median(a["bwd"][1:])
        out[name] = {"head_dim": a["d"], "fwd_us": f, "bwd_us": b, "fwd_us_min_max": [min(a["fwd"][1:]), max(a["fwd"][1:])], "bwd_us_min_max": [min(a["bwd"][1:]), max(a["bwd"][1:])],
                     "fwd_tflops": fl / (f * 1e-6) / 1e12, "bwd_tflops": 2.5 * fl / (b * 1e-6) / 1e12}
    n, y = out[f"hd{hd}"], out["hd64_streaming"]
    out["time_per_flop_ratio"] = {"fwd": y["fwd_tflops"] / n["fwd_tflops"], "bwd": y["bwd_tflops"] / n["bwd_tflops"]}      # > 1: the new kernels take longer per FLOP
    if hd == 72:
        out["vs_hd80"] = {"fwd": n["fwd_us"] / out["hd80"]["fwd_us"], "bwd": n["bwd_us"] / out["hd80"]["bwd_us"]}      # time over the 80-wide kernels' time: <= 1 expected
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", type=int, help="B N H")
    ap.add_argument("--head-dim", type=int, default=64, choices=(64, 72, 80))
    ap.add_argument("--dtype", default=None, choices=("bf16", "fp16"))
    args = ap.parse_args()
    assert len(args.shape) in (0, 3), "B N H"
    be = _lib.load()
    if args.head_dim != 64:
        B, N, H = args.shape or ((64, 256, 16) if args.head_dim == 72 else (64, 257, 16))      # SO400M/14 resp. ViT-H/14 at batch 64: B * H = 1024 items of 256 / 257 tokens
        dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}[args.dtype or "fp16"]
        out = {"B": B, "N": N, "H": H, "dtype": args.dtype or "fp16"}
        out.update(bench_hd(be, B, N, H, args.head_dim, dtype))
        print(json.dumps(out))
        return
    B, N, H = args.shape or (256, 197, 12)
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16}[args.dtype or "bf16"]
    D = H * 64
    torch.manual_seed(0)
    qkv = torch.randn(B, N, 3 * D, device="cuda").to(dt)
    dout = torch.randn(B, N, D, device="cuda").to(dt)
    out = {"B": B, "N": N, "H": H}
    for name, legacy in (("short_sequence", 0), ("flash_style", 1)):
        if legacy and dt != torch.bfloat16:
            continue                                  # the flash-style kernels are bf16 only
        be.lib.vdk_attention_force_legacy(legacy)
        o, lse = ops.attention_fwd(qkv, H, backend=be)
        d = ops.attention_bwd(qkv, o, dout, lse, H, backend=be)
        torch.cuda.synchronize()
        res = {}
        for what, fn in (("fwd", lambda: ops.attention_fwd(qkv, H, backend=be)), ("bwd", lambda: ops.attention_bwd(qkv, o, dout, lse, H, backend=be))):
            for _ in range(3):
                fn()
            res[what + "_us"] = _time(fn, 20)
        out[name] = res
    be.lib.vdk_attention_force_legacy(-1)
    tok = B * N * D * 2
    out["hbm_floor_us"] = {"fwd_bytes": 4 * tok, "bwd_bytes": 8 * tok, "fwd@8TB/s": 4 * tok / 8e6, "fwd@6.3TB/s": 4 * tok / 6.3e6, "bwd@8TB/s": 8 * tok / 8e6, "bwd@6.3TB/s": 8 * tok / 6.3e6}
    fl = 4.0 * B * H * N * N * 64
    out["tflops"] = {k: {"fwd": fl / (v["fwd_us"] * 1e-6) / 1e12, "bwd": 2.5 * fl / (v["bwd_us"] * 1e-6) / 1e12} for k, v in out.items() if isinstance(v, dict) and "fwd_us" in v}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
