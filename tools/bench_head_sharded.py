"""Class-sharded margin head (ArcFace) at ONE rank's share of BASELINE.json configs[2] on 8 GPUs: the 512 all-gathered embeddings of 512 dims against this rank's
125 000 of the 10^6 identities (c_base = 3 * 125 000, labels drawn over all 10^6 classes).  One process, no process group: `heads.sharded_margin_ce` with its
collectives skipped, i.e. the rank-local work of a step (normalisations, the cos GEMM, target cosine / statistics / gradient passes, the host-side merge, both
gradient GEMMs).  Four variants, all with cos_planes = 1 so that they multiply the same operand widths:
  bf16            bf16 operands, no loss scale: vdk_margin_stats / vdk_margin_grad (per-entry evaluation, expf) -- the yardstick
  bf16_scaled     bf16 operands under a loss scale: vdk_margin_stats_amp / vdk_margin_grad_amp (ArcFace once per row, v_exp_f32)
  fp16_scaled     fp16 operands under a loss scale: the same entries
  fp16_scaled_generic   the same with VDK_MARGIN_GENERIC=1 (per-entry evaluation)
Device events, two warm-up calls per variant, `calls` timed calls, the variants alternated inside one process, three rounds; one JSON object with the median and min / max
over the rounds of the ms per call, and the same for the two passes (statistics + gradient) alone on a fixed cosine matrix."""
import ctypes as C
import json
import os
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from visiondk_amd import _abi, _lib, heads  # noqa: E402

VARIANTS = {"bf16": ("bf16", False, "0"), "bf16_scaled": ("bf16", True, "0"), "fp16_scaled": ("fp16", True, "0"), "fp16_scaled_generic": ("fp16", True, "1")}


def _timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(calls):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    be = _lib.load()
    calls = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 20
    B, D, Cloc, Ctot = 512, 512, 125_000, 1_000_000
    c_base = 3 * Cloc
    torch.manual_seed(0)
    h = heads.ArcFace(D, 8, margin_arc=0.35, margin_am=0.0, scale=32, backend=be, device="cuda")      # the head's configuration; the weight is the shard below
    w = torch.empty(D, Cloc, device="cuda").uniform_(-1, 1).renorm_(2, 1, 1e-5).mul_(1e5)
    f = torch.randn(B, D, device="cuda"); y = torch.randint(0, Ctot, (B,), device="cuda")
    ls = torch.tensor([65536.0, 0.0, 0.0], device="cuda")

    def whole(operand, scaled):
        return lambda: heads.sharded_margin_ce(h, f, y, w, c_base, Ctot, cos_planes=1, operand=operand, loss_scale=ls if scaled else None)

    def passes(operand, scaled):
        dt = torch.float16 if operand == "fp16" else torch.bfloat16
        st = heads._forward_cos(be, f, w, 1, dtype=dt)
        gt = torch.empty(B, dtype=torch.float32, device="cuda")
        be.check(be.lib.vdk_margin_target_cos(be.ptr(st.cos), st.Cp, B, Cloc, c_base, be.ptr(y), be.ptr(gt), be.stream()), "vdk_margin_target_cos")
        stats = torch.empty((B, 4), dtype=torch.float32, device="cuda")
        dcos = torch.zeros((st.Bp, st.Cp), dtype=dt, device="cuda")
        cfg, cos = C.byref(h.cfg), st.cos
        # a fixed global max / sum stands in for the merged ones: the passes cost the same
        gmax = torch.full((B,), 32.0, dtype=torch.float32, device="cuda"); gsum = torch.full((B,), float(Ctot), dtype=torch.float32, device="cuda")
        if scaled or operand == "fp16":
            def run():
                be.check(be.lib.vdk_margin_stats_amp(cfg, be.ptr(cos), st.Cp, B, Cloc, c_base, be.ptr(y), be.ptr(gt), be.ptr(stats), be.stream()), "vdk_margin_stats_amp")
                be.check(be.lib.vdk_margin_grad_amp(cfg, be.ptr(cos), st.Cp, B, Cloc, c_base, Ctot, be.ptr(y), be.ptr(gt), be.ptr(gmax), be.ptr(gsum), 0.0, 1.0 / B,
                                                    be.ptr(ls), be.ptr(dcos), st.Cp, _abi.F16_ if operand == "fp16" else _abi.BF16, be.stream()), "vdk_margin_grad_amp")
        else:
            def run():
                be.check(be.lib.vdk_margin_stats(cfg, be.ptr(cos), st.Cp, B, Cloc, c_base, be.ptr(y), be.ptr(gt), be.ptr(stats), be.stream()), "vdk_margin_stats")
                be.check(be.lib.vdk_margin_grad(cfg, be.ptr(cos), st.Cp, B, Cloc, c_base, Ctot, be.ptr(y), be.ptr(gt), be.ptr(gmax), be.ptr(gsum), 0.0, 1.0 / B,
                                                be.ptr(dcos), st.Cp, be.stream()), "vdk_margin_grad")
        return run

    fns = {}
    for key, (operand, scaled, generic) in VARIANTS.items():
        fns[key] = (whole(operand, scaled), passes(operand, scaled), generic)
    ms = {k: [] for k in VARIANTS}; ms_p = {k: [] for k in VARIANTS}
    loss = {}
    for rnd in range(3):
        for key, (fn, fp, generic) in fns.items():
            os.environ["VDK_MARGIN_GENERIC"] = generic          # read by the library on every call
            for _ in range(2):
                out = fn(); fp()
            ms[key].append(_timed(fn, calls)); ms_p[key].append(_timed(fp, calls))
            loss[key] = out[0].mean().item()
            assert all(bool(torch.isfinite(t).all()) for t in out), key
    os.environ.pop("VDK_MARGIN_GENERIC", None)
    res = {"shape": {"B_total": B, "D": D, "C_local": Cloc, "num_class": Ctot, "c_base": c_base, "cos_planes": 1}, "calls_per_round": calls, "rounds": 3,
           "device": torch.cuda.get_device_name(0)}
    for key in VARIANTS:
        res[key] = {"ms_median": statistics.median(ms[key]), "ms_min": min(ms[key]), "ms_max": max(ms[key]),
                    "passes_ms_median": statistics.median(ms_p[key]), "passes_ms_min": min(ms_p[key]), "passes_ms_max": max(ms_p[key]), "loss": loss[key]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
