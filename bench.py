#!/usr/bin/env python
"""bench.py — BASELINE.json's headline metric on MI355X.

    python bench.py --gpus N --steps K --warmup W
    (N > 1: either under a launcher -- python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N ... --
     or bare: with WORLD_SIZE unset, `python bench.py --gpus N` starts its N ranks itself)

Workload (BASELINE.json configs[1]): ViT-B/16 classifier, 16-bit MFMA operands / fp32 accumulate + fp32 master weights,
synthetic ImageNet-1k 224x224, batch 256 PER GPU (weak scaling), one step = forward + CE(label_smoothing 0.05) +
backward + [RCCL all-reduce of the flat gradient, overlapped] + clip(10) + SGD(0.006, 0.937, 5e-4) + EMA (rank 0), i.e.
Trainer.compute_loss + Trainer.update of the reference (engine/procedure/train.py:177-215, configs/classification/pet.yaml).
Operand format (--operand): fp16 (default) is what the reference itself computes in on a GPU -- `torch.autocast(device_type=...)` without a dtype (train.py:118) is
float16, with the GradScaler of train.py:205-211, both done by the step -- and the format that meets north_star's "within 1e-3 of the reference"; bf16 is the format
BASELINE.json's configs[1] names.  Same MFMA rate, same bytes: the headline runs one, the other is timed beside it in the same line (`other_operand`).
Inputs are resident in HBM before the timed region.  Secondary metric (same JSON line, key "cbir"): CBIR query-pairs/s,
10k queries x 1M gallery, D=128, k=100 (configs[3] on one GPU; at N > 1 the gallery is row-sharded over the ranks, 125 k rows each at N = 8).

Prints ONE JSON line on rank 0 (driver contract).  A plain run does only what the headline needs: set up, W warm-up steps, K timed steps
(`ms_per_step` = their wall time / K), the outputs of the last step if --dump-outputs DIR is given, the line.  --full adds everything else,
as the default run did before the option existed: `roofline.dominant_kernel` (the 16-bit GEMM family, timed live with HIP events on its
launch stream inside the timed region -- the events cost the timed steps ~0.2 ms each), the parity legs, the other operand format,
`cpu_baseline` (the oracle restatement timed on the host cores, bounded sample), cfg5, swin, cfg3, the CBIR leg and, at N > 1, the sharded
search and the RCCL topology lines; the --no-* switches drop single legs of a --full run.

--dump-outputs DIR writes, after the timed steps, what the timed path handed its caller in the last step, from rank 0, as float32 .npy:
loss_rows (the per-image losses FusedTrainStep.step returns), params_sample / ema_sample (the flat fp32 master weights and the EMA weights
at a fixed, seeded sample of DUMP_SAMPLE positions) and, on fp16 operands, loss_state (GradScaler scale, growth tracker, skipped steps).
The inputs (weights, images, labels) are seeded: the same arguments give the same inputs on every run and every build.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

VIT_FLOP_PER_IMG = 105.38e9     # fwd+bwd, 2*MACs, attention included
PEAK_BF16_TFLOPS = 2500.0       # dense bf16 MFMA peak, MI355X_MICROARCH.md
PEAK_F32_MFMA_TFLOPS = 157.3
PEAK_HBM_GBS = 8000.0


def cpu_baseline_vit(seconds_budget: float = 25.0):
    """Oracle (plain-torch fp32 restatement of the reference's CPU path) fwd+bwd+SGD step, bounded sample."""
    from oracle.vit_ref import VisionTransformerRef, train_step_reference
    from oracle.cbir import usable_cores
    torch.manual_seed(2)
    cores = usable_cores()
    torch.set_num_threads(cores)
    bs = 32            # bs 32 (256 is about a minute per step on these cores), 1 warm-up + up to 3 timed steps
    model = VisionTransformerRef(224, 16, 3, 1000, 768, 12, 12)
    x = torch.randn(bs, 3, 224, 224)
    y = torch.randint(0, 1000, (bs,))
    bufs = None
    t0 = time.time()
    _, _, _, _, bufs = train_step_reference(model, x, y, lr=0.006, momentum=0.937, weight_decay=5e-4, label_smoothing=0.05, momentum_bufs=bufs)
    warm = time.time() - t0
    steps = max(1, min(3, int((seconds_budget - warm) / max(warm, 1e-3))))
    t0 = time.time()
    for _ in range(steps):
        train_step_reference(model, x, y, lr=0.006, momentum=0.937, weight_decay=5e-4, label_smoothing=0.05, momentum_bufs=bufs)
    dt = time.time() - t0
    return {"value": round(bs * steps / dt, 3), "unit": "images/sec", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"oracle/vit_ref.py ViT-B/16 fp32 fwd+bwd+clip+SGD, bs={bs}, {steps} step(s) after 1 warm-up, torch CPU"}


TOL_LOGITS, TOL_GRAD = 1e-3, 5e-3      # north_star: "logits/embeddings within 1e-3 rel of reference"; gradients 5e-3


def parity_vit(be, dev, operand="fp16"):
    """Full-size parity before timing: ViT-B/16 (BASELINE.json configs[1]) forward + backward at batch 8, the HIP engine in the given operand format against the fp32
    oracle (`vs_fp32`: the reference's PyTorch-CPU path restated -- the comparison north_star's tolerance is about, pass / fail printed) and against the oracle's
    16-bit-operand mode of the same format (o32 / o64 = float32 / float64 accumulation; `floor` = o32 vs o64, two valid evaluations of the same arithmetic).
    Independent arm: the same fp32 module under torch.autocast("cpu", that dtype).  Frobenius-relative errors, every parameter gradient."""
    from oracle.parity import vit_fwd_bwd_vs_oracle, vit_pair
    ref, model = vit_pair(be, dev, 224, 16, 768, 12, 12, 3072, 1000, seed=2, operand=operand)
    torch.manual_seed(6)
    x = torch.randn(8, 3, 224, 224); y = torch.randint(0, 1000, (8,))
    r = vit_fwd_bwd_vs_oracle(ref, model, x, y, dev)
    fl = r["floor_o32_vs_o64"]
    ok = all(r[s_]["logits"] <= 1.5 * fl["logits"] + 1e-5 and r[s_]["worst_grad"] <= 1.5 * fl["worst_grad"] + 1e-5 for s_ in ("vs_o32", "vs_o64"))
    out = {"config": "ViT-B/16 224 1000 classes, batch 8, forward + backward, every parameter gradient", "operand": operand, "loss_scale": r["loss_scale"],
           "tolerance_stated": {"logits_rel": TOL_LOGITS, "worst_grad_rel": TOL_GRAD, "against": "vs_fp32 (the reference's PyTorch-CPU fp32 path, oracle/vit_ref.py)"},
           "tolerance_met": bool(r["vs_fp32"]["logits"] <= TOL_LOGITS and r["vs_fp32"]["worst_grad"] <= TOL_GRAD), "within_1p5x_floor": ok}
    for k_, v_ in r.items():
        if isinstance(v_, dict):
            out[k_] = {"logits_rel": v_["logits"], "loss_rel": v_["loss"], "worst_grad_rel": v_["worst_grad"], "worst_grad": v_["worst_grad_name"]}
    del model, ref
    torch.cuda.empty_cache()
    return out


GEMM_EVENT_STRIDE = 4      # steps between two event-timed steps of the timed region
DUMP_SAMPLE = 1 << 22      # weight positions written by --dump-outputs (16 MB per array)


def pmc_traffic_per_launch():
    """HBM-side bytes per GEMM launch from the committed PMC passes of this same command (rocprofv3 cannot run inside the timed process):
    profiles/r0N_pmc_traffic.json is written by tools/pmc_traffic.py from two `rocprofv3 --kernel-trace --pmc {FETCH_SIZE|WRITE_SIZE}` runs,
    FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes for gfx950.  None if the artifact is absent."""
    for name in ("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json", "r01_pmc_traffic.json"):      # the newest round's passes of this command
        p = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", name)
        try:
            with open(p) as f:
                return json.load(f)["bytes_per_launch"]
        except (OSError, KeyError, ValueError):
            continue
    return None


def pmc_cbir():
    """L2 memory-side bytes of one search from the committed PMC passes of tools/pmc_cbir.py (None if absent)"""
    for name in ("r06_cbir_pmc.json", "r05_cbir_pmc.json", "r04_cbir_pmc.json", "r03_cbir_pmc.json", "r02_cbir_pmc.json"):
        p = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", name)
        try:
            with open(p) as f:
                return json.load(f)
        except (OSError, ValueError):
            continue
    return None


def bench_cbir(dev, nq=10000, n=1_000_000, d=128, k=100, iters=6, with_cpu=True):
    from visiondk_amd import cbir
    g = torch.Generator(device="cpu"); g.manual_seed(0)
    gal = cbir.l2_normalize(torch.randn(n, d, generator=g).to(dev))
    g.manual_seed(1)
    qry = cbir.l2_normalize(torch.randn(nq, d, generator=g).to(dev))

    def timed(method, storage="float32", optimistic=False, gal_=None, qry_=None, dim=d, small_lists=True):
        index = cbir.FlatIPIndex(dim, device=dev, method=method, storage=storage, optimistic=optimistic, small_lists=small_lists)
        index.add(gal if gal_ is None else gal_)
        qq = qry if qry_ is None else qry_
        for _ in range(4):           # warm-up: allocates the workspace, the prefilter path builds its bf16 gallery copy (add-time work); several searches because this
            s, i = index.search(qq, k)   # leg follows ~20 s of host-only work (cpu_baseline) and one 3.5 ms search does not bring the clocks back up (measured 3.89 vs 3.54 ms)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            s, i = index.search(qq, k)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters, s, i, index.fallbacks

    ms, s, i, fb = timed("prefilter")                                  # default: 16 384-entry candidate lists (1.5 GB of workspace), overflow reported and repaired
    ms_gs, s_gs, i_gs, fb_s = timed("prefilter", small_lists=False)    # the guaranteed schedule alone: lists of cap entries (8.0 GB), no host read
    ms_g, s_g, i_g, fb_o = timed("prefilter", optimistic=True)      # bootstrap + two stages, overflow-checked (measured slower: more survivors per query)
    ms_scan, s_scan, i_scan, _ = timed("exact_scan")
    ms16, s16, i16, _ = timed("prefilter", storage="float16")      # faiss useFloat16 storage
    # the rate with the transfers the reference's loop pays (engine/cbir/evaluation.py:171-200: numpy queries in, numpy scores / indices out): wall clock
    # around cbir.search() on host arrays (H2D of the queries, D2H of scores and indices) -- reported beside `value`, never as it
    index = cbir.FlatIPIndex(d, device=dev)
    index.add(gal)
    q_host = qry.cpu().numpy()
    cbir.search(None, None, index, dev, None, k, 256, query_embeddings=q_host)      # warm-up at the same size: the workspace is keyed on it
    torch.cuda.synchronize(); t0 = time.time()
    s_h, i_h = cbir.search(None, None, index, dev, None, k, 256, query_embeddings=q_host)
    host_ms = (time.time() - t0) * 1e3
    pairs = nq * n / (ms * 1e-3)
    qb = 256
    alg_bytes = -(-nq // qb) * n * d * 4 + nq * d * 4 + nq * k * 12   # BASELINE.md §2 definition, qb=256, s_g=4
    alg16 = -(-nq // qb) * n * d * 2 + nq * d * 4 + nq * k * 12
    gbs = alg_bytes / (ms * 1e-3) / 1e9
    tf = 2.0 * nq * n * d / (ms * 1e-3) / 1e12
    tf_scan = 2.0 * nq * n * d / (ms_scan * 1e-3) / 1e12
    pmc = pmc_cbir()
    rep16 = cbir.fp16_swap_report(s.cpu().numpy(), i.cpu().numpy(), i16.cpu().numpy())
    out = {"metric": "CBIR query-pairs/sec (exact fp32 inner product + top-100)", "value": pairs, "unit": "pairs/sec",
           "ms_per_search": ms, "optimistic_fallbacks": fb, "value_incl_h2d_d2h": nq * n / (host_ms * 1e-3), "ms_incl_h2d_d2h": host_ms,
           "host_results_equal": bool((torch.from_numpy(i_h).to(i.device) == i).all()),
           "config": {"workload": f"cbir Q={nq} N={n} D={d} k={k} fp32 gallery, 1 GPU",
                      "method": "bf16-MFMA pre-filter (rigorous bound), threshold bootstrap, stages of cap - k rows ranked on the approximate scores (every row within 2 eps of the k-th best kept), exact fp32 fmaf-chain re-score + exact sort of the rows kept at the end (the kept set contains the exact top-k: bit-identical results)"},
           "dtype": "f32",
           # what binds: the scan is MFMA work on bf16 copies (2.56 TFLOP per search); the HBM figure is BASELINE.md §2's byte DEFINITION (the fp32 gallery re-streamed
           # once per 256-query batch like the reference's loop), which this kernel does not actually move -- `traffic` is the measured L2 memory-side byte count
           "roofline": {"bound": "mfma", "achieved": tf, "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": tf / PEAK_BF16_TFLOPS,
                        "mfma_frac": tf / PEAK_BF16_TFLOPS,
                        "counted_hbm_frac": None if pmc is None else pmc.get("bytes_per_search", 0) / (ms * 1e-3) / 1e9 / PEAK_HBM_GBS,
                        "traffic": None if pmc is None else pmc.get("bytes_per_search"),
                        "measured_traffic_GBps": None if pmc is None else pmc.get("bytes_per_search", 0) / (ms * 1e-3) / 1e9,
                        "note_hbm_by_baseline_definition": {"achieved": gbs, "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": gbs / PEAK_HBM_GBS,
                                                            "note": f"NOT what the kernels move: BASELINE.md section 2's byte DEFINITION (the fp32 gallery re-streamed per {qb}-query batch like the reference's loop, {alg_bytes / 1e9:.2f} GB per search); the search scans the gallery once per 16 384 queries -- counted bytes are `traffic`"},
                        "pmc": pmc},
           "workspace": "default: candidate lists of 16 384 entries per query (1.48 GB at 10 k queries); an overflow is reported by the kernels and repaired with the guaranteed schedule (one flag read per search)",
           "guaranteed_schedule_only": {"ms_per_search": ms_gs, "value": nq * n / (ms_gs * 1e-3), "workspace_GB": 8.0, "fallbacks": fb_s,
                                        "note": "FlatIPIndex(small_lists=False): lists of cap = 98 304 entries, cannot overflow, no host read",
                                        "bit_equal": bool(torch.equal(i, i_gs) and torch.equal(s.view(torch.int32), s_gs.view(torch.int32)))},
           "optimistic_two_stage_schedule": {"ms_per_search": ms_g, "value": nq * n / (ms_g * 1e-3), "fallbacks": fb_o,
                                             "bit_equal": bool(torch.equal(i, i_g) and torch.equal(s.view(torch.int32), s_g.view(torch.int32)))},
           "float16_storage": {"ms_per_search": ms16, "value": nq * n / (ms16 * 1e-3),
                               "hbm_by_baseline_definition_frac": alg16 / (ms16 * 1e-3) / 1e9 / PEAK_HBM_GBS, "vs_float32_storage": rep16},
           "exact_scan": {"value": nq * n / (ms_scan * 1e-3), "ms_per_search": ms_scan,
                          "roofline": {"bound": "mfma", "achieved": tf_scan, "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                                       "frac": tf_scan / PEAK_F32_MFMA_TFLOPS, "note": "every pair on v_mfma_f32_32x32x2_f32"}},
           "methods_bit_equal_full_size": bool(torch.equal(i, i_scan) and torch.equal(s.view(torch.int32), s_scan.view(torch.int32)))}
    # D = 512 ("also bench D=512"; face feat_dim): the wide pre-filter kernels
    d5 = 512
    g.manual_seed(2)
    gal5 = cbir.l2_normalize(torch.randn(n, d5, generator=g).to(dev)); qry5 = cbir.l2_normalize(torch.randn(nq, d5, generator=g).to(dev))
    ms5, s5, i5, fb5 = timed("prefilter", gal_=gal5, qry_=qry5, dim=d5)
    out["d512"] = {"ms_per_search": ms5, "value": nq * n / (ms5 * 1e-3), "mfma_frac": 2.0 * nq * n * d5 / (ms5 * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, "optimistic_fallbacks": fb5}
    if with_cpu:
        from oracle import cbir as ocbir
        so5, io5 = ocbir.flat_ip_search(qry5[:16].cpu().numpy(), gal5[:200_000].cpu().numpy(), k)
        idx5 = cbir.FlatIPIndex(d5, device=dev); idx5.add(gal5[:200_000])
        s5b, i5b = idx5.search(qry5[:16], k)
        out["d512"]["parity_vs_oracle"] = {"indices_equal": bool((i5b.cpu().numpy() == io5).all()), "scores_bit_equal": bool((s5b.cpu().numpy().view("uint32") == so5.view("uint32")).all())}
    del gal5, qry5
    if with_cpu:
        from oracle import cbir as ocbir
        qs = qry[:64].cpu().numpy(); gs = gal[:500_000].cpu().numpy()
        t0 = time.time(); so, io = ocbir.flat_ip_search(qs, gs, k); dt = time.time() - t0
        out["cpu_baseline_c_port"] = {"value": 64 * 500_000 / dt, "unit": "pairs/sec", "cores": ocbir.usable_cores(), "kind": "port",
                                      "sample": "oracle/cbir_oracle.c (OpenMP, AVX2 fmaf chains): 64 queries x 500k gallery rows, D=128, k=100"}
        # the whole gallery against the oracle: the timed search's own answer for the first 1024 queries x all 1 M rows (the 64 x 500 k check below is a prefix problem)
        t0 = time.time(); so_f, io_f = ocbir.flat_ip_search(qry[:1024].cpu().numpy(), gal.cpu().numpy(), k); dt_f = time.time() - t0
        out["parity_full_gallery_vs_oracle"] = {"queries": 1024, "gallery_rows": n, "indices_equal": bool((i[:1024].cpu().numpy() == io_f).all()),
                                                "scores_bit_equal": bool((s[:1024].cpu().numpy().view("uint32") == so_f.view("uint32")).all()),
                                                "oracle_seconds": round(dt_f, 2), "oracle_pairs_per_sec": 1024 * n / dt_f}
        # BASELINE.md §3's protocol beside it: the loop the reference's faiss call stands for, torch.topk(q @ G.T, k) in query batches of 256 over the FULL gallery, fp32, all cores
        # (bounded: 4 batches = 1024 queries x 1 M rows, ~3 s; the whole 10 k would be ~30 s)
        torch.set_num_threads(ocbir.usable_cores())
        gh, qh = gal.cpu(), qry[:1024].cpu()
        torch.topk(qh[:256] @ gh.t(), k)
        t0 = time.time()
        for i0 in range(0, 1024, 256):
            torch.topk(qh[i0:i0 + 256] @ gh.t(), k)
        dt2 = time.time() - t0
        # (the faster of the two CPU paths, and the one BASELINE.md §3 describes: this is the baseline the GPU number stands beside)
        out["cpu_baseline"] = {"value": 1024 * n / dt2, "unit": "pairs/sec", "cores": torch.get_num_threads(), "kind": "port",
                               "sample": "torch.topk(q @ G.T, 100), fp32, query batches of 256, 4 batches over the full 1 M x 128 gallery"}
        del gh, qh
        # parity on the sample: the GPU's answer restricted to the same gallery prefix
        idx2 = cbir.FlatIPIndex(d, device=dev); idx2.add(gal[:500_000])
        s2, i2 = idx2.search(qry[:64], k)
        out["parity_vs_oracle"] = {"indices_equal": bool((i2.cpu().numpy() == io).all()),
                                   "scores_bit_equal": bool((s2.cpu().numpy().view("uint32") == so.view("uint32")).all())}
        # fp16 storage against ITS oracle: the same search on the fp16-rounded vectors
        q16 = qs.astype("float16").astype("float32"); g16 = gs.astype("float16").astype("float32")
        so16, io16 = ocbir.flat_ip_search(q16, g16, k)
        idx3 = cbir.FlatIPIndex(d, device=dev, storage="float16"); idx3.add(gal[:500_000])
        s3, i3 = idx3.search(qry[:64], k)
        out["float16_storage"]["parity_vs_fp16_oracle"] = {"indices_equal": bool((i3.cpu().numpy() == io16).all()),
                                                           "scores_bit_equal": bool((s3.cpu().numpy().view("uint32") == so16.view("uint32")).all())}
    return out


def bench_cfg5(be, dev, batch: int = 128, steps: int = 3):
    """BASELINE.json configs[4] (stretch) beside the headline: vit_large_patch14_siglip_336 (576 tokens, MAP head), per-GPU batch 128, a Mixup pair every step + SAM (two
    forward-backward passes) on fp16 operands (the headline: the mode that meets north_star's tolerance at full size, tests/test_fp16_operands.py), bf16 operands and the
    engine's fp8 operand mode beside it; and what fp8 costs in accuracy, measured live against the fp32 oracle on a 2-block ViT whose branch weights are scaled 3x
    (tests/test_vit_fp8.py; the full-size figures of tests/test_parity_fullsize_gpu.py are quoted)."""
    from oracle.vit_ref import VisionTransformerRef
    from visiondk_amd import ops, vit
    out = {"workload": f"cfg5: vit_large_patch14_siglip_336, per-GPU batch {batch}, Mixup pair + SAM (2 fwd/bwd per step), CE ls 0.05, SGD + EMA",
           "dtype": "fp16 operands + GradScaler protocol (headline) | bf16 operands | fp8 (e4m3 forward, e5m2 gradients, delayed per-tensor scaling) in the forward / input-gradient GEMMs of the block Linears, bf16 weight gradients"}
    # ---- tolerance: 2-block ViT, fp8 vs the fp32 oracle and vs the same engine with bf16 operands
    torch.manual_seed(0)
    ref = VisionTransformerRef(64, 8, 3, 10, 256, 2, 4, 512)
    with torch.no_grad():
        for blk in ref.blocks:
            for lin in (blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2):
                lin.weight.mul_(3.0)
    small = vit.VisionTransformer(vit.VitSpec(img_size=64, patch_size=8, num_classes=10, dim=256, depth=2, heads=4, mlp_dim=512), device=dev, backend=be, seed=1)
    small.load_state_dict(ref.state_dict())
    x = torch.randn(4, 3, 64, 64); y = torch.randint(0, 10, (4,))
    lr = ref(x); torch.nn.functional.cross_entropy(lr, y).backward()
    rel = lambda a, b: ((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-30)).item()

    def fb():
        for p_ in small.parameters():
            p_.grad = None
        lo = small(x.to(dev)); torch.nn.functional.cross_entropy(lo, y.to(dev)).backward()
        return lo.detach().cpu(), {n: p_.grad.detach().cpu().clone() for n, p_ in small.named_parameters()}
    l16, g16 = fb()
    small.engine.enable_fp8(2)
    l8, g8 = fb()
    small.engine.enable_fp8(0)
    out["fp8_tolerance"] = {"model": "2-block ViT (dim 256, 64 x 64 input, branch weights x 3), batch 4, forward + backward vs oracle/vit_ref.py (fp32)",
                            "fp8_logits_rel": rel(l8, lr.detach()), "fp8_worst_grad_rel": max(rel(g8[n], p_.grad) for n, p_ in ref.named_parameters()),
                            "bf16_logits_rel": rel(l16, lr.detach()), "bf16_worst_grad_rel": max(rel(g16[n], p_.grad) for n, p_ in ref.named_parameters()),
                            "full_size_quoted": "vit_large_patch14_siglip_336, 2 images, every gradient vs the fp32 oracle: fp16 operands asserted <= 1e-3 / <= 5e-3 (tests/test_fp16_operands.py); bf16 logits 4.2e-3 / worst gradient 8.0e-3; fp8 logits 6.8e-2 / median gradient 7.6e-2 / worst 1.3e-1 (tests/test_parity_fullsize_gpu.py)"}
    del small, ref
    # ---- throughput of the real model
    xb = torch.randn(batch, 3, 336, 336, device=dev); ya = torch.randint(0, 1000, (batch,), device=dev)
    perm = torch.randperm(batch, device=dev); yb = ya[perm].contiguous()
    for key, operand, fp8 in (("sam_fp16", "fp16", 0), ("sam_bf16", "bf16", 0), ("sam_fp8", "bf16", 1)):
        model = vit.create_model("vit_large_patch14_siglip_336", num_classes=1000, device=dev, operand=operand)
        ntok = model.engine.tokens
        flop_img = 3 * 2 * (302.3e6 * ntok + 24 * 2 * ntok * ntok * 1024 + 2 * 1024 * 1024 * ntok)
        model.engine.enable_fp8(fp8)
        step = vit.MapTrainStep(model, lr=0.006, momentum=0.937, weight_decay=5e-4, label_smoothing=0.05, max_norm=10.0, ema=True, sam=True)

        def one():
            step.step(ops.mixup(xb, perm, 0.4), ya, yb, 0.4)
        for _ in range(2):
            one()
        torch.cuda.synchronize(); t0 = time.time()
        for _ in range(steps):
            one()
        torch.cuda.synchronize(); dt = (time.time() - t0) / steps
        out[key] = {"images_per_sec": batch / dt, "ms_per_step": dt * 1e3, "model_tflops": flop_img * batch * 2 / dt / 1e12, "loss": step.loss_value()}
        if operand == "fp16":
            out[key]["loss_scale"] = step.loss_scale(); out[key]["skipped_steps"] = step.skipped_steps()
        model.engine.enable_fp8(0)
        del step, model
        torch.cuda.empty_cache()
    # Which figure stands for cfg5: BASELINE.json configs[4] says "fp8 MFMA", north_star says logits within 1e-3 of the reference.  The fp8 operand mode is two orders outside
    # that tolerance (fp8_tolerance above: an e4m3 operand carries 2^-4 of rounding) and bf16 operands measure 4.2e-3 / 8.0e-3 at full size; fp16 operands -- the
    # reference's own autocast dtype -- meet 1e-3 / 5e-3 literally on this model (tests/test_fp16_operands.py).  SAM under fp16: the reference's update_sam calls
    # loss.backward() without its GradScaler (train.py:157-170); this step runs both passes at the scaler's current loss scale (e(w) is invariant under it), un-scales in the
    # base step, and an overflow in either pass skips the update, restores w and halves the scale (vit.MapTrainStep).
    out["headline"] = {"key": "sam_fp16", "tolerance_met": True,
                       "why": "fp16 operands meet north_star's 1e-3 / 5e-3 at full size (asserted in tests/test_fp16_operands.py); bf16 (4.2e-3 / 8.0e-3) and fp8 (6.8e-2) are reported beside it as non-conforming opt-in modes"}
    return out


def bench_cfg3(be, dev, batch: int = 512, steps: int = 4, ncls: int = 1_000_000):
    """BASELINE.json configs[2] on one GPU: ConvNeXt-Base + neck (feat_dim 512) + ArcFace(C = 10^6, m = .35, s = 32), batch 512 -- one step = compute_loss(face=True) +
    Trainer.update (forward, fused margin head + CE that never writes the B x C logits, backward, clip 10, layer-wise SGD, EMA; /root/reference/configs/faceX/cbir.yaml:30-37,
    engine/procedure/train.py:217-280) on fp16 operands with the GradScaler protocol: the mode tests/test_parity_fullsize_gpu.py holds to north_star's tolerance against the
    reference's fp32 loop at C = 10^6.  The head's class dimension is what the 8-GPU configuration shards; here it is whole (2 GB of fp32 weights + momentum + EMA)."""
    from visiondk_amd import face
    cfg = {"task": "cbir", "image_size": 224, "backbone": {"timm-convnext_base": {"pretrained": False, "image_size": 224, "feat_dim": 512, "operand": "fp16"}},
           "head": {"arcface": {"feat_dim": 512, "num_class": ncls, "margin_arc": 0.35, "margin_am": 0.0, "scale": 32}}}
    torch.manual_seed(0)
    model = face.get_model(cfg, None, 0).model.train()
    step = face.FaceTrainStep(model, lr=0.01, momentum=0.9, weight_decay=5e-4, max_norm=10.0, ema=True, layer_wise=True, cos_planes=1)      # cosines from single fp16 operands: the mode of the full-size parity test
    g = torch.Generator(device="cpu"); g.manual_seed(0)
    x = torch.randn(batch, 3, 224, 224, generator=g).to(dev)
    y = torch.randint(0, ncls, (batch,), generator=g).to(dev)
    for _ in range(2):
        step.step(x, y)
    torch.cuda.synchronize(); t0 = time.time()
    for _ in range(steps):
        rows = step.step(x, y)
    torch.cuda.synchronize(); dt = (time.time() - t0) / steps
    flop_img = 92.1e9 + 0.15e9 + 3.07e9 * ncls / 1e6          # ConvNeXt-B fwd+bwd (3 x 2 x 15.35 GMAC), neck, the 512 x C head fwd + two backward products
    out = {"workload": f"cfg3: convnext_base + neck 512 + ArcFace(C = {ncls}), batch {batch}: fwd + fused margin CE + bwd + clip + layer-wise SGD + EMA, fp16 operands + GradScaler protocol",
           "dtype": "fp16", "images_per_sec": batch / dt, "ms_per_step": dt * 1e3, "loss": rows.mean().item(), "loss_scale": step.loss_scale(), "skipped_steps": step.skipped_steps(),
           "roofline": {"bound": "mfma", "achieved": flop_img * batch / dt / 1e12, "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": flop_img * batch / dt / 1e12 / PEAK_BF16_TFLOPS,
                        "traffic": None, "flop_per_image": flop_img},
           "parity": "tests/test_parity_fullsize_gpu.py: embeddings <= 1e-3 and every gradient <= 5e-3 against the reference's fp32 loop at C = 10^6 (fp16 operands)"}
    del step, model, x, y
    torch.cuda.empty_cache()
    return out


def bench_swin(be, dev, batch: int = 128, steps: int = 4):
    """swin_base_patch4_window7_224 -- the `name:` both shipped configs of the reference default to (pet.yaml:25, cbir.yaml:26) -- beside the headline: the classifier step
    forward + CE + backward + clip_grad_norm_ + SGD + EMA through the native engine (csrc/swin_engine.hip: one C-ABI call forward, one backward) under vit.FusedTrainStep,
    and a live check of a 2-stage Swin (logits and the worst parameter gradient) against the fp32 oracle (oracle/swin_ref.py, pinned against transformers.SwinModel)."""
    from oracle.swin_ref import SwinTransformerRef
    from visiondk_amd import swin, vit
    out = {"workload": f"swin_base_patch4_window7_224, 37 classes (pet.yaml), batch {batch}: fwd + CE(ls 0.05) + bwd + clip_grad_norm_ + SGD + EMA (native engine, fused step)", "dtype": "fp16 operands (the reference's autocast dtype), fp32 residual stream; bf16 beside it",
           "drop_path_rate": 0.1}      # timm's default for the family: stochastic depth is ON in the timed steps, as it is in the reference's training loop
    torch.manual_seed(0)
    ref = SwinTransformerRef(img_size=224, num_classes=7, embed_dim=32, depths=(2, 2), heads=(1, 2))
    with torch.no_grad():
        for n_, p_ in ref.named_parameters():
            if "relative_position_bias_table" in n_:
                p_.copy_(torch.randn_like(p_) * 0.3)
    small = swin.SwinTransformer(swin.SwinSpec(img_size=224, num_classes=7, embed_dim=32, depths=(2, 2), heads=(1, 2)), device=dev, backend=be, seed=0, operand="fp16")
    small.load_state_dict(ref.state_dict())
    x = torch.randn(2, 3, 224, 224); y = torch.randint(0, 7, (2,))
    lr_ = ref(x); torch.nn.functional.cross_entropy(lr_, y).backward()
    lo = small(x.to(dev)); (torch.nn.functional.cross_entropy(lo, y.to(dev)) * 256.0).backward()          # (GradScaler: scaled backward, unscaled below)
    rel = lambda a, b: ((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-30)).item()
    grads = {n_: rel(p_.grad / 256.0, dict(ref.named_parameters())[n_].grad) for n_, p_ in small.named_parameters()}
    worst = max(grads, key=grads.get)
    out["parity_vs_fp32_oracle"] = {"operand": "fp16", "model": "2-stage Swin (dim 32 / 64, 56 x 56 and 28 x 28 maps: shifted windows, masks, patch merging), batch 2", "logits_rel": rel(lo.detach(), lr_.detach()),
                                    "worst_grad_rel": grads[worst], "worst_grad": worst,
                                    "full_size_quoted": "swin_base, every gradient vs the fp32 oracle (tests/test_swin.py): bf16 operands logits 5.9e-3, worst gradient 1.1e-2; fp16 operands asserted <= 1e-3 / <= 5e-3"}
    del small, ref
    xb = torch.randn(batch, 3, 224, 224, device=dev); yb = torch.randint(0, 37, (batch,), device=dev)
    for operand in ("fp16", "bf16"):          # fp16: the reference's autocast dtype (GradScaler protocol inside the fused step); bf16 beside it
        model = swin.create_model("swin_base_patch4_window7_224", num_classes=37, device=dev, backend=be, seed=0, operand=operand)
        fused = vit.FusedTrainStep(model, lr=0.006, momentum=0.937, weight_decay=5e-4, label_smoothing=0.05, max_norm=10.0, ema=True)
        for _ in range(2):
            fused.step(xb, yb)
        torch.cuda.synchronize(); t0 = time.time()
        for _ in range(steps):
            fused.step(xb, yb)
        torch.cuda.synchronize(); dt = (time.time() - t0) / steps
        rec = {"images_per_sec": batch / dt, "ms_per_step": dt * 1e3, "model_tflops": 3 * 15.47e9 * batch / dt / 1e12, "loss": fused.loss_value()}
        if operand == "fp16":
            out.update(rec)
            out["operand"] = "fp16"
        else:
            out["bf16_operands"] = rec
        del model, fused
        torch.cuda.empty_cache()
    return out


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)


def _barrier(world):
    if world > 1:
        dist.barrier()


def _max_over_ranks(dt: float, world: int, dev) -> float:
    if world == 1:
        return dt
    t = torch.tensor([dt], dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def train_leg(be, dev, rank: int, world: int, steps: int, warmup: int, batch: int, spec=None, img: int = 224, classes: int = 1000, events: bool = True,
              bucket_bytes: int = 24 << 20, operand: str = "bf16", outputs: dict | None = None):
    """Hot path A on this rank (one process per GPU): W warm-up steps, barrier + sync, K timed steps, sync + barrier, MAX over ranks.
    Returns (seconds for K steps, final loss, gemm event totals or None, collectives issued).  N > 1: the flat gradient leaves in buckets from inside the backward
    (visiondk_amd/comm.py), overlapped with the remaining backward kernels.  The same function runs on CPU over gloo with the emulated kernels (tests/test_ddp_gloo.py).
    `outputs` (a dict) receives, after the timing, the host copies --dump-outputs writes (last_step_outputs)."""
    from visiondk_amd import comm as vcomm, vit
    if spec is None:
        spec = vit.spec_from_timm_name("vit_base_patch16_224", classes)
    model = vit.VisionTransformer(spec, device=dev, backend=be, seed=2, operand=operand)
    comm = vcomm.GradAllReduce(bucket_bytes=bucket_bytes) if world > 1 else None      # FusedTrainStep broadcasts rank 0's weights (DDP-constructor semantics)
    step = vit.FusedTrainStep(model, lr=0.006, momentum=0.937, weight_decay=5e-4, label_smoothing=0.05, max_norm=10.0, ema=(rank == 0), comm=comm)
    g = torch.Generator(device="cpu"); g.manual_seed(1000 + rank)
    x = torch.randn(batch, 3, img, img, generator=g).to(dev)
    y = torch.randint(0, classes, (batch,), generator=g).to(dev)
    for _ in range(warmup):
        step.step(x, y)
    _sync(dev); _barrier(world)
    # live per-launch timing of the dominant kernel (bf16 GEMM) with HIP events on the launch stream
    launches_per_step = (7 * spec.depth * 2 + 8) * 2            # (a GEMM that splits its rows over two kernels carries one pair per kernel)
    ev = events and dev.type == "cuda" and os.environ.get("VDK_BENCH_NO_EVENTS") != "1"      # (diagnostic: what the per-launch HIP events themselves cost)
    if ev:
        be.check(be.lib.vdk_prof_begin(launches_per_step * steps + 64), "vdk_prof_begin")
    _sync(dev)
    t0 = time.perf_counter()
    rows = None
    for it in range(steps):
        if ev:      # every GEMM launch of every 4th timed step carries a (start, stop) event pair: a timed dispatch costs ~5 us of queue time, 0.7-1.0 ms per step if all 149 are timed
            be.lib.vdk_prof_pause(0 if it % GEMM_EVENT_STRIDE == 0 else 1)
        rows = step.step(x, y)
    _sync(dev); _barrier(world)
    dt = time.perf_counter() - t0
    gemm = None
    if ev:
        gemm_ms, gemm_n, gemm_fl, gemm_bytes = C.c_double(0), C.c_int64(0), C.c_double(0), C.c_double(0)
        be.check(be.lib.vdk_prof_end(C.byref(gemm_ms), C.byref(gemm_n), C.byref(gemm_fl)), "vdk_prof_end")
        be.check(be.lib.vdk_prof_bytes(C.byref(gemm_bytes)), "vdk_prof_bytes")
        gemm = {"ms": gemm_ms.value, "n": gemm_n.value, "flops": gemm_fl.value, "bytes": gemm_bytes.value}
    dt = _max_over_ranks(dt, world, dev)
    loss = step.loss_value()
    ncoll = comm.collectives if comm is not None else 0
    if gemm is not None and step.amp:
        gemm["loss_scale"] = step.loss_scale(); gemm["skipped_steps"] = step.skipped_steps()
    if outputs is not None:
        outputs.update(last_step_outputs(step, rows))
    del step, model
    return dt, loss, gemm, ncoll


def last_step_outputs(step, rows) -> dict:
    """what FusedTrainStep hands its caller after the last step, as float32 host arrays: the per-image losses it returned, the fp32 master weights and the EMA
    weights (at DUMP_SAMPLE positions drawn from a fixed seed, sorted; all of them when there are fewer), the GradScaler state on fp16 operands"""
    params = step.eng.params
    n = params.numel()
    if n <= DUMP_SAMPLE:
        idx = torch.arange(n)
    else:
        g = torch.Generator(device="cpu"); g.manual_seed(0)
        idx = torch.randint(0, n, (DUMP_SAMPLE,), generator=g).sort().values
    idx = idx.to(params.device)
    out = {"params_sample": params.reshape(-1)[idx]}
    if rows is not None:
        out["loss_rows"] = rows
    if step.ema is not None:
        out["ema_sample"] = step.ema.reshape(-1)[idx]
    if step.loss_state is not None:
        out["loss_state"] = step.loss_state
    return {k: v.detach().float().cpu().numpy() for k, v in out.items()}


def dump_outputs(outdir: str, arrays: dict) -> None:
    import numpy as np
    os.makedirs(outdir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(outdir, f"{name}.npy"), np.ascontiguousarray(a, dtype=np.float32))


def cbir_sharded_leg(be, dev, rank: int, world: int, nq: int = 10000, n: int = 1_000_000, d: int = 128, k: int = 100, iters: int = 6, warm: int = 3, cap=None,
                     check_queries: int = 16):
    """Hot path B at N > 1: the gallery's rows are sharded over the ranks (n / world each, 125 k at N = 8), every rank owns nq / world of the
    queries; one search = all-gather of the queries, every rank scans its shard for ALL queries, all-to-all of the per-shard top-k lists, merge
    (visiondk_amd/cbir.py search_sharded).  Strong scaling: nq x n pairs per search whatever N is.  Timing: barrier + sync, `iters` searches, sync + barrier, MAX
    over ranks.  Rank 0 checks its first `check_queries` queries against the oracle over the WHOLE gallery (every shard regenerated on the host from its seed)."""
    from visiondk_amd import cbir
    rows = [n // world + (1 if r < n % world else 0) for r in range(world)]
    qn = [nq // world + (1 if r < nq % world else 0) for r in range(world)]
    base = sum(rows[:rank])

    def shard(r):          # rank r's gallery rows, the same on whichever host generates them
        g = torch.Generator(device="cpu"); g.manual_seed(7000 + r)
        return torch.nn.functional.normalize(torch.randn(rows[r], d, generator=g))

    def queries(r):
        g = torch.Generator(device="cpu"); g.manual_seed(9000 + r)
        return torch.nn.functional.normalize(torch.randn(qn[r], d, generator=g))

    gal = shard(rank).to(dev); qry = queries(rank).to(dev)
    kw = {} if cap is None else {"cap": cap}
    index = cbir.FlatIPIndex(d, backend=be, device=dev, idx_base=base, **kw)
    index.add(gal)
    s = i = None
    for _ in range(warm):
        s, i = cbir.search_sharded(qry, gal, k, base, backend=be, device=dev, query_counts=qn, index=index)
    _sync(dev); _barrier(world)
    t0 = time.perf_counter()
    for _ in range(iters):
        s, i = cbir.search_sharded(qry, gal, k, base, backend=be, device=dev, query_counts=qn, index=index)
    _sync(dev); _barrier(world)
    dt = _max_over_ranks(time.perf_counter() - t0, world, dev) / iters
    out = {"metric": "CBIR query-pairs/sec (exact fp32 inner product + top-100), gallery sharded over the ranks", "value": nq * n / dt, "unit": "pairs/sec",
           "ms_per_search": dt * 1e3, "n_gpus": world, "scaling": "strong",
           "config": {"workload": f"cbir Q={nq} N={n} D={d} k={k} fp32 gallery, {rows[0]} rows and {qn[0]} queries per rank",
                      "exchange": "all-gather of the queries, all-to-all of the per-shard top-k lists (scores + global row ids), merge by (score desc, index asc)"}}
    if rank == 0 and check_queries > 0:
        from oracle import cbir as ocbir
        whole = torch.cat([shard(r) for r in range(world)]).numpy()
        nchk = min(check_queries, qn[0])
        so, io = ocbir.flat_ip_search(queries(0)[:nchk].numpy(), whole, k)
        out["parity_vs_oracle"] = {"queries": nchk, "gallery_rows": n, "indices_equal": bool((i[:nchk].cpu().numpy() == io).all()),
                                   "scores_bit_equal": bool((s[:nchk].cpu().numpy().view("uint32") == so.view("uint32")).all())}
    return out


def rccl_topology_lines(path: str, limit: int = 24):
    """the ring / tree / transport lines RCCL logged at communicator creation (NCCL_DEBUG=INFO, subsystems INIT + GRAPH, written to `path` by rank 0)"""
    import re
    try:
        with open(path, errors="replace") as f:
            lines = f.read().splitlines()
    except OSError:
        return None
    pat = re.compile(r"(Ring \d+|Trees? |Channel \d+|channels|xgmi|XGMI|via P2P|via SHM|NET/|RCCL version|NCCL version|comm 0x.* rank 0 nranks)", re.I)
    keep = [re.sub(r"^\S+:\d+:\d+ \[\d+\] ", "", ln) for ln in lines if pat.search(ln)]
    return keep[:limit]


def self_spawn(n: int):
    """`python bench.py --gpus N` without a launcher: start the N ranks here (one process per GPU, the same torch.distributed.run line the driver uses) and
    pass their output and exit code through."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1", "--master-port", str(port),
           str(Path(__file__).resolve()), *sys.argv[1:]]
    raise SystemExit(subprocess.call(cmd))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256, help="per-GPU batch (BASELINE: 256)")
    ap.add_argument("--no-cbir", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-parity", action="store_true")
    ap.add_argument("--no-cfg5", action="store_true")
    ap.add_argument("--no-swin", action="store_true")
    ap.add_argument("--no-cfg3", action="store_true")
    ap.add_argument("--operand", choices=("fp16", "bf16"), default="fp16",
                    help="16-bit operand format of the headline leg: fp16 = the reference's autocast dtype + GradScaler (train.py:118,205-211), bf16 = BASELINE.json configs[1]'s word; the other one is timed beside it")
    ap.add_argument("--no-other-operand", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beyond the headline: GEMM event timing (roofline.dominant_kernel), parity, the other operand, cpu_baseline, cfg5, swin, cfg3, CBIR "
                         "(the --no-* switches drop single legs of it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last step's outputs (rank 0) to DIR/<name>.npy, float32")
    args = ap.parse_args()

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        self_spawn(args.gpus)
    rank = int(os.environ.get("RANK", "0")); local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    assert torch.cuda.is_available(), "bench.py needs the MI355X (there is no CPU fallback)"
    # DIAGNOSTIC, never a measurement: VDK_BENCH_SHARE_GPU=1 puts every rank on cuda:0 and exchanges over gloo, so that the N > 1 code path of this file (bucketed gradient
    # exchange inside the backward, max-over-ranks timing, the sharded search, the JSON assembly) can be executed end to end on a 1-GPU box; the line says so in `diagnostic`
    share_gpu = world > 1 and os.environ.get("VDK_BENCH_SHARE_GPU") == "1"
    if share_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    rccl_log = None
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("NCCL_MAX_NCHANNELS", "32")      # = the CUs GradAllReduce keeps out of the persistent GEMM grids (profiles/r03_w4_contention.json)
        if args.full and rank == 0 and "NCCL_DEBUG" not in os.environ:      # the rings / trees RCCL builds over xGMI, quoted in the JSON line (rank 0's log only)
            import tempfile
            rccl_log = os.path.join(tempfile.gettempdir(), f"vdk_rccl_{os.getpid()}.log")
            os.environ.update({"NCCL_DEBUG": "INFO", "NCCL_DEBUG_SUBSYS": "INIT,GRAPH", "NCCL_DEBUG_FILE": rccl_log})
        if share_gpu:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    from visiondk_amd import _lib
    be = _lib.load()

    other = "bf16" if args.operand == "fp16" else "fp16"
    full = args.full
    parity = parity_vit(be, dev, args.operand) if (full and world == 1 and rank == 0 and not args.no_parity) else None
    parity_other = parity_vit(be, dev, other) if (parity is not None and not args.no_other_operand) else None
    outputs = {} if (args.dump_outputs and rank == 0) else None
    dt, loss, gemm, ncoll = train_leg(be, dev, rank, world, args.steps, args.warmup, args.batch, events=full, operand=args.operand, outputs=outputs)
    if outputs is not None:
        dump_outputs(args.dump_outputs, outputs)
        del outputs
    leg2 = None
    if full and world == 1 and not args.no_other_operand:      # the other operand format, same box, same steps, right after the headline leg
        torch.cuda.empty_cache()
        leg2 = train_leg(be, dev, rank, world, args.steps, args.warmup, args.batch, operand=other)
    cbir_n = None
    if full and world > 1 and not args.no_cbir:
        torch.cuda.empty_cache()
        cbir_n = cbir_sharded_leg(be, dev, rank, world)

    if rank == 0:
        imgs = args.batch * world * args.steps
        value = imgs / dt
        per_gpu_tflops = value / world * VIT_FLOP_PER_IMG / 1e12
        out = {
            "metric": "images/sec fwd+bwd+optimizer step (ViT-B/16, bs=256 per GPU)", "value": value, "unit": "images/sec",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.operand, "data": "synthetic",
            "config": {"workload": "ViT-B/16 ICT, synthetic ImageNet-1k 224x224, random-init weights (reference re-init), "
                                   f"per-GPU batch {args.batch}, CE label_smoothing 0.05, SGD 0.006/0.937/5e-4, clip 10, EMA on rank 0",
                       "global_batch": args.batch * world, "parallelism": f"dp{world}", "final_loss": loss,
                       "operand": (f"{args.operand} MFMA operands, fp32 accumulation, fp32 master weights / residual stream"
                                   + ("; fp16 = the reference's autocast dtype (engine/procedure/train.py:118), loss scaling + inf-skip of train.py:205-211 inside the step"
                                      if args.operand == "fp16" else "; the format BASELINE.json configs[1] names"))},
            # achieved = images/s x 105.38 GFLOP per image (every counted FLOP is matmul-shaped) against the dense 16-bit MFMA peak -- the WHOLE step, every
            # kernel of it, not the GEMM family alone (that is `dominant_kernel` below)
            "roofline": {"bound": "mfma", "achieved": per_gpu_tflops, "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": per_gpu_tflops / PEAK_BF16_TFLOPS,
                         "what": "step level: images/sec/GPU x 105.38 GFLOP (fwd + bwd, BASELINE.md section 2) / 2.5 PFLOP/s", "flop_per_image": VIT_FLOP_PER_IMG,
                         "traffic": None},
        }
        if gemm is not None:
            gemm_avg_ms = gemm["ms"] / max(gemm["n"], 1)
            gemm_tflops = gemm["flops"] / max(gemm["ms"], 1e-9) / 1e9
            out["roofline"]["traffic"] = pmc_traffic_per_launch()
            out["roofline"]["dominant_kernel"] = {"bound": "mfma", "kernel": "gemm_w4_kernel / gemm_w4h_kernel <NT|TN> (one wave per SIMD, 256x256 / 256x128 tiles), the GEMM family of the step",
                               "achieved": gemm_tflops, "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                               "frac": gemm_tflops / PEAK_BF16_TFLOPS, "traffic": pmc_traffic_per_launch(),
                               "algorithmic_bytes_per_launch": gemm["bytes"] / max(gemm["n"], 1),
                               "avg_launch_ms": gemm_avg_ms, "launches": gemm["n"], "gemm_calls_per_step": gemm["n"] // max(1, -(-args.steps // GEMM_EVENT_STRIDE)),
                               "timed_launches": f"every GEMM dispatch of every {GEMM_EVENT_STRIDE}th step of the timed region (start / stop events attached to the dispatch itself)",
                               "flops_per_launch": gemm["flops"] / max(gemm["n"], 1),
                               "gemm_share_of_step_time": (gemm["ms"] / max(1, -(-args.steps // GEMM_EVENT_STRIDE))) / (dt / args.steps * 1e3)}
        if share_gpu:
            out["diagnostic"] = "VDK_BENCH_SHARE_GPU=1: all ranks on ONE GPU, gloo exchange -- exercises the N > 1 code path, the numbers are not a measurement"
        if world > 1:
            out["exchange"] = {"collectives_per_step": ncoll // max(1, args.steps + args.warmup), "bucket_bytes": 24 << 20,
                               "what": "bucketed all-reduce (sum) of the flat fp32 gradient over RCCL, issued from inside the backward; 1/world folded into the SGD kernel",
                               "rccl": rccl_topology_lines(rccl_log) if rccl_log else None}
        if gemm is not None and "loss_scale" in gemm:
            out["config"]["loss_scale_after_run"] = gemm["loss_scale"]; out["config"]["skipped_steps"] = gemm["skipped_steps"]
        if leg2 is not None:
            dt2, loss2, gemm2, _ = leg2
            v2 = args.batch * args.steps / dt2
            out["other_operand"] = {"operand": other, "value": v2, "unit": "images/sec", "ms_per_step": dt2 / args.steps * 1e3, "final_loss": loss2,
                                    "roofline_frac_step": v2 * VIT_FLOP_PER_IMG / 1e12 / PEAK_BF16_TFLOPS,
                                    "gemm_tflops": None if gemm2 is None else gemm2["flops"] / max(gemm2["ms"], 1e-9) / 1e9,
                                    "gemm_avg_launch_ms": None if gemm2 is None else gemm2["ms"] / max(gemm2["n"], 1)}
        if parity is not None:
            out["parity"] = parity
        if parity_other is not None:
            out["parity_other_operand"] = parity_other
        if full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline_vit()
        if full and world == 1 and not args.no_cfg5:
            torch.cuda.empty_cache()
            out["cfg5"] = bench_cfg5(be, dev)
        if full and world == 1 and not args.no_swin:
            torch.cuda.empty_cache()
            out["swin"] = bench_swin(be, dev)
        if full and world == 1 and not args.no_cfg3:
            torch.cuda.empty_cache()
            out["cfg3"] = bench_cfg3(be, dev)
        if full and world == 1 and not args.no_cbir:
            torch.cuda.empty_cache()
            out["cbir"] = bench_cbir(dev, with_cpu=not args.no_cpu_baseline)
        elif cbir_n is not None:
            out["cbir"] = cbir_n
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
