"""Cosine HDBSCAN timings (csrc/cbir_mst.hip + the host tree code of visiondk_amd/cluster.py) on seeded mixtures.

    python tools/bench_hdbscan.py [--sizes 1000,10000,100000] [--d 128] [--cpu-sizes 1000,10000] [--out profiles/hdbscan.json]

Per size (N = 1000 is the slice the reference's tools/clustering.py takes): a warm-up run, then
* a run with the stage callback of cluster._mst_device, which synchronises at every stage: normalise + prepare, core distances (the top-k self-search), every round's
  row scan (bound + propose + decide together: their split is the kernel trace's, below) and bookkeeping, and after every scan the number of proposed pairs per row,
  counted from the one-bit-per-pair matrix the scan left in its workspace;
* a run without the callback: the device part end to end, and the host tree code (tree_to_labels) on the tree it returned;
* rounds, workspace bytes, clusters and noise points found.
The CPU leg is sklearn.cluster.HDBSCAN(metric="cosine") on the host at --cpu-sizes, with the number of cores it may use and the adjusted Rand index against the device.
Host clock around a device synchronise, profiler off.  Kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats -- python tools/bench_hdbscan.py --sizes 100000 --cpu-sizes "" --trace-run
One JSON line per measurement on stdout; --out also writes them to a file.  Needs the GPU: there is no fallback."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from visiondk_amd import _lib, cluster

LINES = []


def emit(**kw):
    LINES.append(kw)
    print(json.dumps(kw), flush=True)


def mixture(n, d, seed, dev):
    """centres randn, points = centre + 0.45 randn (about 500 per centre, at least 6 centres), 15 % of the rows replaced by pure randn; float32 on the device"""
    gen = torch.Generator(device=dev).manual_seed(seed)
    centres = torch.randn((max(6, n // 500), d), generator=gen, device=dev)
    x = centres[torch.randint(0, centres.shape[0], (n,), generator=gen, device=dev)] + 0.45 * torch.randn((n, d), generator=gen, device=dev)
    noise = torch.randperm(n, generator=gen, device=dev)[: int(0.15 * n)]
    x[noise] = torch.randn((noise.numel(), d), generator=gen, device=dev)
    return x.contiguous(), int(centres.shape[0])


def popcount_rows(be, info):
    """set bits of the bit matrix in the workspace (the last row block's), SWAR over slabs of 256 column blocks"""
    off, pitch, blocks = C.c_size_t(0), C.c_int64(0), C.c_int64(0)
    be.check(be.lib.vdk_mst_scan_mask_layout(info["rows"], info["n"], info["d"], C.byref(off), C.byref(pitch), C.byref(blocks)), "vdk_mst_scan_mask_layout")
    words = info["ws"][off.value: off.value + blocks.value * pitch.value * 4].view(torch.int32).view(blocks.value, pitch.value)
    total = 0
    for b0 in range(0, blocks.value, 256):
        v = words[b0:b0 + 256, :info["rows"]].to(torch.int64) & 0xffffffff
        v = v - ((v >> 1) & 0x55555555)
        v = (v & 0x33333333) + ((v >> 2) & 0x33333333)
        v = (v + (v >> 4)) & 0x0f0f0f0f
        total += int(((v * 0x01010101) >> 24 & 0xff).sum().item())
    return total / info["rows"]


def staged_run(be, x, ms):
    stages, state = [], {"t": None}

    def on_stage(stage, rnd, info):
        torch.cuda.synchronize()
        now = time.perf_counter()
        rec = {"stage": stage, "round": rnd, "ms": (now - state["t"]) * 1e3}
        if stage == "scan":
            rec["proposed_pairs_per_row"] = popcount_rows(be, info)       # (outside the timed span)
        if stage == "bookkeeping":
            rec["components_left"] = info["components"]
        stages.append(rec)
        torch.cuda.synchronize()
        state["t"] = time.perf_counter()
    cluster._mst_device.on_stage = on_stage
    try:
        torch.cuda.synchronize()
        state["t"] = time.perf_counter()
        cluster.mutual_reachability_mst(x, ms)
    finally:
        cluster._mst_device.on_stage = None
    return stages


def bench_size(args, be, dev, n):
    x, planted = mixture(n, args.d, n, dev)
    mcs, ms, eps = args.min_cluster_size, args.min_samples, args.epsilon
    cluster.mutual_reachability_mst(x, ms)                        # warm-up of every kernel and allocation of this shape
    stages = [] if args.trace_run else staged_run(be, x, ms)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    u, v, w, core = cluster.mutual_reachability_mst(x, ms)
    torch.cuda.synchronize()
    t_dev = time.perf_counter() - t0
    rounds = cluster.mutual_reachability_mst.last_rounds
    un, vn, wn = u.cpu().numpy(), v.cpu().numpy(), w.cpu().numpy().astype(np.float64)
    t0 = time.perf_counter()
    labels, prob = cluster.tree_to_labels(un, vn, wn, mcs, eps)
    t_tree = time.perf_counter() - t0
    scans = [s for s in stages if s["stage"] == "scan"]
    emit(what="cluster.hdbscan", n=n, d=args.d, min_cluster_size=mcs, min_samples=ms, cluster_selection_epsilon=eps, planted=planted, clusters=int(labels.max()) + 1,
         noise=int((labels < 0).sum()), rounds=rounds, workspace_bytes=cluster._mst_device.last_workspace_bytes, device_ms=t_dev * 1e3, host_tree_ms=t_tree * 1e3,
         prepare_ms=sum(s["ms"] for s in stages if s["stage"] == "prepare"), core_ms=sum(s["ms"] for s in stages if s["stage"] == "core"),
         scan_ms_per_round=[round(s["ms"], 3) for s in scans], bookkeeping_ms_per_round=[round(s["ms"], 3) for s in stages if s["stage"] == "bookkeeping"],
         proposed_pairs_per_row_per_round=[round(s["proposed_pairs_per_row"], 2) for s in scans],
         components_left_per_round=[s["components_left"] for s in stages if s["stage"] == "bookkeeping"])
    return x, labels


def bench_cpu(args, x, labels):
    from sklearn.cluster import HDBSCAN
    from sklearn.metrics import adjusted_rand_score
    xs = x.cpu().numpy()
    cores = len(os.sched_getaffinity(0))
    t0 = time.perf_counter()
    sk = HDBSCAN(min_cluster_size=args.min_cluster_size, min_samples=args.min_samples, cluster_selection_epsilon=args.epsilon, metric="cosine", n_jobs=min(16, cores)).fit(xs)
    s = time.perf_counter() - t0
    emit(what="sklearn.cluster.HDBSCAN(metric=cosine) on the host", n=int(xs.shape[0]), d=args.d, host_cores=cores, n_jobs=min(16, cores), seconds=s,
         clusters=int(sk.labels_.max()) + 1, noise=int((sk.labels_ < 0).sum()), adjusted_rand_index_against_device=float(adjusted_rand_score(sk.labels_, labels)),
         noise_status_differs=int(((sk.labels_ < 0) != (labels < 0)).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,10000,100000")
    ap.add_argument("--cpu-sizes", default="1000,10000")
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--min-cluster-size", type=int, default=10)
    ap.add_argument("--min-samples", type=int, default=5)
    ap.add_argument("--epsilon", type=float, default=0.2)
    ap.add_argument("--trace-run", action="store_true", help="no staged run (under rocprofv3 --kernel-trace: the kernels of a warm-up and one plain run only)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_hdbscan.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    be = _lib.load()
    cpu_sizes = {int(v) for v in args.cpu_sizes.split(",") if v}
    for n in [int(v) for v in args.sizes.split(",") if v]:
        x, labels = bench_size(args, be, dev, n)
        if n in cpu_sizes:
            bench_cpu(args, x, labels)
        del x
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(LINES, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
