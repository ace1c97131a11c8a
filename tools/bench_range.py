"""Range search and cosine DBSCAN timings (csrc/cbir_range.hip), beside the top-k search of the same index in the same process.

    python tools/bench_range.py [--nq 10000] [--n 1000000] [--d 128] [--mean 100] [--windows 5] [--dbscan 100000,1000000] [--cpu-n 20000] [--out profiles/NAME.json]

* range search at cfg4's shape (Q = 10 000, N = 1 000 000, D = 128), fp32 and fp16 storage; the radius is chosen per run from a sample of exact scores so that the mean
  result count is about --mean per query, and is stated with the count it gave;
* `search(k = 100)` on the same index, alternating with the range search, best of --windows windows each (a window = `reps` back-to-back calls ended by a synchronise);
* where the time goes per kernel: a run of its own under `rocprofv3 --kernel-trace --stats -- python tools/bench_range.py --windows 1 --reps 2 --dbscan "" --cpu-n 0`;
* cluster.dbscan on a planted mixture at every N of --dbscan: eps, clusters found, mean neighbourhood size, propagation rounds;
* the CPU leg sklearn.cluster.DBSCAN(metric="cosine") at --cpu-n rows of the same mixture (the largest N the host finishes in about a minute), labelled with that N.
One JSON line per measurement on stdout; --out also writes them to a file.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from visiondk_amd import cbir, cluster

LINES = []


def emit(**kw):
    LINES.append(kw)
    print(json.dumps(kw), flush=True)


def unit_rows(n, d, gen, dev, centres=None, spread=0.0):
    """L2-normalised rows on the device: Gaussian, or (centres given) a planted mixture centre + spread * randn"""
    x = torch.randn((n, d), generator=gen, device=dev, dtype=torch.float32)
    if centres is not None:
        x = centres[torch.randint(0, centres.shape[0], (n,), generator=gen, device=dev)] + spread * x
    return torch.nn.functional.normalize(x, dim=1)


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def radius_for(index, q, g, mean, gen):
    """the radius whose mean result count is about `mean` per query, from the exact scores of 256 queries against 65 536 sampled rows"""
    qs = q[torch.randperm(q.shape[0], generator=gen, device=q.device)[:256]]
    gs = g[torch.randperm(g.shape[0], generator=gen, device=g.device)[:65536]].float()
    s = (qs @ gs.T).reshape(-1)
    frac = min(1.0, mean / g.shape[0])
    kth = max(1, int(round(frac * s.numel())))
    return float(torch.topk(s, kth).values[-1])


def bench_search(args, dev, storage):
    gen = torch.Generator(device=dev).manual_seed(0)
    g, q = unit_rows(args.n, args.d, gen, dev), unit_rows(args.nq, args.d, gen, dev)
    index = cbir.FlatIPIndex(args.d, device=dev, storage=storage)
    index.add(g)
    r = radius_for(index, q, index._materialize(), args.mean, gen)
    lims, D, I = index.range_search(q, r)                       # warm-up of every shape; also the count the radius gives
    index.search(q, 100)
    mean = float(lims[-1]) / args.nq
    # the range result against the top-k result where both are defined: a query with <= 100 results owns exactly the top of its top-k list
    s100, i100 = index.search(q, 100)
    cnt = (lims[1:] - lims[:-1])
    small = torch.nonzero(cnt <= 100).reshape(-1)[:64].tolist()
    for qi in small:
        a = set(I[lims[qi]:lims[qi + 1]].tolist())
        b = set(i100[qi, :int(cnt[qi])].tolist())
        assert a == b, f"query {qi}: range result and top-k disagree"
    t_range, t_topk = [], []
    for _ in range(args.windows):                               # alternating windows
        t_range.append(window(lambda: index.range_search(q, r), args.reps))
        t_topk.append(window(lambda: index.search(q, 100), args.reps))
    emit(what="range_search vs search(k=100)", storage=storage, nq=args.nq, n=args.n, d=args.d, radius=r, mean_results=mean, checked_against_topk=len(small),
         range_ms_best=min(t_range), range_ms_windows=t_range, topk_ms_best=min(t_topk), topk_ms_windows=t_topk, reps_per_window=args.reps)
    return index, q, r


def bench_dbscan(args, dev, n):
    gen = torch.Generator(device=dev).manual_seed(1)
    centres = torch.randn((n // 500, args.d), generator=gen, device=dev)          # ~500 rows per planted cluster
    x = unit_rows(n, args.d, gen, dev, centres, 0.45)
    cluster.dbscan(x[: min(n, 20000)], args.eps, 5)                               # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    labels, core = cluster.dbscan(x, args.eps, 5)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    emit(what="cluster.dbscan", n=n, d=args.d, eps=args.eps, min_samples=5, planted=int(centres.shape[0]), clusters=int(labels.max()) + 1, core=int(core.numel()),
         noise=int((labels < 0).sum()), mean_neighbourhood=cluster.dbscan.last_mean_neighbours, rounds=cluster.dbscan.last_rounds, ms=ms)
    return x


def bench_cpu(args, x):
    from sklearn.cluster import DBSCAN
    xs = x[: args.cpu_n].cpu().numpy()
    t0 = time.perf_counter()
    sk = DBSCAN(eps=args.eps, min_samples=5, metric="cosine", n_jobs=16).fit(xs)
    s = time.perf_counter() - t0
    t0 = time.perf_counter()
    labels, _ = cluster.dbscan(xs, args.eps, 5)
    s_dev = time.perf_counter() - t0
    emit(what="sklearn.cluster.DBSCAN(metric=cosine, n_jobs=16) on the host", n=int(xs.shape[0]), d=args.d, eps=args.eps, seconds=s, clusters=int(sk.labels_.max()) + 1,
         device_seconds_same_rows=s_dev, labels_equal=bool((labels == sk.labels_).all()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--mean", type=float, default=100.0)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--eps", type=float, default=0.4)
    ap.add_argument("--dbscan", default="100000,1000000")
    ap.add_argument("--cpu-n", type=int, default=20000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_range.py measures on the GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    for storage in ("float32", "float16"):
        bench_search(args, dev, storage)
        torch.cuda.empty_cache()
    x = None
    for n in [int(v) for v in args.dbscan.split(",") if v]:
        x = bench_dbscan(args, dev, n)
        torch.cuda.empty_cache()
    if x is not None and args.cpu_n > 0:
        bench_cpu(args, x)
    if args.out:
        with open(args.out, "w") as f:
            for line in LINES:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
