"""Cosine DBSCAN and HDBSCAN on the device (HDBSCAN: the second half of this file, with its contract).  The reference's tools/clustering.py asks

    clustering = DBSCAN(eps=0.4, min_samples=5, metric="cosine").fit(features)      # sklearn, brute-force N x N distances on the host
    labels = clustering.labels_

of the embeddings hot path B extracts.  Here the neighbourhoods come from the exact range search (cbir.FlatIPIndex.range_search over the L2-normalised rows: cosine
distance <= eps  <=>  inner product >= 1 - eps) and the clustering from the small gather kernels of csrc/cbir_range.hip; the N x N matrix is never formed.

The result is sklearn's `dbscan_inner` result, numbering included: a core point's cluster is the rank of its component's smallest core index, a border point joins the
smallest cluster among its core neighbours, everything else is -1.  A pair counts as neighbours on its fp32 score (the k-ordered fmaf chain of the search) against
float32(1 - eps); sklearn decides on float64 distances, so a pair within rounding of the radius can fall on the other side (tests/test_dbscan.py states the bound).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib, cbir


def dbscan(x, eps: float, min_samples: int = 5, metric: str = "cosine", storage: str = "float32", backend: Optional[_lib.Backend] = None, device=None,
           max_results: Optional[int] = None):
    """-> (labels int64 [N], core_sample_indices int64 [n_core]); x float32 [N, D], numpy (numpy out) or tensor (tensors on the device out).
    storage: how the self-search keeps the normalised rows ("float32" | "float16", as cbir.FlatIPIndex); max_results bounds the neighbourhood CSR (RuntimeError with the
    exact total otherwise).  D <= 512."""
    if metric != "cosine":
        raise ValueError(f"dbscan: only metric=\"cosine\" is served, got {metric!r}")
    if int(min_samples) < 1:
        raise ValueError("dbscan: min_samples >= 1")
    as_numpy = isinstance(x, np.ndarray)
    if as_numpy:
        if x.dtype != np.float32:
            raise TypeError("dbscan expects float32 rows")
        x = torch.from_numpy(np.ascontiguousarray(x))
    if x.dtype != torch.float32 or x.dim() != 2:
        raise ValueError("dbscan expects a float32 [N, D] matrix")
    be = backend or _lib.load()
    index = cbir.FlatIPIndex(x.shape[1], backend=be, device=device, storage=storage)
    dev = index.device
    n = x.shape[0]
    xn = cbir.l2_normalize(x.to(dev).contiguous(), 1e-12, backend=be) if n else x.to(dev)
    index.add(xn)
    lims, _, nbr = index.range_search(xn, float(np.float32(1.0 - float(eps))), inclusive=True, max_results=max_results)
    labels, core, rounds = _dbscan_csr(be, lims, nbr, n, int(min_samples), dev)
    dbscan.last_rounds = rounds                       # propagation rounds of the last call (tools/bench_range.py reports it)
    dbscan.last_mean_neighbours = float(nbr.numel()) / max(n, 1)
    core_idx = torch.nonzero(core).reshape(-1)
    if as_numpy:
        return labels.cpu().numpy(), core_idx.cpu().numpy()
    return labels, core_idx


def _dbscan_csr(be, lims: torch.Tensor, nbr: torch.Tensor, n: int, min_samples: int, dev):
    """labels, core flags and the number of propagation rounds from a neighbourhood CSR on the device"""
    core = torch.empty(n, dtype=torch.uint8, device=dev)
    lab = [torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)]
    out = torch.empty(n, dtype=torch.int64, device=dev)
    if n == 0:
        return out, core, 0
    st = be.stream()
    pn = be.ptr(nbr) if nbr.numel() else None
    be.check(be.lib.vdk_dbscan_core(be.ptr(lims), n, min_samples, be.ptr(core), be.ptr(lab[0]), st), "vdk_dbscan_core")
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    rounds, cur = 0, 0
    while True:
        flag.zero_()
        be.check(be.lib.vdk_dbscan_round(be.ptr(lims), pn, n, be.ptr(core), be.ptr(lab[cur]), be.ptr(lab[1 - cur]), be.ptr(flag), st), "vdk_dbscan_round")
        cur = 1 - cur
        rounds += 1
        if int(flag.item()) == 0:                     # one flag read per round
            break
    label = lab[cur]
    root = (core != 0) & (label == torch.arange(n, dtype=torch.int32, device=dev))
    rank = (torch.cumsum(root.to(torch.int32), 0, dtype=torch.int32) - root.to(torch.int32)).contiguous()      # exclusive prefix sum of the root mask
    be.check(be.lib.vdk_dbscan_assign(be.ptr(lims), pn, n, be.ptr(core), be.ptr(label), be.ptr(rank), be.ptr(out), st), "vdk_dbscan_assign")
    return out, core, rounds


class DBSCAN:
    """sklearn.cluster.DBSCAN's surface as tools/clustering.py uses it: DBSCAN(eps, min_samples, metric="cosine").fit(X) -> labels_, core_sample_indices_ (numpy)."""

    def __init__(self, eps: float = 0.5, min_samples: int = 5, metric: str = "cosine", n_jobs=None, storage: str = "float32", backend: Optional[_lib.Backend] = None, device=None,
                 max_results: Optional[int] = None):
        """n_jobs (tools/clustering.py passes 16: sklearn's host threads) is accepted and has no meaning here"""
        if metric != "cosine":
            raise ValueError(f"DBSCAN: only metric=\"cosine\" is served, got {metric!r}")
        self.eps, self.min_samples, self.metric, self.storage = eps, min_samples, metric, storage
        self._backend, self._device, self._max_results = backend, device, max_results
        self.labels_ = None
        self.core_sample_indices_ = None

    def fit(self, X, y=None):
        X = np.ascontiguousarray(np.asarray(X, dtype=np.float32))
        self.labels_, self.core_sample_indices_ = dbscan(X, self.eps, self.min_samples, self.metric, self.storage, self._backend, self._device, self._max_results)
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_


# ------------------------------------------------------------------------------------ HDBSCAN
# The commented alternative of tools/clustering.py:
#     db = HDBSCAN(min_cluster_size = 10, min_samples = 5, cluster_selection_epsilon = 0.2, metric = "cosine", n_jobs = 16).fit(X)
#
# Contract (DESIGN.md section 3 "HDBSCAN").  Rows xn = cbir.l2_normalize(x, 1e-12); every quantity fp32 with one bit pattern per input:
#   s_ij    the exact score, the k-ordered fmaf chain of the search (symmetric in i, j);       d_ij = max(0, 1.0f - s_ij);
#   core_i  max(0, 1.0f - t_i), t_i = the min_samples-th largest entry of row i of s, the self pair included with its own chain score (sklearn's k-th smallest distance
#           counts the point itself in the same way);                                           w_ij = max(core_i, core_j, d_ij), i != j;
#   edges are ordered by the strict, total key (w, min(i, j), max(i, j)), and THE TREE IS THE UNIQUE MINIMUM SPANNING TREE UNDER THAT ORDER: what Kruskal builds from the
#   edges sorted by the key, and what Boruvka builds when every component picks its smallest outgoing edge under the key.  Output: N - 1 edges (u < v, w) sorted by the key.
# Labels and probabilities are what sklearn's tree_to_labels returns for make_single_linkage of those edges IN THAT ORDER, weights widened to float64, with
# cluster_selection_method="eom", allow_single_cluster=False, max_cluster_size=None, alpha=1.0; the numbering is part of the contract.  sklearn is not imported: the tree
# code is restated below (tests/test_hdbscan_tree.py holds it against sklearn's on tie-laden trees).  sklearn.cluster.HDBSCAN.fit itself inherits the order of its Prim
# walk and of an unstable argsort among the many exactly equal weights of a mutual-reachability graph, so label-for-label equality with it is not a property it has with
# itself; tests/test_hdbscan.py states the cap (adjusted Rand index, cluster count, noise status) and shows that sklearn's own tree code under two tie orders meets it too.
#
# Device part (csrc/cbir_mst.hip): the core distances are the last column of the top-k self-search; a Boruvka round is the row scan vdk_mst_scan (bf16-MFMA bound and
# propose passes, exact decide pass, one bit per pair) over row blocks, then O(N log N) bookkeeping in torch ops on the device (two stable sorts, gathers, a prefix sum,
# pointer jumps: no atomics, the same bits on every run) and ONE host read, the number of components left.  The loop is bounded: more than ceil(log2 N) rounds raise.

MST_MASK_BYTES = 1 << 30    # cap of the one-bit-per-pair matrix of a row block (rows N / 8 bytes): the rows are walked in blocks of whole 512-row workgroups under it


def _rows_on_device(x, who: str):
    as_numpy = isinstance(x, np.ndarray)
    if as_numpy:
        if x.dtype != np.float32:
            raise TypeError(f"{who} expects float32 rows")
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2:
        raise ValueError(f"{who} expects a float32 [N, D] matrix")
    return x, as_numpy


def _mst_device(x: torch.Tensor, min_samples: int, be, device):
    """-> u, v int64 [N - 1], w float32 [N - 1], core float32 [N] on the device, and the number of rounds"""
    n, d = x.shape
    if n < 2:
        raise ValueError("mutual_reachability_mst: at least two rows")
    if not 1 <= min_samples <= n:
        raise ValueError(f"mutual_reachability_mst: 1 <= min_samples <= N = {n}, got {min_samples}")
    if min_samples > 1024:
        raise ValueError("mutual_reachability_mst: min_samples <= 1024 (the top-k search's k)")
    if d > 512:
        raise ValueError("mutual_reachability_mst: D <= 512")
    if n >= 1 << 31:
        raise ValueError("mutual_reachability_mst: N < 2^31")
    index = cbir.FlatIPIndex(d, backend=be, device=device)
    dev = index.device
    hook = _mst_device.on_stage
    x = x.to(dev).contiguous()
    if not bool(torch.isfinite(x).all().item()):                 # (one host read)
        raise ValueError("mutual_reachability_mst: the rows hold a NaN or an infinity")
    xn = cbir.l2_normalize(x, 1e-12, backend=be)
    index.add(xn)
    xp = index._materialize()                                   # the unit rows, zero-padded to D % 4 == 0 (exact zeros: the chain's bits do not change)
    dp = xp.shape[1]
    lib, p, st = be.lib, be.ptr, be.stream()
    # the bf16 copy and the error norms, once for the self-search and for every round (the index keeps no row norms, the scan needs them: the rows are their own queries)
    gb = torch.empty((n, (dp + 127) // 128 * 128), dtype=torch.bfloat16, device=dev)
    gnorm = torch.empty(3 * n, dtype=torch.float32, device=dev)
    gmax = torch.zeros(4, dtype=torch.int32, device=dev)
    be.check(lib.vdk_cbir_prepare_gallery(p(xp), n, dp, p(gb), p(gnorm), p(gmax), st), "vdk_cbir_prepare_gallery")
    index._gb, index._gmax = gb, gmax
    if hook is not None:
        hook("prepare", 0, None)
    top, _ = index.search(xn, min_samples)
    core = torch.clamp(1.0 - top[:, min_samples - 1], min=0.0).contiguous()
    if hook is not None:
        hook("core", 0, None)
    words = (n + 31) // 32
    blk = min(n, max(512, MST_MASK_BYTES // (4 * words) // 512 * 512))
    need = C.c_size_t(0)
    be.check(lib.vdk_mst_scan_workspace_bytes(blk, n, dp, C.byref(need)), "vdk_mst_scan_workspace_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    _mst_device.last_workspace_bytes = need.value
    ar = torch.arange(n, dtype=torch.int64, device=dev)
    comp = ar.to(torch.int32)
    best_w = torch.empty(n, dtype=torch.float32, device=dev)
    best_j = torch.empty(n, dtype=torch.int32, device=dev)
    eu, ev = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev)      # N - 1 edges; slot N - 1 takes the writes of non-edges
    ew = torch.empty(n, dtype=torch.float32, device=dev)
    ncomp, rounds, max_rounds = n, 0, (n - 1).bit_length()       # ceil(log2 N): every round at least halves the components
    while ncomp > 1:
        if rounds == max_rounds:
            raise RuntimeError(f"mutual_reachability_mst: {ncomp} components left after ceil(log2 N) = {max_rounds} rounds")
        for q0 in range(0, n, blk):
            nq = min(blk, n - q0)
            be.check(lib.vdk_mst_scan(p(xp), p(gb), p(gnorm), p(gmax), p(core), p(comp), n, dp, q0, nq, p(best_w), p(best_j), p(ws), ws.numel(), st), "vdk_mst_scan")
        if hook is not None:
            hook("scan", rounds, dict(ws=ws, rows=nq, n=n, d=dp))          # (the workspace holds the last block's bit matrix)
        # per component the smallest key among its rows: rows sorted by (comp, w, min, max); w >= 0, so its bit pattern orders like the value
        cl, bj = comp.long(), best_j.long()
        a, b = torch.minimum(ar, bj), torch.maximum(ar, bj)
        o = torch.argsort(a * n + b, stable=True)
        o = o[torch.argsort(((cl << 32) | best_w.view(torch.int32).long())[o], stable=True)]
        cs = cl[o]
        head = torch.ones(n, dtype=torch.bool, device=dev)
        head[1:] = cs[1:] != cs[:-1]
        # hook: component c -> the component its edge leads to.  Under a strict total order the chosen edges hold no cycle but the pairs that chose the SAME edge; of
        # such a pair the smaller label becomes the root and the larger one's copy of the edge is dropped
        parent = torch.arange(n + 1, dtype=torch.int64, device=dev)
        parent[torch.where(head, cs, n)] = torch.where(head, cl[bj[o]], n)
        parent = parent[:n]
        mutual = (parent[parent] == ar) & (parent != ar)
        root = mutual & (ar < parent)
        drop = mutual & (ar > parent)
        parent = torch.where(root, ar, parent)
        keep = head & ~drop[cs]
        pos = torch.where(keep, (n - ncomp) + torch.cumsum(keep, 0) - 1, n - 1)
        eu[pos], ev[pos], ew[pos] = a[o], b[o], best_w[o]
        for _ in range(ncomp.bit_length()):                      # pointer jumps: the hooked forest is at most ncomp deep
            parent = parent[parent]
        comp = parent[cl].to(torch.int32).contiguous()
        left = int(root.sum().item())                            # the one host read of the round: every tree of the hooked forest holds exactly one such pair
        if not 1 <= left <= ncomp // 2:
            raise RuntimeError(f"mutual_reachability_mst: a round went from {ncomp} to {left} components")
        ncomp = left
        rounds += 1
        if hook is not None:
            hook("bookkeeping", rounds - 1, dict(components=ncomp))
    eu, ev, ew = eu[:n - 1], ev[:n - 1], ew[:n - 1]
    o = torch.argsort(eu * n + ev, stable=True)
    o = o[torch.argsort(ew.view(torch.int32)[o], stable=True)]
    return eu[o].contiguous(), ev[o].contiguous(), ew[o].contiguous(), core, rounds


_mst_device.on_stage = None             # tools/bench_hdbscan.py: called as (stage, round, info) after "prepare", "core" and every round's "scan" and "bookkeeping"
_mst_device.last_workspace_bytes = 0


def mutual_reachability_mst(x, min_samples: int, backend: Optional[_lib.Backend] = None, device=None):
    """-> (u int64 [N - 1], v int64 [N - 1], w float32 [N - 1], core float32 [N]): the unique minimum spanning tree of the cosine mutual-reachability graph under the key
    (w, u, v), u < v, sorted by it (the contract above).  x float32 [N, D], N >= 2, D <= 512, 1 <= min_samples <= min(N, 1024) (the top-k search's k): numpy (numpy out) or
    tensor (tensors on the device out).  Sets .last_rounds, the number of Boruvka rounds of the last call."""
    x, as_numpy = _rows_on_device(x, "mutual_reachability_mst")
    be = backend or _lib.load()
    u, v, w, core, rounds = _mst_device(x, int(min_samples), be, device)
    mutual_reachability_mst.last_rounds = rounds
    if as_numpy:
        return u.cpu().numpy(), v.cpu().numpy(), w.cpu().numpy(), core.cpu().numpy()
    return u, v, w, core


def hdbscan(x, min_cluster_size: int = 5, min_samples: Optional[int] = None, cluster_selection_epsilon: float = 0.0, metric: str = "cosine", alpha: float = 1.0,
            cluster_selection_method: str = "eom", allow_single_cluster: bool = False, max_cluster_size: Optional[int] = None, store_centers=None,
            backend: Optional[_lib.Backend] = None, device=None):
    """-> (labels int64 [N], probabilities float64 [N]); x float32 [N, D], numpy (numpy out) or tensor (tensors on the device out).  min_samples=None means
    min_cluster_size, as in sklearn.  Only the cosine metric and sklearn's default selection are served: any other knob set to a non-default value is a ValueError."""
    if metric != "cosine":
        raise ValueError(f"hdbscan: only metric=\"cosine\" is served, got {metric!r}")
    if float(alpha) != 1.0 or cluster_selection_method != "eom" or allow_single_cluster or max_cluster_size is not None or store_centers is not None:
        raise ValueError("hdbscan: alpha, cluster_selection_method, allow_single_cluster, max_cluster_size and store_centers are served at sklearn's defaults only")
    if int(min_cluster_size) < 2:
        raise ValueError("hdbscan: min_cluster_size >= 2")
    if float(cluster_selection_epsilon) < 0.0 or cluster_selection_epsilon != cluster_selection_epsilon:
        raise ValueError("hdbscan: cluster_selection_epsilon >= 0")
    ms = int(min_cluster_size) if min_samples is None else int(min_samples)
    if ms < 1:
        raise ValueError("hdbscan: min_samples >= 1")
    x, as_numpy = _rows_on_device(x, "hdbscan")
    n = x.shape[0]
    if n < 2:
        raise ValueError("hdbscan: at least two rows")
    if ms > n:
        raise ValueError(f"hdbscan: min_samples ({ms}) must be at most the number of rows ({n})")
    be = backend or _lib.load()
    u, v, w, core, rounds = _mst_device(x, ms, be, device)
    mutual_reachability_mst.last_rounds = rounds
    labels, prob = tree_to_labels(u.cpu().numpy(), v.cpu().numpy(), w.cpu().numpy().astype(np.float64), int(min_cluster_size), float(cluster_selection_epsilon))
    if as_numpy:
        return labels, prob
    return torch.from_numpy(labels).to(core.device), torch.from_numpy(prob).to(core.device)


class HDBSCAN:
    """sklearn.cluster.HDBSCAN's surface as tools/clustering.py's commented call uses it: HDBSCAN(min_cluster_size, min_samples, cluster_selection_epsilon, metric="cosine",
    n_jobs).fit(X) -> labels_, probabilities_ (numpy)."""

    def __init__(self, min_cluster_size: int = 5, min_samples: Optional[int] = None, cluster_selection_epsilon: float = 0.0, max_cluster_size: Optional[int] = None,
                 metric: str = "cosine", alpha: float = 1.0, cluster_selection_method: str = "eom", allow_single_cluster: bool = False, store_centers=None, n_jobs=None,
                 backend: Optional[_lib.Backend] = None, device=None):
        """n_jobs (sklearn's host threads) is accepted and has no meaning here"""
        if metric != "cosine":
            raise ValueError(f"HDBSCAN: only metric=\"cosine\" is served, got {metric!r}")
        self.min_cluster_size, self.min_samples, self.cluster_selection_epsilon, self.metric = min_cluster_size, min_samples, cluster_selection_epsilon, metric
        self.max_cluster_size, self.alpha, self.cluster_selection_method = max_cluster_size, alpha, cluster_selection_method
        self.allow_single_cluster, self.store_centers = allow_single_cluster, store_centers
        self._backend, self._device = backend, device
        self.labels_ = None
        self.probabilities_ = None

    def fit(self, X, y=None):
        X = np.ascontiguousarray(np.asarray(X, dtype=np.float32))
        self.labels_, self.probabilities_ = hdbscan(X, self.min_cluster_size, self.min_samples, self.cluster_selection_epsilon, self.metric, self.alpha,
                                                    self.cluster_selection_method, self.allow_single_cluster, self.max_cluster_size, self.store_centers,
                                                    self._backend, self._device)
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_


# ---- the host tree code: sklearn/cluster/_hdbscan (_linkage.pyx make_single_linkage, _tree.pyx tree_to_labels; BSD-3-Clause) restated in plain Python, statement order and
# float64 operation order kept wherever a result can depend on them (the stability sums, the runs of max_lambdas, the iteration order of the epsilon search's set)
_INF = float("inf")


def _single_linkage(u, v, w):
    """union-find single linkage of the edges IN THE GIVEN ORDER -> left, right, value, size per merge; merge i creates node N + i"""
    n = len(u) + 1
    parent = list(range(2 * n - 1))
    size = [1] * n + [0] * (n - 1)
    left, right, value, csize = [0] * (n - 1), [0] * (n - 1), [0.0] * (n - 1), [0] * (n - 1)

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r
    for i in range(n - 1):
        a, b = find(u[i]), find(v[i])
        left[i], right[i], value[i], csize[i] = a, b, w[i], size[a] + size[b]
        parent[a] = parent[b] = n + i
        size[n + i] = csize[i]
    return left, right, value, csize


def _bfs_hierarchy(left, right, n, root):
    out, k = [root], 0
    while k < len(out):
        x = out[k]
        k += 1
        if x >= n:
            out.append(left[x - n])
            out.append(right[x - n])
    return out


def _condense(left, right, value, csize, min_cluster_size):
    """-> parent, child, lambda, size lists of the condensed tree (the root cluster is N, new clusters are numbered as they split off, in breadth-first order)"""
    n = len(left) + 1
    root = 2 * (n - 1)
    relabel = [0] * (root + 1)
    relabel[root] = n
    next_label = n + 1
    ignore = [False] * (root + 1)
    cp, cc, cl, cz = [], [], [], []
    for node in _bfs_hierarchy(left, right, n, root):
        if ignore[node] or node < n:
            continue
        lf, rt, dist = left[node - n], right[node - n], value[node - n]
        lam = 1.0 / dist if dist > 0.0 else _INF
        lcount = csize[lf - n] if lf >= n else 1
        rcount = csize[rt - n] if rt >= n else 1
        me = relabel[node]
        if lcount >= min_cluster_size and rcount >= min_cluster_size:
            for side, count in ((lf, lcount), (rt, rcount)):
                relabel[side] = next_label
                next_label += 1
                cp.append(me); cc.append(relabel[side]); cl.append(lam); cz.append(count)
            continue
        if lcount >= min_cluster_size:
            relabel[lf] = me
            fall = (rt,)
        elif rcount >= min_cluster_size:
            relabel[rt] = me
            fall = (lf,)
        else:
            fall = (lf, rt)
        for side in fall:
            for sub in _bfs_hierarchy(left, right, n, side):
                if sub < n:
                    cp.append(me); cc.append(sub); cl.append(lam); cz.append(1)
                ignore[sub] = True
    return cp, cc, cl, cz


def _stability(cp, cc, cl, cz):
    smallest = min(cp)
    births = [float("nan")] * (max(max(cc), smallest) + 1)
    for k in range(len(cp)):
        births[cc[k]] = cl[k]
    births[smallest] = 0.0
    result = [0.0] * (max(cp) - smallest + 1)
    for k in range(len(cp)):
        result[cp[k] - smallest] += (cl[k] - births[cp[k]]) * cz[k]
    return {k + smallest: result[k] for k in range(len(result))}


def tree_to_labels(u, v, w, min_cluster_size: int = 5, cluster_selection_epsilon: float = 0.0):
    """labels int64 [N] and probabilities float64 [N] from N - 1 spanning-tree edges (u, v, w float64), merged in the given order: excess-of-mass selection with the
    epsilon merge, allow_single_cluster=False, max_cluster_size=None"""
    u, v, w = [int(t) for t in u], [int(t) for t in v], [float(t) for t in w]
    n = len(u) + 1
    cp, cc, cl, cz = _condense(*_single_linkage(u, v, w), int(min_cluster_size))
    stability = _stability(cp, cc, cl, cz)
    node_list = sorted(stability.keys(), reverse=True)[:-1]                  # (the root is excluded)
    tk = [k for k in range(len(cp)) if cz[k] > 1]                           # the cluster tree: the condensed edges between clusters
    tp, tc = [cp[k] for k in tk], [cc[k] for k in tk]
    lam_of, parent_of, kids = {cc[k]: cl[k] for k in tk}, {cc[k]: cp[k] for k in tk}, {}
    for a, b in zip(tp, tc):
        kids.setdefault(a, []).append(b)

    def below(node):                                                        # the clusters of node's subtree, breadth first, node included
        out, k = [node], 0
        while k < len(out):
            out.extend(kids.get(out[k], ()))
            k += 1
        return out
    is_cluster = {c: True for c in node_list}
    for node in node_list:
        sub = 0.0
        for c in kids.get(node, ()):
            sub += stability[c]
        if sub > stability[node]:
            is_cluster[node] = False
            stability[node] = sub
        else:
            for s in below(node):
                if s != node:
                    is_cluster[s] = False
    eps = float(cluster_selection_epsilon)
    if eps != 0.0 and tk:
        eom = [c for c in is_cluster if is_cluster[c]]
        troot = min(tp)
        selected = set()
        if not (len(eom) == 1 and eom[0] == troot):
            inv = lambda lam: _INF if lam == 0.0 else 1.0 / lam
            chosen, processed = [], set()
            for leaf in set(eom):                                           # (sklearn walks a set of these ints built in this order: the same iteration order)
                if inv(lam_of[leaf]) < eps:
                    if leaf not in processed:
                        node = leaf
                        while True:                                         # climb to the first ancestor born at a distance above eps, or to the child of the root
                            par = parent_of[node]
                            if par == troot:
                                break
                            node = par
                            if inv(lam_of[par]) > eps:
                                break
                        chosen.append(node)
                        processed.update(s for s in below(node) if s != node)
                else:
                    chosen.append(leaf)
            selected = set(chosen)
        for c in is_cluster:
            is_cluster[c] = c in selected
    clusters = sorted(c for c in is_cluster if is_cluster[c])
    number = {c: k for k, c in enumerate(clusters)}
    # labelling: a condensed node belongs to the nearest selected cluster above it (sklearn's union-find over the unselected edges, whose representative is always the
    # top of a set: every child is fresh when it is joined to its parent's set), the root's own set is noise
    top = [n] * (max(max(cp), max(cc), n) + 1)
    for k in range(len(cp)):
        top[cc[k]] = cc[k] if cc[k] in number else top[cp[k]]
    labels = np.full(n, -1, np.int64)
    for i in range(n):
        if top[i] != n:
            labels[i] = number[top[i]]
    # probabilities: lambda of the point over the lambda at which its cluster dies -- the maximum of the LAST run of condensed edges with that parent, as max_lambdas has it
    deaths = [0.0] * (max(cp) + 1)
    cur, mx = cp[0], cl[0]
    for k in range(1, len(cp)):
        if cp[k] == cur:
            mx = max(mx, cl[k])
        else:
            deaths[cur] = mx
            cur, mx = cp[k], cl[k]
    deaths[cur] = mx
    prob = np.zeros(n, np.float64)
    for k in range(len(cp)):
        i = cc[k]
        if i >= n or labels[i] < 0:
            continue
        mx = deaths[clusters[labels[i]]]
        prob[i] = 1.0 if (mx == 0.0 or cl[k] == _INF) else min(cl[k], mx) / mx
    return labels, prob
