"""Cosine DBSCAN on the device: the reference's tools/clustering.py asks

    clustering = DBSCAN(eps=0.4, min_samples=5, metric="cosine").fit(features)      # sklearn, brute-force N x N distances on the host
    labels = clustering.labels_

of the embeddings hot path B extracts.  Here the neighbourhoods come from the exact range search (cbir.FlatIPIndex.range_search over the L2-normalised rows: cosine
distance <= eps  <=>  inner product >= 1 - eps) and the clustering from the small gather kernels of csrc/cbir_range.hip; the N x N matrix is never formed.

The result is sklearn's `dbscan_inner` result, numbering included: a core point's cluster is the rank of its component's smallest core index, a border point joins the
smallest cluster among its core neighbours, everything else is -1.  A pair counts as neighbours on its fp32 score (the k-ordered fmaf chain of the search) against
float32(1 - eps); sklearn decides on float64 distances, so a pair within rounding of the radius can fall on the other side (tests/test_dbscan.py states the bound).
"""
from __future__ import annotations

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
