"""The minimum spanning tree of the cosine mutual-reachability graph (visiondk_amd.cluster.mutual_reachability_mst: csrc/cbir_mst.hip + the bookkeeping of cluster.py), bit
for bit against an oracle written here: every pair's exact score in the oracle's own bits (oracle.cbir.flat_ip_search with k = N returns all N scores of a row, scattered
back by index as tests/test_cbir_range.py does), from them core, w and a numpy Kruskal under the key (w, min(i, j), max(i, j)).  Under a strict total order the minimum
spanning tree is unique, so u, v, w (as uint32) and core (as uint32) must be EQUAL, on the CPU SIMT emulation and (-m gpu) through the same C ABI on the MI355X.

The unit rows the oracle scores are oracle.cbir.l2norm_rows(x) where the device's normalisation gives the same bits, and the device's own rows otherwise (unit_rows).
"""
import functools
import hashlib
import math

import numpy as np
import pytest
import torch
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from oracle import cbir as ocbir
from tests.test_dbscan import mixture
from visiondk_amd import cbir, cluster

F32 = np.float32


def gaussian(seed, n, d):
    return np.random.default_rng(seed).standard_normal((n, d), dtype=F32)


def near_ties():
    """257 rows = one unit centre + 1e-3 randn at D = 64: every pairwise distance lies inside the bf16 error of every other, so the propose pass must pass nearly
    everything and the exact chain alone decides the order"""
    rng = np.random.default_rng(5)
    c = rng.standard_normal(64)
    c /= np.linalg.norm(c)
    return np.ascontiguousarray((c + 1e-3 * rng.standard_normal((257, 64))).astype(F32))


COPIES = [3, 7, 8, 20, 31, 32, 33, 50, 64, 77, 98, 99]


def duplicates():
    """12 copies of one row among 100: zero weights and index tie-breaks.  The copied row is one whose unit form scores itself at >= 1 (a chain of D products of a unit
    row lands within a few ulp of 1 on either side), so that the distance between two copies is exactly zero"""
    x = gaussian(6, 100, 16)
    self_score = ocbir.flat_ip_search(ocbir.l2norm_rows(x), ocbir.l2norm_rows(x), 1)[0][:, 0]
    src = int(np.nonzero(self_score >= 1)[0][0])
    row = x[src].copy()
    x[src] = gaussian(60, 1, 16)[0]
    x[COPIES] = row
    return x


def two_far_clusters():
    """two tight clusters around c and -c: once each has become one component, both pick the same joining edge in the same round"""
    rng = np.random.default_rng(7)
    c = rng.standard_normal(16)
    x = np.concatenate([c + 0.05 * rng.standard_normal((20, 16)), -c + 0.05 * rng.standard_normal((21, 16))])
    return np.ascontiguousarray(x[rng.permutation(41)].astype(F32))


FIXTURES = {
    "mixture300": lambda: mixture(0, 300, 16),
    "mixture700": lambda: mixture(208, 700, 64),
    **{f"tail{n}": (lambda n=n: gaussian(n, n, 16)) for n in (2, 3, 31, 32, 33, 257)},
    "near_ties": near_ties,
    "duplicates": duplicates,
    "two_far": two_far_clusters,
    # -m gpu only: the 512-query workgroup + 1, one 2048-row mask chunk + 1, and a gallery-like shape
    "tail513": lambda: gaussian(513, 513, 16),
    "tail2049": lambda: gaussian(2049, 2049, 16),
    "mixture5000": lambda: mixture(11, 5000, 128, centres=12, noise_rows=600),
}
EMU_FIXTURES = ["mixture300", "mixture700", "tail2", "tail3", "tail31", "tail32", "tail33", "tail257", "near_ties", "duplicates", "two_far"]
GPU_FIXTURES = ["tail513", "tail2049", "mixture5000"]


ROWS = {"tail2": 2, "tail3": 3}          # (every other fixture has more than 10 rows)


def cases(names):
    return [(name, ms) for name in names for ms in (1, 5, 10) if ms <= ROWS.get(name, 11)]


@functools.lru_cache(maxsize=None)
def rows(name):
    x = FIXTURES[name]()
    x.setflags(write=False)
    return x


_UNIT = {}       # digest -> the unit rows it stands for


def unit_rows(be, dev, x):
    """the rows the oracle scores -> (xn, digest).  oracle.cbir.l2norm_rows(x) where the device's normalisation gives the same bits; the device sums the squares in fp32 in
    its wave's order and the oracle in double, so on most inputs a few elements differ in the last place: then the oracle is fed the device's rows (as
    tests/test_dbscan.py's fp16 case feeds it the rows the index holds), which must lie within 4 ulp of its own"""
    want = ocbir.l2norm_rows(x)
    got = cbir.l2_normalize(torch.from_numpy(x.copy()).to(dev), 1e-12, backend=be).cpu().numpy()
    if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        assert np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max() <= 4
        want = got
    digest = hashlib.sha1(want.tobytes()).hexdigest()
    _UNIT.setdefault(digest, want)
    return want, digest


@functools.lru_cache(maxsize=None)
def pair_scores(digest):
    """every pair's exact score in the oracle's bits, S [N, N] (computed once per set of rows, never modified)"""
    xn = _UNIT[digest]
    n = xn.shape[0]
    so, io = ocbir.flat_ip_search(xn, xn, n)
    S = np.empty((n, n), F32)
    np.put_along_axis(S, io, so, axis=1)
    assert np.array_equal(S.view(np.uint32), S.T.view(np.uint32))             # the chain is symmetric in i, j
    S.setflags(write=False)
    return S


def kruskal(n, iu, ju, order):
    """the edges (iu, ju), visited in `order`, that join two components: union-find, with the edges that already lie inside a component filtered out a block at a time"""
    parent = np.arange(n)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    picked, at, step = [], 0, 4096
    while len(picked) < n - 1:
        blk = order[at:at + step]
        at += step
        assert blk.size, "the graph is complete: Kruskal cannot run out of edges"
        roots = parent.copy()
        for _ in range(64):
            nxt = roots[roots]
            if np.array_equal(nxt, roots):
                break
            roots = nxt
        for e in blk[roots[iu[blk]] != roots[ju[blk]]]:
            a, b = find(iu[e]), find(ju[e])
            if a != b:
                parent[a] = b
                picked.append(e)
        step *= 2
    return np.array(picked[:n - 1], np.int64)


@functools.lru_cache(maxsize=None)
def oracle_tree(digest, min_samples):
    S = pair_scores(digest)
    n = S.shape[0]
    t = np.sort(S, axis=1)[:, n - min_samples]                                  # the min_samples-th largest entry of the row, the self pair included
    core = np.maximum(F32(0), F32(1) - t).astype(F32)
    iu, ju = np.triu_indices(n, 1)
    w = np.maximum(np.maximum(core[iu], core[ju]), np.maximum(F32(0), F32(1) - S[iu, ju])).astype(F32)
    order = np.lexsort((ju, iu, w))                                            # the key (w, min, max); iu < ju
    e = kruskal(n, iu, ju, order)
    return iu[e].astype(np.int64), ju[e].astype(np.int64), w[e], core


def check(be, dev, name, ms):
    x = rows(name)
    n = x.shape[0]
    _, digest = unit_rows(be, dev, x)
    want = oracle_tree(digest, ms)
    u, v, w, core = cluster.mutual_reachability_mst(x.copy(), ms, backend=be, device=dev)
    rounds = cluster.mutual_reachability_mst.last_rounds
    assert u.dtype == np.int64 and v.dtype == np.int64 and w.dtype == F32 and core.dtype == F32
    # what holds whatever the oracle says: N - 1 edges u < v, one component, sorted by the key
    assert u.shape == v.shape == w.shape == (n - 1,) and core.shape == (n,)
    assert (u < v).all() and (u >= 0).all() and (v < n).all()
    ncomp, _ = connected_components(coo_matrix((np.ones(n - 1), (u, v)), shape=(n, n)), directed=False)
    assert ncomp == 1
    np.testing.assert_array_equal(np.lexsort((v, u, w)), np.arange(n - 1))
    assert 1 <= rounds <= max(1, math.ceil(math.log2(n)))
    # the oracle's tree, bit for bit
    np.testing.assert_array_equal(core.view(np.uint32), want[3].view(np.uint32))
    np.testing.assert_array_equal(u, want[0])
    np.testing.assert_array_equal(v, want[1])
    np.testing.assert_array_equal(w.view(np.uint32), want[2].view(np.uint32))
    again = cluster.mutual_reachability_mst(x.copy(), ms, backend=be, device=dev)                  # the same bits on a second call
    for a, b in zip((u, v, w, core), again):
        np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == F32 else a, b.view(np.uint32) if b.dtype == F32 else b)
    return u, v, w, core


@pytest.mark.parametrize("name,ms", cases(EMU_FIXTURES))
def test_tree_bit_exact(be, dev, name, ms):
    check(be, dev, name, ms)


@pytest.mark.gpu
@pytest.mark.parametrize("name,ms", cases(GPU_FIXTURES))
def test_tree_bit_exact_large(hip, name, ms):
    check(hip, "cuda", name, ms)


def test_duplicates_give_zero_weights_and_index_ties(be, dev):
    u, v, w, core = check(be, dev, "duplicates", 5)
    copies = COPIES
    assert (core[copies] == 0).all()                                            # 12 copies: the fifth nearest is a copy
    z = w == 0
    assert z.sum() == 11 and (u[z] == 3).all() and v[z].tolist() == copies[1:]  # among equal zero weights the smallest (u, v) win: a star around the first copy


def test_near_ties_are_ties_for_the_prefilter(be, dev):
    S = pair_scores(unit_rows(be, dev, rows("near_ties"))[1])
    off = S[~np.eye(257, dtype=bool)]
    # all scores within 2e-4 of each other: far inside the band of the bf16 scores of unit rows (two operands rounded to 8 bits: ~2 * 2^-9 = 4e-3), yet many distinct values
    assert off.max() - off.min() < 2e-4 and np.unique(off).size > 50


def test_two_far_clusters_join_by_one_edge(be, dev):
    x = rows("two_far")
    u, v, w, _ = check(be, dev, "two_far", 1)
    side = x @ x[0] > 0
    across = side[u] != side[v]
    assert across.sum() == 1 and across[-1] and w[-1] > 1.5                     # one joining edge, the heaviest: both components picked it in the last round


def test_row_blocks(be, dev, monkeypatch):
    """a bit-matrix cap small enough that the 700 rows go through two blocks: the same tree"""
    monkeypatch.setattr(cluster, "MST_MASK_BYTES", 1)       # -> the minimum block of 512 rows
    check(be, dev, "mixture700", 5)


def test_tensor_in_tensor_out_and_refusals(be, dev):
    x = rows("tail33").copy()
    want = oracle_tree(unit_rows(be, dev, x)[1], 5)
    out = cluster.mutual_reachability_mst(torch.from_numpy(x).to(dev), 5, backend=be, device=dev)
    assert all(isinstance(t, torch.Tensor) and t.device.type == torch.device(dev).type for t in out)
    assert [t.dtype for t in out] == [torch.int64, torch.int64, torch.float32, torch.float32]
    for a, b in zip(out, want):
        np.testing.assert_array_equal(a.cpu().numpy(), b)
    for bad in (x[:1], ):
        with pytest.raises(ValueError):
            cluster.mutual_reachability_mst(bad, 1, backend=be, device=dev)
    with pytest.raises(ValueError):
        cluster.mutual_reachability_mst(x, 34, backend=be, device=dev)
    with pytest.raises(ValueError):
        cluster.mutual_reachability_mst(x, 0, backend=be, device=dev)
    with pytest.raises(ValueError):
        cluster.mutual_reachability_mst(np.zeros((4, 516), F32), 1, backend=be, device=dev)
    nan = x.copy()
    nan[5, 3] = np.nan
    with pytest.raises(ValueError):
        cluster.mutual_reachability_mst(nan, 5, backend=be, device=dev)
    with pytest.raises(TypeError):
        cluster.mutual_reachability_mst(x.astype(np.float64), 5, backend=be, device=dev)
