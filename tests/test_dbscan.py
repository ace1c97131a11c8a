"""Cosine DBSCAN on the device (visiondk_amd.cluster.dbscan: exact range search over the L2-normalised rows + the gather kernels of csrc/cbir_range.hip) against
sklearn.cluster.DBSCAN(metric="cosine") on the rows cast to float64: labels equal element for element (the numbering is part of the contract), core sets equal.

The rule the kernels implement is restated here in float64 (`rule`) and asserted equal to sklearn's result, which ties the rule to sklearn and not to the code under test:
core = neighbourhood (the point included) of at least min_samples points; clusters = components of the core points over core-core edges, numbered by their smallest core
index; a non-core point with a core neighbour takes the smallest cluster id among its core neighbours' clusters; everything else is -1.

Precondition, from float64 alone: the device decides a pair on its fp32 score against float32(1 - eps), sklearn on float64.  For fp32-normalised unit rows the two differ by at
most BOUND(D) = (2 D + 8) 2^-24 (the sum of squares, the square root and the division per row, the D-term chain, the rounding of the threshold: derived, not measured), so no
pair's cosine may lie within BOUND of 1 - eps.  The seeds below satisfy it and every test asserts it; a seed that does not is replaced, not dropped.
fp16 storage: the device scores the fp16-ROUNDED normalised rows without normalising them again, sklearn's cosine does normalise them again (their norms are 1 +- 1e-4), so
for that case the precondition is that, for every pair, the float64 inner product AND the float64 cosine of the rounded rows lie on the same side of 1 - eps, both further
than BOUND away; the rounded rows are formed by the library's own normalisation (vdk_l2norm_rows) so that reference and device round the same values.
"""
import functools

import numpy as np
import pytest
import torch
from scipy.sparse.csgraph import connected_components
from sklearn.cluster import DBSCAN as SkDBSCAN

from visiondk_amd import cbir, cluster

F32 = np.float32


def BOUND(d):
    return (2 * d + 8) * 2.0 ** -24


def mixture(seed, n=300, d=16, centres=6, noise_rows=40):
    """6 Gaussian centres, points = centre + 0.45 randn, 40 of them replaced by pure noise rows; float32"""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centres, d))
    x = c[rng.integers(0, centres, n)] + 0.45 * rng.standard_normal((n, d))
    x[rng.choice(n, noise_rows, replace=False)] = rng.standard_normal((noise_rows, d))
    return np.ascontiguousarray(x.astype(F32))


def cosines(x64):
    xn = x64 / np.maximum(np.linalg.norm(x64, axis=1, keepdims=True), 1e-300)
    return xn @ xn.T


def rule(nb, min_samples):
    """the float64 restatement: nb = bool [N, N] neighbourhood matrix (diagonal set) -> labels, core indices, number of border points with core neighbours in two clusters"""
    n = nb.shape[0]
    core = nb.sum(1) >= min_samples
    ci = np.nonzero(core)[0]
    labels = np.full(n, -1, np.int64)
    two = 0
    if ci.size:
        _, comp = connected_components(nb[np.ix_(ci, ci)], directed=False)
        roots = np.array([ci[comp == k].min() for k in range(comp.max() + 1)])        # smallest core index of every component
        order = np.argsort(np.argsort(roots))                                         # cluster id = rank of the root among the roots
        labels[ci] = order[comp]
        for i in np.nonzero(~core)[0]:
            cn = np.nonzero(nb[i] & core)[0]
            if cn.size:
                labels[i] = labels[cn].min()
                two += int(np.unique(labels[cn]).size > 1)
    return labels, ci.astype(np.int64), two


@functools.lru_cache(maxsize=None)
def reference(seed, n, d, eps, min_samples):
    """x, sklearn's labels and core indices (computed once per case), with the precondition and the restatement asserted"""
    x = mixture(seed, n, d)
    x64 = x.astype(np.float64)
    cs = cosines(x64)
    gap = np.abs(cs - (1.0 - eps)).min()
    assert gap > BOUND(d), f"seed {seed}: a pair's cosine lies {gap:.3g} from 1 - eps (bound {BOUND(d):.3g}): take another seed"
    sk = SkDBSCAN(eps=eps, min_samples=min_samples, metric="cosine").fit(x64)
    labels, core, two = rule(cs >= 1.0 - eps, min_samples)
    np.testing.assert_array_equal(labels, sk.labels_)                                 # the rule IS sklearn's
    np.testing.assert_array_equal(core, sk.core_sample_indices_)
    kinds = (core.size > 0, bool(((labels >= 0) & ~np.isin(np.arange(n), core)).any()), bool((labels < 0).any()))
    assert all(kinds), f"core / border / noise present: {kinds}"
    return x, sk.labels_.astype(np.int64), sk.core_sample_indices_.astype(np.int64), two


# (seed, n, d, eps, min_samples): the recipe at D = 16 with eps in {0.15, 0.25} x min_samples in {5, 8}; D = 64, N = 700 crosses a 32-row gallery tile, the 512-query
# workgroup of the filter and the 256-query tiles of the count kernels
# seed 7 at eps 0.15 / min_samples 8 holds a border point whose core neighbours lie in two clusters; at D = 64 and eps 0.15 the 245 k pairs are dense around 1 - eps, seed 208 is
# the first of the recipe whose gap (9.6e-6) clears BOUND(64) = 8.1e-6
CASES = [(0, 300, 16, 0.15, 5), (0, 300, 16, 0.15, 8), (0, 300, 16, 0.25, 5), (0, 300, 16, 0.25, 8), (2, 300, 16, 0.25, 8), (7, 300, 16, 0.15, 8), (208, 700, 64, 0.15, 5)]


@pytest.mark.parametrize("seed,n,d,eps,min_samples", CASES)
def test_dbscan_equals_sklearn(be, dev, seed, n, d, eps, min_samples):
    x, labels, core, _ = reference(seed, n, d, eps, min_samples)
    got_l, got_c = cluster.dbscan(x, eps, min_samples, backend=be, device=dev)
    assert got_l.dtype == np.int64 and got_c.dtype == np.int64
    np.testing.assert_array_equal(got_l, labels)
    np.testing.assert_array_equal(got_c, core)
    again_l, again_c = cluster.dbscan(x, eps, min_samples, backend=be, device=dev)     # the same labels on a second run
    np.testing.assert_array_equal(again_l, got_l)
    np.testing.assert_array_equal(again_c, got_c)


def test_a_border_point_between_two_clusters_is_among_the_cases():
    assert any(reference(*c)[3] > 0 for c in CASES)


def test_class_wrapper_and_tensor_input(be, dev):
    seed, n, d, eps, ms = CASES[0]
    x, labels, core, _ = reference(seed, n, d, eps, ms)
    m = cluster.DBSCAN(eps=eps, min_samples=ms, metric="cosine", n_jobs=16, backend=be, device=dev).fit(x)       # the reference's call, argument for argument
    np.testing.assert_array_equal(m.labels_, labels)
    np.testing.assert_array_equal(m.core_sample_indices_, core)
    tl, tc = cluster.dbscan(torch.from_numpy(x).to(dev), eps, ms, backend=be, device=dev)
    assert isinstance(tl, torch.Tensor) and tl.dtype == torch.int64 and tc.dtype == torch.int64
    np.testing.assert_array_equal(tl.cpu().numpy(), labels)
    np.testing.assert_array_equal(tc.cpu().numpy(), core)


@pytest.mark.parametrize("seed,eps,min_samples", [(13, 0.15, 5), (4, 0.25, 8)])
def test_fp16_storage(be, dev, seed, eps, min_samples):
    n, d = 300, 16
    x = mixture(seed, n, d)
    xh = cbir.l2_normalize(torch.from_numpy(x).to(dev), backend=be).half().cpu().numpy().astype(np.float64)      # the rows the fp16 index holds
    ip, cs = xh @ xh.T, cosines(xh)
    thr = 1.0 - eps
    lo, hi = np.minimum(ip, cs), np.maximum(ip, cs)
    assert bool(((lo - thr > BOUND(d)) | (hi - thr < -BOUND(d))).all()), "a pair's inner product and cosine straddle 1 - eps, or lie within the bound: take another seed"
    sk = SkDBSCAN(eps=eps, min_samples=min_samples, metric="cosine").fit(xh)
    labels, core, _ = rule(cs >= thr, min_samples)
    np.testing.assert_array_equal(labels, sk.labels_)
    assert core.size and bool(((labels >= 0) & ~np.isin(np.arange(n), core)).any()) and bool((labels < 0).any())        # core, border and noise points
    got_l, got_c = cluster.dbscan(x, eps, min_samples, storage="float16", backend=be, device=dev)
    np.testing.assert_array_equal(got_l, sk.labels_)
    np.testing.assert_array_equal(got_c, sk.core_sample_indices_)


def test_min_samples_one_and_tiny_eps(be, dev):
    seed, n, d, eps, _ = CASES[0]
    x = reference(seed, n, d, eps, 5)[0]
    cs = cosines(x.astype(np.float64))
    assert np.abs(cs - (1.0 - eps)).min() > BOUND(d)
    sk = SkDBSCAN(eps=eps, min_samples=1, metric="cosine").fit(x.astype(np.float64))
    got_l, got_c = cluster.dbscan(x, eps, 1, backend=be, device=dev)                   # every point is a core point
    np.testing.assert_array_equal(got_c, np.arange(n))
    np.testing.assert_array_equal(got_l, sk.labels_)
    got_l, got_c = cluster.dbscan(x, 1e-7, 5, backend=be, device=dev)                  # an eps so small that everything is noise
    assert (got_l == -1).all() and got_c.size == 0


def test_other_metrics_are_refused(be, dev):
    x = mixture(0)
    for metric in ("euclidean", "l2", "precomputed"):
        with pytest.raises(ValueError, match="cosine"):
            cluster.dbscan(x, 0.2, 5, metric=metric, backend=be, device=dev)
        with pytest.raises(ValueError, match="cosine"):
            cluster.DBSCAN(eps=0.2, metric=metric, backend=be, device=dev)
