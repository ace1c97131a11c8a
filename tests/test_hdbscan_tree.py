"""The host tree code of visiondk_amd.cluster (single linkage in the given edge order, condensed tree, stabilities, excess-of-mass selection with the epsilon merge, labels
and probabilities) against sklearn's own: tree_to_labels(make_single_linkage(mst), min_cluster_size, "eom", False, epsilon, None).  No backend is involved.

Labels must be equal element for element (the numbering included); probabilities within rtol = 1e-12: they are two float64 divisions of exactly widened weights, so the bound
is loose by three orders of magnitude on purpose.  The trees are seeded random spanning trees whose weights come from a handful of small integers, zeros included, so that
most weights tie and the order of the edges decides the dendrogram."""
import functools
import warnings

import numpy as np
import pytest
from sklearn.cluster._hdbscan._linkage import MST_edge_dtype, make_single_linkage
from sklearn.cluster._hdbscan._tree import tree_to_labels as sk_tree_to_labels

from visiondk_amd import cluster

WEIGHTS = np.array([0.0, 1.0, 2.0, 3.0, 5.0, 8.0])
EPS_BETWEEN = 2.5                     # between the weights 2 and 3
PARAMS = [(mcs, eps) for mcs in (2, 5, 10) for eps in (0.0, EPS_BETWEEN)]


def sk_labels(u, v, w, mcs, eps):
    mst = np.zeros(len(u), dtype=MST_edge_dtype)
    mst["current_node"], mst["next_node"], mst["distance"] = u, v, w
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")                   # (sklearn's own array-to-scalar conversions)
        labels, prob = sk_tree_to_labels(make_single_linkage(mst), mcs, "eom", False, float(eps), None)
    return np.asarray(labels, np.int64), np.asarray(prob, np.float64)


def random_tree(seed):
    """a random spanning tree on N in [2, 200] points (every point hangs off an earlier one, under a random relabelling), weights from WEIGHTS, the edges in a random
    order that is NOT sorted by weight for a third of the seeds (the code must follow the order it is given) and sorted by (w, u, v) otherwise"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 201))
    perm = rng.permutation(n)
    a = perm[np.arange(1, n)]
    b = perm[(rng.random(n - 1) * np.arange(1, n)).astype(np.int64)]
    u, v = np.minimum(a, b), np.maximum(a, b)
    # clustered weights: edges inside a block of consecutive attachment steps are light, the others heavy, so that real clusters exist
    w = np.where(rng.random(n - 1) < 0.8, rng.choice(WEIGHTS[:4], n - 1), rng.choice(WEIGHTS[3:], n - 1))
    if seed % 3 == 0:
        order = rng.permutation(n - 1)
    else:
        order = np.lexsort((v, u, w))
    return u[order].astype(np.int64), v[order].astype(np.int64), w[order].astype(np.float64)


@functools.lru_cache(maxsize=None)
def outcomes():
    """every (seed, parameter set) once: (ours, sklearn's)"""
    out = []
    for seed in range(200):
        u, v, w = random_tree(seed)
        for mcs, eps in PARAMS:
            out.append((seed, mcs, eps, cluster.tree_to_labels(u, v, w, mcs, eps), sk_labels(u, v, w, mcs, eps)))
    return out


def same(got, want, what):
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"labels: {what}")
    assert got[0].dtype == np.int64 and got[1].dtype == np.float64
    np.testing.assert_allclose(got[1], want[1], rtol=1e-12, atol=0.0, err_msg=f"probabilities: {what}")


def test_200_random_trees_equal_sklearn():
    for seed, mcs, eps, got, want in outcomes():
        same(got, want, f"seed {seed}, min_cluster_size {mcs}, epsilon {eps}")


def test_the_random_trees_cover_the_interesting_outcomes():
    res = outcomes()
    assert any((want[0] == -1).all() for *_, want in res)                                   # no cluster at all
    assert any(want[0].max() >= 2 for *_, want in res)                                      # three clusters and more
    assert any(((want[0] >= 0) & (want[1] < 1.0)).any() for *_, want in res)                # a probability below one
    by = {(s, m, e): want[0] for s, m, e, _, want in res}
    assert any(e != 0.0 and not np.array_equal(l, by[(s, m, 0.0)]) for (s, m, e), l in by.items())        # the epsilon merge changes a result


def chain(blocks, gaps, inner=1.0):
    """a path graph: blocks[k] points joined by `inner`-weight edges, consecutive blocks joined by gaps[k]; edges sorted by (w, u, v)"""
    u, w, at = [], [], 0
    for k, size in enumerate(blocks):
        for i in range(size - 1):
            u.append(at + i); w.append(inner)
        at += size
        if k + 1 < len(blocks):
            u.append(at - 1); w.append(gaps[k])
    u = np.array(u, np.int64)
    v, w = u + 1, np.array(w, np.float64)
    o = np.lexsort((v, u, w))
    return u[o], v[o], w[o]


@pytest.mark.parametrize("eps", [0.0, EPS_BETWEEN])
def test_no_cluster_at_all(eps):
    u, v, w = chain([4, 3], [5.0])                        # nothing ever reaches min_cluster_size = 5 on both sides of a split
    got, want = cluster.tree_to_labels(u, v, w, 5, eps), sk_labels(u, v, w, 5, eps)
    same(got, want, "all noise")
    assert (got[0] == -1).all() and (got[1] == 0.0).all()


def test_epsilon_merge_swallows_every_leaf():
    # four blocks of 6 split at distances 2, 2 and 3 -- all below epsilon = 4: every excess-of-mass leaf climbs to a child of the root
    u, v, w = chain([6, 6, 6, 6], [2.0, 3.0, 2.0])
    plain, merged = cluster.tree_to_labels(u, v, w, 5, 0.0), cluster.tree_to_labels(u, v, w, 5, 4.0)
    same(plain, sk_labels(u, v, w, 5, 0.0), "four blocks")
    same(merged, sk_labels(u, v, w, 5, 4.0), "four blocks, epsilon 4")
    assert plain[0].max() == 3 and merged[0].max() == 1      # four leaves -> the two children of the root


def test_zero_weights_give_infinite_lambda():
    # exact duplicates: a block joined by zero-weight edges (lambda = inf, probability 1 by sklearn's rule), next to an ordinary block
    u, v, w = chain([7, 7], [3.0], inner=0.0)
    w = w.copy()
    w[(u >= 7)] = 1.0
    o = np.lexsort((v, u, w))
    u, v, w = u[o], v[o], w[o]
    for mcs, eps in PARAMS:
        same(cluster.tree_to_labels(u, v, w, mcs, eps), sk_labels(u, v, w, mcs, eps), f"zero weights, {mcs}, {eps}")


def test_two_points():
    u, v, w = np.array([0]), np.array([1]), np.array([0.5])
    for mcs, eps in PARAMS:
        same(cluster.tree_to_labels(u, v, w, mcs, eps), sk_labels(u, v, w, mcs, eps), f"two points, {mcs}, {eps}")
