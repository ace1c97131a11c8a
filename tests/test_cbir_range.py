"""Exact range search (csrc/cbir_range.hip: cbir.FlatIPIndex.range_search, faiss IndexFlat.range_search) against the oracle: every pair's exact score in the oracle's own bits
(oracle.cbir.flat_ip_search with k = N returns all N scores of a query), thresholded in numpy.  lims, I (ascending inside a query) and D (compared as uint32) must be equal,
on the CPU SIMT emulation and (-m gpu) through the same C ABI on the MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import cbir as ocbir
from visiondk_amd import cbir, faiss_shim

F32 = np.float32
EINVAL = -1


@functools.lru_cache(maxsize=None)
def _case(nq, n, d, storage, seed=0):
    """continuous Gaussian rows, L2-normalised, plus a planted block (40 gallery rows close to the first four queries: dense answers) -> q, g, S = all exact scores [nq, n]
    (fp16 storage: the oracle is fed the fp16-rounded vectors, as tests/test_cbir.py does); computed once per shape, never modified"""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, d), dtype=F32)
    q = ocbir.l2norm_rows(rng.standard_normal((nq, d), dtype=F32))
    for j in range(min(40, n)):
        g[(7 * j + 3) % n] = q[j % min(4, nq)] * F32(4.0) + F32(0.35) * rng.standard_normal(d, dtype=F32)
    g = ocbir.l2norm_rows(g)
    qo, go = (q.astype(np.float16).astype(F32), g.astype(np.float16).astype(F32)) if storage == "float16" else (q, g)
    so, io = ocbir.flat_ip_search(qo, go, n)
    S = np.empty((nq, n), F32)
    np.put_along_axis(S, io, so, axis=1)
    S.setflags(write=False)
    return q, g, S


def _expect(S, r, inclusive=False, idx_base=0):
    hit = (S >= r) if inclusive else (S > r)
    lims = np.concatenate([[0], np.cumsum(hit.sum(1))]).astype(np.int64)
    rows, cols = np.nonzero(hit)                       # row-major: ascending gallery index inside each query
    return lims, S[rows, cols], cols.astype(np.int64) + idx_base


def _index(be, dev, d, g, storage="float32", **kw):
    idx = cbir.FlatIPIndex(d, backend=be, device=dev, storage=storage, **kw)
    idx.add(g)
    return idx


def _same(got, want):
    lims, D, I = got
    assert lims.dtype == np.int64 and D.dtype == F32 and I.dtype == np.int64
    np.testing.assert_array_equal(lims, want[0])
    np.testing.assert_array_equal(I, want[2])
    np.testing.assert_array_equal(D.view(np.uint32), want[1].view(np.uint32))


def _radii(S):
    """above every score; about 1.5 results per query; about 5 % of N per query; below every score"""
    flat = np.sort(S.reshape(-1))[::-1]
    nq, n = S.shape
    return {"empty": np.nextafter(flat[0], F32(np.inf)), "few": flat[int(1.5 * nq)], "5pct": flat[int(0.05 * n * nq)], "all": np.nextafter(flat[-1], F32(-np.inf))}


SHAPES = [(33, 1000, 128, "float32"),
          (130, 333, 64, "float32"),      # the second 128-query block of the count kernels, a ragged last tile, D padded to 128
          (33, 700, 192, "float32"),      # the wide filter, NK 16
          (9, 1000, 512, "float16"),      # the wide filter, NK 32
          (33, 1000, 128, "float16"),
          (5, 2100, 30, "float32"),       # d % 4 != 0: the class pads; more than one 2048-row chunk
          (600, 70, 128, "float32")]      # the second 512-query workgroup of the D <= 128 filter


@pytest.mark.parametrize("which", ["empty", "few", "5pct", "all"])
@pytest.mark.parametrize("nq,n,d,storage", SHAPES)
def test_range_bit_exact(be, dev, nq, n, d, storage, which):
    q, g, S = _case(nq, n, d, storage)
    r = _radii(S)[which]
    got = _index(be, dev, d, g, storage).range_search(q, r)
    want = _expect(S, r)
    _same(got, want)
    if which == "empty":
        assert not got[0].any() and got[1].size == 0
    if which == "all":
        assert got[0][-1] == nq * n                    # every pair, with no capacity anywhere
    if which == "few":
        assert 0 < got[0][-1] <= 3 * nq


def _bf16_scores(q, g):
    """the pre-filter's approximate score of every pair (bf16-rounded operands; float64 accumulation stands in for the MFMA's fp32)"""
    qb, gb = torch.from_numpy(q).bfloat16().double().numpy(), torch.from_numpy(g).bfloat16().double().numpy()
    return qb @ gb.T


@pytest.mark.parametrize("side", ["approx_below", "approx_above"])
@pytest.mark.parametrize("nq,n,d,storage", [(33, 1000, 128, "float32"), (33, 700, 192, "float32"), (33, 1000, 128, "float16")])
def test_radius_equal_to_a_score(be, dev, nq, n, d, storage, side):
    """r = an existing pair's exact score, bit for bit, chosen where the bf16 approximate score lies on the OTHER side of r: the pair is absent without `inclusive`, present
    with it, and everything else is identical.  Fails if the decision is taken on the approximate score."""
    q, g, S = _case(nq, n, d, storage)
    qo, go = (q.astype(np.float16).astype(F32), g.astype(np.float16).astype(F32)) if storage == "float16" else (q, g)
    diff = _bf16_scores(qo, go) - S.astype(np.float64)
    # among the pairs of the top 5 % (so that r is a radius with real answers): the one whose approximate score is furthest on the chosen side
    cand = S >= _radii(S)["5pct"]
    pick = np.where(cand, diff, np.inf if side == "approx_below" else -np.inf)
    qi, gi = np.unravel_index(np.argmin(pick) if side == "approx_below" else np.argmax(pick), S.shape)
    assert (diff[qi, gi] < 0) if side == "approx_below" else (diff[qi, gi] > 0)     # such a pair exists among the data
    r = S[qi, gi]
    idx = _index(be, dev, d, g, storage)
    ex, inc = idx.range_search(q, r), idx.range_search(q, r, inclusive=True)
    _same(ex, _expect(S, r))
    _same(inc, _expect(S, r, inclusive=True))
    in_q = lambda res: set(res[2][res[0][qi]:res[0][qi + 1]].tolist())
    assert gi not in in_q(ex) and gi in in_q(inc)
    assert inc[0][-1] - ex[0][-1] == int((S == r).sum())


def test_idx_base_two_adds_and_repeat(be, dev):
    q, g, S = _case(33, 1000, 128, "float32")
    r = _radii(S)["5pct"]
    idx = cbir.FlatIPIndex(128, backend=be, device=dev, idx_base=70000)
    idx.add(g[:333])
    idx.add(g[333:])                                   # a gallery added in two calls
    assert idx.ntotal == 1000
    want = _expect(S, r, idx_base=70000)
    first = idx.range_search(q, r)
    _same(first, want)
    second = idx.range_search(q, r)                    # the same bits on a second call
    for a, b in zip(first, second):
        np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == F32 else a, b.view(np.uint32) if b.dtype == F32 else b)
    s, i = idx.search(q, 10)                           # the top-k search of the same index is untouched by the range search's workspace use
    so, io = ocbir.flat_ip_search(q, g, 10, idx_base=70000)
    np.testing.assert_array_equal(i, io)


def test_empty_gallery_and_no_queries(be, dev):
    q, g, S = _case(33, 1000, 128, "float32")
    idx = cbir.FlatIPIndex(128, backend=be, device=dev)
    lims, D, I = idx.range_search(q, 0.0)              # N == 0
    assert lims.shape == (34,) and not lims.any() and D.shape == (0,) and I.shape == (0,) and D.dtype == F32 and I.dtype == np.int64
    idx.add(g)
    lims, D, I = idx.range_search(q[:0], 0.0)          # nq == 0
    assert lims.tolist() == [0] and D.shape == (0,) and I.shape == (0,)


def test_tensor_in_tensor_out(be, dev):
    q, g, S = _case(33, 1000, 128, "float32")
    r = _radii(S)["5pct"]
    idx = _index(be, dev, 128, g)
    lims, D, I = idx.range_search(torch.from_numpy(q).to(dev), float(r))
    assert all(isinstance(t, torch.Tensor) and t.device.type == torch.device(dev).type for t in (lims, D, I))
    assert lims.dtype == torch.int64 and D.dtype == torch.float32 and I.dtype == torch.int64
    _same((lims.cpu().numpy(), D.cpu().numpy(), I.cpu().numpy()), _expect(S, r))


def test_query_blocks_are_concatenated(be, dev, monkeypatch):
    """a bit matrix bound small enough that the 600 queries go through two blocks: the same triple"""
    q, g, S = _case(600, 70, 128, "float32")
    monkeypatch.setattr(cbir, "RANGE_MASK_BYTES", 1)   # -> the minimum block of 512 queries
    r = _radii(S)["5pct"]
    _same(_index(be, dev, 128, g).range_search(q, r), _expect(S, r))


def test_max_results_states_the_exact_total(be, dev):
    q, g, S = _case(33, 1000, 128, "float32")
    r = _radii(S)["5pct"]
    total = int((S > r).sum())
    idx = _index(be, dev, 128, g)
    with pytest.raises(RuntimeError, match=rf"\b{total}\b"):
        idx.range_search(q, r, max_results=total - 1)
    _same(idx.range_search(q, r, max_results=total), _expect(S, r))


def test_refusals(be, dev):
    q, g, S = _case(33, 1000, 128, "float32")
    with pytest.raises(NotImplementedError, match="512"):
        cbir.FlatIPIndex(516, backend=be, device=dev).range_search(np.zeros((1, 516), F32), 0.5)
    with pytest.raises(NotImplementedError, match="512"):
        _index(be, dev, 128, g, method="exact_scan").range_search(q, 0.5)
    idx = _index(be, dev, 128, g)
    with pytest.raises(ValueError):
        idx.range_search(q, float("nan"))
    with pytest.raises(ValueError):
        idx.range_search(q[:, :64], 0.5)
    with pytest.raises(TypeError):
        idx.range_search(q.astype(np.float64), 0.5)
    # the raw entries
    idx._prepare()
    p, lib = be.ptr, be.lib
    qd, gd = torch.from_numpy(q).to(dev), idx._gallery
    need = C.c_size_t(0)
    be.check(lib.vdk_cbir_range_workspace_bytes(33, 1000, 128, C.byref(need)), "workspace")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    lims = torch.zeros(34, dtype=torch.int64, device=dev)

    def count(D=128, gdt=1, radius=0.5, lims_=lims, n_=need.value, ws_=ws):
        return lib.vdk_cbir_range_count(p(qd), 33, p(gd), gdt, p(idx._gb), p(idx._gmax), 1000, D, radius, 0, p(lims_), p(ws_), n_, be.stream())
    for kw in (dict(D=126), dict(D=124, gdt=2), dict(D=516), dict(radius=float("nan")), dict(lims_=None), dict(gdt=0)):
        assert count(**kw) == EINVAL and b"vdk_cbir_range" in lib.vdk_last_error(), kw
    assert lib.vdk_cbir_range_workspace_bytes(33, 1000, 516, C.byref(need)) == EINVAL and lib.vdk_cbir_range_workspace_bytes(33, 1000, 128, None) == EINVAL
    assert lib.vdk_cbir_range_workspace_bytes(-1, 1000, 128, C.byref(need)) == EINVAL
    assert count() == 0
    if be.device_only:
        torch.cuda.synchronize()
    total = int(lims[33].item())
    assert total > 0
    rc = lib.vdk_cbir_range_fill(p(qd), 33, p(gd), 1, 1000, 128, 0, p(lims), total, None, None, p(ws), ws.numel(), be.stream())
    assert rc == EINVAL and b"null output" in lib.vdk_last_error()         # null outputs with a non-zero count
    assert lib.vdk_cbir_range_fill(p(qd), 33, p(gd), 1, 1000, 126, 0, p(lims), total, None, None, p(ws), ws.numel(), be.stream()) == EINVAL


def test_through_the_faiss_shim(be, dev):
    q, g, S = _case(130, 333, 64, "float32")
    r = _radii(S)["5pct"]
    faiss_shim.set_default(backend=be, device=dev)
    try:
        idx = faiss_shim.index_factory(64, "Flat", faiss_shim.METRIC_INNER_PRODUCT)
        idx.add(g)
        _same(idx.range_search(q, r), _expect(S, r))
    finally:
        faiss_shim.set_default()
