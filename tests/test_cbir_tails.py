"""CBIR search at ragged gallery, stage and shard ends: the last 32-row accumulator block of a scan range holds fewer valid rows than it has registers, and the
pre-filter fills the rest with clamped copies of the range's last row.  Every case asserts the oracle's indices, its score bits and `fallbacks == 0` (no fix
may pass by repeating the search with another schedule).  Own module: test_cbir.py's autouse fixture would run every case twice.

Basis queries: query j is e_j, so a row's j-th coordinate is its score for query j and one search puts a survivor at every position of the tail block.  Layout of a
32 x 32 block of the bf16 pre-filter (mfma_f32_32x32x16_bf16): lane l holds query l & 31, and register r of lane half h = l >> 5 holds row
    ROWB + (r & 3) + 8 (r >> 2) + 4 h        -> half 0: offsets 0-3, 8-11, 16-19, 24-27      half 1: offsets 4-7, 12-15, 20-23, 28-31
With rho valid rows (offsets 0 .. rho - 1, rho - 1 = the top row), a lone survivor's lane half mixes it with clamped copies of the top row exactly when it lies in
the half opposite the top row AND that half has an offset >= rho: residues 5..28.  For rho <= 4 every survivor shares half 0 with the top row, for rho >= 29 half 0
is all valid rows and half 1 holds the top row.  Such a survivor once took the lane's maximum -- the top row's score -- as its approximate score, the approximate
ranking then cut the true k-th neighbour (csrc/cbir.hip, CF_EMIT_OWNED)."""
import numpy as np
import pytest
import torch

from oracle import cbir as ocbir
from visiondk_amd import cbir

TOP, SURVIVOR, BELOW, NEIGHBOUR = 0.9, 0.5, -0.5, 0.7


def _plant_tail(g, begin, end, cols):
    """the ragged last 32-row block of the scan range [begin, end) (blocks are aligned to `begin`): for the queries `cols`, row end - 1 is the best row, one lone
    survivor per query at block offset 0, 1, ..., every other row of the block below the cut.  Returns the queries planted (at most rho - 1 of `cols`)."""
    lo = begin + (end - begin - 1) // 32 * 32
    cols = np.asarray(cols)[:max(1, end - lo - 1)]
    g[lo:end, cols] = BELOW
    g[end - 1, cols] = TOP
    g[lo + np.arange(len(cols)), cols] = SURVIVOR
    return cols


def _tail_case(n, d, k=2, seed=0, noise=0.01):
    """background far below the plants, the tail pattern at the gallery end, and the true neighbours 2..k of every query early in the gallery (rows 100 ..,
    descending from 0.7): the exact top-k is row n - 1 and those k - 1 rows, the lone survivors rank right behind them"""
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal((n, d)) * noise).astype(np.float32)
    cols = _plant_tail(g, 0, n, np.arange(min(d, 32)))
    if n >= 100 + k + 32:
        g[100:100 + k - 1, cols] = (NEIGHBOUR - 1e-3 * np.arange(k - 1, dtype=np.float32))[:, None]
    return np.eye(d, dtype=np.float32)[cols], g


def _index(be, d, g, **kw):
    index = cbir.FlatIPIndex(d, backend=be, device="cuda" if be.device_only else "cpu", **kw)
    index.add(g)
    return index


def _mismatch(be, q, g, k, round16=False, **kw):
    """None if the search equals the oracle (indices, score bits) without a fallback, else a description"""
    index = _index(be, q.shape[1], g, **kw)
    s, i = index.search(q, k)
    if round16:      # fp16 storage: the oracle searches the fp16-rounded vectors
        q, g = q.astype(np.float16).astype(np.float32), g.astype(np.float16).astype(np.float32)
    so, io = ocbir.flat_ip_search(q, g, k)
    bad = np.nonzero((i != io).any(1) | (s.view(np.uint32) != so.view(np.uint32)).any(1))[0]
    if len(bad) == 0 and index.fallbacks == 0:
        return None
    return f"fallbacks={index.fallbacks}, queries {bad.tolist()} wrong (first: {i[bad[0]].tolist() if len(bad) else None} vs {io[bad[0]].tolist() if len(bad) else None})"


def _check(be, q, g, k, **kw):
    m = _mismatch(be, q, g, k, **kw)
    assert m is None, m


@pytest.mark.parametrize("d", [128, 256])
def test_lone_survivor_beside_clamped_rows_keeps_its_own_score(be, dev, d):
    """N = 1000 (8 rows in the last block), q = e0: row 999 = 0.9, row 993 = 0.5 alone in its lane half with three rows below the cut and the clamped copies of
    row 999; row 100 = 0.7 is the true second neighbour.  The leak returned [999, 993]."""
    rng = np.random.default_rng(0)
    g = (rng.standard_normal((1000, d)) * 0.01).astype(np.float32)
    g[999, 0], g[993, 0], g[100, 0] = TOP, SURVIVOR, NEIGHBOUR
    g[[992, 994, 995], 0] = BELOW
    q = np.eye(d, dtype=np.float32)[:1]
    index = _index(be, d, g)
    s, i = index.search(q, 2)
    assert i.tolist() == [[999, 100]]
    assert index.fallbacks == 0
    so, io = ocbir.flat_ip_search(q, g, 2)
    np.testing.assert_array_equal(s.view(np.uint32), so.view(np.uint32))


@pytest.mark.parametrize("d", [128, 256])      # the D <= 128 kernel (128-row tiles) and the wide one (32-row tiles): both end a range in a 32-row block
def test_every_tail_residue_every_survivor_position(be, dev, d):
    """N = 1024 + rho for rho = 1..32 (one whole stage: bootstrap, N >= 128 k); residues 5..28 are the exposed ones (module docstring), the rest pin the others"""
    bad = {}
    for rho in range(1, 33):
        q, g = _tail_case(1024 + rho, d, seed=rho)
        m = _mismatch(be, q, g, 2)
        if m:
            bad[rho] = m
    assert not bad, bad


@pytest.mark.parametrize("d", [128, 256])
def test_interior_stage_ends(be, dev, d):
    """Stage lengths of vdk_cbir_search_fast2: FlatIPIndex passes |schedule| = max(1024, cap - 448) rows for the approximate schedule (cap - k for the exact
    staged one); with a threshold bootstrap every stage has that length from the first (without one: 512, 4096, ... up to it), the last stage takes the rest.
    Splits inside a stage are whole tiles from the stage's first row, so every stage ends in a block aligned to its own start.  The default cap (131 072) gives
    130 624-row stages, a multiple of 64: only the gallery end is exposed there.  cap = 1500 gives 1052-row stages (1052 = 32 * 32 + 28): the pattern sits at
    each interior stage end (27 queries each), the true second neighbour of those queries in a later stage, which a leaked score's threshold would cut."""
    stage, n = 1500 - 448, 3500
    ends = [stage, 2 * stage, 3 * stage]
    rng = np.random.default_rng(1)
    g = (rng.standard_normal((n, d)) * 0.01).astype(np.float32)
    cols = []
    for s, e in enumerate(ends):
        c = _plant_tail(g, e - stage, e, np.arange(27 * s, 27 * s + 27))
        assert len(c) == 27
        g[ends[-1] + 100 + c, c] = NEIGHBOUR          # in the last stage
        cols.append(c)
    q = np.eye(d, dtype=np.float32)[np.concatenate(cols)]
    _check(be, q, g, 2, cap=1500)


SCHEDULES = {
    "exact_rank": dict(approx_rank=False),
    "guaranteed": dict(small_lists=False),
    "optimistic": dict(optimistic=True),
    "exact_scan": dict(method="exact_scan"),
    "float16": dict(storage="float16", round16=True),
    "d512": dict(d=512),
    "k32": dict(k=32),
    "k300": dict(k=300),     # k > 256: exact ranking with a workgroup per query
}


@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_tail_residues_through_every_schedule(be, dev, sched):
    """Stratified residues through the other search paths and shapes.  Most do not read the approximate score today; these pin their tail handling.  k = 32 on
    N = 4096 + rho (bootstrap: N >= 128 k) with 31 planted neighbours, over a 0.05 background: eps_q (~0.009 here, the bf16 error of the 0.9 row) is as wide as
    a 0.01 background's spread, ~650 rows would survive the cut, more than one 512-slot ranking pass, and a first pass without the planted rows keeps more than
    448 -- a legitimate overflow whose occurrence depends on the order of the survivors.  k = 300 without a bootstrap (that would take N >= 38 400), on the
    ramp of stages."""
    kw = dict(SCHEDULES[sched])
    d, k = kw.pop("d", 128), kw.pop("k", 2)
    bad = {}
    for rho in (1, 4, 5, 12, 17, 28, 29, 31, 32):
        q, g = _tail_case((4096 if k == 32 else 1024) + rho, d, k=k, seed=rho, noise=0.05 if k == 32 else 0.01)
        m = _mismatch(be, q, g, k, **kw)
        if m:
            bad[rho] = m
    assert not bad, bad


@pytest.mark.parametrize("d", [128, 256])
def test_ragged_shards_merge_to_the_whole_gallery_result(be, dev, d):
    """search_sharded in one process: slices of ragged length (last blocks of 11, 20, 21 and 26 rows), the pattern at every slice end and each query's true second
    neighbour early in its own slice; per-slice searches with idx_base, merged with cbir.merge_topk = the oracle over the whole gallery"""
    bounds = [0, 555, 555 + 788, 555 + 788 + 1013, 555 + 788 + 1013 + 666]
    rng = np.random.default_rng(2)
    g = (rng.standard_normal((bounds[-1], d)) * 0.01).astype(np.float32)
    cols, c0 = [], 0
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        c = _plant_tail(g, lo, hi, np.arange(c0, c0 + 32))
        g[lo + 100 + (c - c0), c] = NEIGHBOUR
        cols.append(c); c0 += len(c)
    q = np.eye(d, dtype=np.float32)[np.concatenate(cols)]
    k, parts_s, parts_i = 2, [], []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        index = _index(be, d, g[lo:hi], idx_base=lo)
        s, i = index.search(q, k)
        assert index.fallbacks == 0
        parts_s.append(torch.from_numpy(s)); parts_i.append(torch.from_numpy(i))
    ms, mi = cbir.merge_topk(torch.stack(parts_s).to(dev), torch.stack(parts_i).to(dev), backend=be)
    so, io = ocbir.flat_ip_search(q, g, k)
    np.testing.assert_array_equal(mi.cpu().numpy(), io)
    np.testing.assert_array_equal(ms.cpu().numpy().view(np.uint32), so.view(np.uint32))


@pytest.mark.parametrize("d", [128, 256])
@pytest.mark.parametrize("n", [20, 1056, 1088])      # one partial block only; a multiple of 32; a multiple of 128 plus 64 (the last 128-row tile half full)
def test_tail_controls(be, dev, n, d):
    q, g = _tail_case(n, d)
    _check(be, q, g, 2)


def _host_splits(begin, end, nq, bg=128):
    """split starts of one pre-filter launch, as vdk_cbir_search_fast2 computes them (D <= 128: 128-row tiles, 512 queries per workgroup)"""
    tiles = -(-(end - begin) // bg)
    nsplit = max(1, min(256 // -(-nq // 512), tiles // 4))
    rps = -(-tiles // nsplit) * bg
    return list(range(begin + rps, end, rps))


def _boundary_case(n=1_000_027, d=128, nq=128, k=64, seed=4):
    """N random unit rows, nq basis queries; planted neighbours of query j (0.55 .. 0.85, above any random coordinate; bf16-exact, so they add nothing to
    eps_q): row 0, both sides of every stage boundary of the default index, a round-robin share of both sides of every split boundary inside the stages.  The
    first rho - 1 queries also carry the tail pattern at the gallery end and random rows up to exactly k planted ones with row n - 1: their lone survivor (0.5)
    is the (k + 1)-th best, and the k-th best (0.55) lies 0.05 > 2 eps_q below the (k - 1)-th, so a survivor ranked on a leaked score would push it out of the
    kept band.  Returns q, g and the planted rows of every query."""
    stage = cbir.DEFAULT_CAP - 448
    rng = np.random.default_rng(seed)
    g = ocbir.l2norm_rows(rng.standard_normal((n, d), dtype=np.float32))
    planted = [{0} for _ in range(nq)]
    for b in range(stage, n, stage):
        for p in planted:
            p.update((b - 1, b))
    sides = [r for s0 in range(0, n, stage) for b in _host_splits(s0, min(s0 + stage, n), nq) for r in (b - 1, b)]
    for j, r in enumerate(sides):
        planted[j % nq].add(r)
    lo = (n - 1) // 32 * 32
    tail = np.arange(min(nq, max(1, n - lo - 1)))       # the queries _plant_tail takes
    for j, p in enumerate(planted):
        assert max(p) < lo
        if j in tail:
            p.update(rng.choice(np.setdiff1d(np.arange(1, lo), list(p)), k - 1 - len(p), replace=False).tolist())
        rows = np.array(sorted(p))
        v = rng.integers(154, 218, len(rows)) / np.float32(256)
        v[rng.integers(len(rows))] = 141 / 256
        g[rows, j] = v
    for j in _plant_tail(g, 0, n, tail):
        planted[j].add(n - 1)
    return np.eye(d, dtype=np.float32)[:nq], g, planted


@pytest.mark.gpu
def test_million_row_gallery_planted_at_every_boundary(hip):
    """cfg4 scale: N = 1 000 027 (default index: 130 624-row stages, the last block 27 rows long: 26 queries carry the tail pattern), 128 basis queries, k = 64.
    Every planted row is found, the result is the oracle's bit for bit, no fallback; again with fp16 storage."""
    k = 64
    q, g, planted = _boundary_case(k=k)
    assert max(map(len, planted)) <= k and sum(len(p) == k and len(g) - 1 in p for p in planted) == 26
    for storage in ("float32", "float16"):
        index = _index(hip, q.shape[1], g, storage=storage)
        s, i = index.search(q, k)
        assert index.fallbacks == 0
        missed = {j: sorted(p - set(i[j].tolist())) for j, p in enumerate(planted) if not p <= set(i[j].tolist())}
        assert not missed, (storage, missed)
        qo, go = (q, g) if storage == "float32" else (q.astype(np.float16).astype(np.float32), g.astype(np.float16).astype(np.float32))
        so, io = ocbir.flat_ip_search(qo, go, k)
        np.testing.assert_array_equal(i, io)
        np.testing.assert_array_equal(s.view(np.uint32), so.view(np.uint32))
        del index
