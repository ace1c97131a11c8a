"""The row-bound checker of tests/rowbound.py, tested on itself: CPU only, no kernels.  The oracle's own 16-bit result must pass; the same result with one planted fault --
"query pi^-1(j) ignores key j" in o and dq, "key j's row misses query pi^-1(j)" in dk and dv -- must be rejected, at the first key, the last key and both sides of every
32-key tile edge (which covers the 64- and 96-key chunk edges) of two shapes."""
import pytest
import torch

from tests import rowbound as rb

BF, HF = torch.bfloat16, torch.float16
# (B, N, H, hd, dtype, dout seed): one past a 96-key chunk in bf16; the first streaming N of the 80-wide geometry in fp16, the faults planted in the last of four items.
# The dout seeds were chosen so that no edge key's dS cancels (asserted below through rb.covered, from float64 alone).
SHAPES = [(1, 97, 2, 64, BF, 4), (2, 257, 2, 80, HF, 0)]
_CASE = {}


def edge_keys(N):
    return sorted({0, N - 1} | {j for e in range(32, N, 32) for j in (e - 1, e)})


def case(B, N, H, hd, dtype, dseed):
    key = (B, N, H, hd, dtype, dseed)
    if key not in _CASE:
        sc = hd ** -0.5
        qkv, dout, pi = rb.peaked_inputs(B, N, H, hd, dtype, 5, dout_seed=dseed)
        q, k, v = rb.split_heads(qkv, H)
        g = rb.heads_of(dout, H)
        ref = rb.reference64(q, k, v, g, sc)
        orc = rb.oracle16(q, k, v, g, sc, dtype)
        _CASE[key] = (sc, pi, (q, k, v, g), ref, orc, rb.bounds(ref, orc))
    return _CASE[key]


def test_permutation_and_matched_mass():
    """pi is a permutation; the matched key holds between 3 % and 97 % of its query's mass, about half in the median: the fault of ignoring it is O(1),
    and so is the rest of the row (a wrong rescale or a wrong unmatched key shows as well)"""
    for N in (1, 2, 17, 33, 65, 97, 197, 224, 225, 256, 257, 290):
        pi = rb.permutation(N)
        assert sorted(pi.tolist()) == list(range(N))
    for hd in (64, 72, 80):
        for N in (17, 97, 290):
            qkv, dout, pi = rb.peaked_inputs(2, N, 2, hd, BF, 0)
            q, k, v = rb.split_heads(qkv, 2)
            P = rb.reference64(q, k, v, rb.heads_of(dout, 2), hd ** -0.5)["P"]
            m = P[..., torch.arange(N), pi]
            assert 0.03 <= float(m.min()) and float(m.max()) <= 0.97 and 0.3 <= float(m.median()) <= 0.7, (hd, N, float(m.min()), float(m.median()), float(m.max()))


@pytest.mark.parametrize("B,N,H,hd,dtype,dseed", SHAPES)
def test_the_oracle_itself_passes(B, N, H, hd, dtype, dseed):
    sc, pi, (q, k, v, g), ref, orc, bnd = case(B, N, H, hd, dtype, dseed)
    for kind in rb.KINDS:
        assert rb.check_rows(kind, orc[kind], ref, bnd[kind], "oracle") == pytest.approx(1.0)
    lse32 = torch.logsumexp(sc * (q.float() @ k.float().transpose(-2, -1)), -1)
    rb.check_lse(lse32, q, k, sc, ref, "float32 torch")


@pytest.mark.parametrize("kind", rb.KINDS)
@pytest.mark.parametrize("B,N,H,hd,dtype,dseed", SHAPES)
def test_every_planted_fault_is_rejected(B, N, H, hd, dtype, dseed, kind):
    sc, pi, inp, ref, orc, bnd = case(B, N, H, hd, dtype, dseed)
    inv, _ = rb.pairs_of(pi)
    item = (B - 1, H - 1)
    keys = edge_keys(N)
    kj = torch.tensor(keys)
    assert bool(rb.covered(kind, ref, *inp, sc, inv[kj], kj, bnd[kind])[item].all())          # the precondition, from float64 alone
    for j in keys:
        bad = rb.plant(kind, orc, ref, *inp, sc, int(inv[j]), j, item)
        with pytest.raises(AssertionError):
            rb.check_rows(kind, bad[kind], ref, bnd[kind], f"planted {kind} key {j}")
        for other in rb.KINDS:                      # and nothing else moved
            if other != kind:
                assert torch.equal(bad[other], orc[other])


def test_lse_with_a_key_ignored_is_rejected():
    B, N, H, hd, dtype, dseed = SHAPES[0]
    sc, pi, (q, k, v, g), ref, orc, bnd = case(B, N, H, hd, dtype, dseed)
    s = sc * (q.double() @ k.double().transpose(-2, -1))
    inv, _ = rb.pairs_of(pi)
    for j in edge_keys(N):
        s2 = s.clone()
        s2[0, 0, inv[j], j] = float("-inf")
        bad = ref["lse"].clone()
        bad[0, 0, inv[j]] = torch.logsumexp(s2[0, 0, inv[j]], -1)
        with pytest.raises(AssertionError):
            rb.check_lse(bad, q, k, sc, ref, f"lse key {j}")
