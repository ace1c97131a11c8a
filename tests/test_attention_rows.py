"""K3 attention, every output ROW bounded on inputs in which every key matters (tests/rowbound.py): the general kernels at head dims 64 and 80 (public entries) and 72
(the debug entries, tests/test_attention_hd72.py) in bf16 and fp16, on the CPU SIMT emulation and on the device.

The whole-tensor norms of tests/test_attention*.py accept a result with one entirely wrong row (1 / sqrt(rows) of the norm) and, on dense Gaussian q / k, one with a key
dropped, duplicated or misplaced at a tile, chunk or tail edge (1 / N of a row's mass).  Here q / k are permutation-peaked -- every key is the dominant key of exactly one
query, every query the dominant contributor of exactly one dK / dV row -- and o, dq, dk, dv are bounded row by row: |got_r - ref64_r| / s(r) <= 4 x the worst such row of
oracle/bf16ops.py in the case's 16-bit mode, s(r) the absolute-value product that went into the row; lse element by element against 8 x torch's float32 error.  Before a
kernel result is looked at, the case asserts from float64 alone that ignoring any single key would break the bound (rowbound.assert_sensitive).

Routes: the default routing; VDK_ATTN_LONG_MIN=1 (the streaming kernels of csrc/attention_long.hip at short N; head dim 64 -- the 72 / 80-wide kernels stream at every N);
vdk_attention_force_legacy(1) (bf16, head dim 64); VDK_ATTN_GRID=2 on one short and one long shape (a workgroup walks over several items / units).

Shapes: the smallest N that reach each edge -- 1; 17 (one partial tile); 33, 65 (one past a tile / a 64-key chunk); 97 (one past a 96-key chunk); 197; 224 | 225 (the last N
of the one-pass backward | the first of the streaming one); 256 | 257 (the last LDS-resident forward | the first streaming one); 290; an odd item count."""
import pytest
import torch

from tests import rowbound as rb
from tests.test_attention_hd72 import run_hd
from visiondk_amd import ops

BF, HF = torch.bfloat16, torch.float16
SHAPES = [(2, 1, 1), (2, 17, 2), (1, 33, 2), (1, 65, 2), (1, 97, 2), (1, 197, 2), (1, 224, 2), (1, 225, 2), (1, 256, 2), (1, 257, 2), (1, 290, 2), (3, 65, 3)]
GRID_SHAPES = [(3, 65, 2), (3, 290, 2)]
SEED = 11
# dout seeds per case, chosen on the CPU (float64 and the oracle only): the smallest set of seeds 0 .. 7 under which every key position's "ignored" fault stands 3 x above
# the dq and dk bounds in at least one seed, with 12 % to spare (rowbound.assert_sensitive asserts the 3 x in every run).  Cases not listed: (0,).
DOUT_SEEDS = {
    (1, 33, 2, 64, 'bf16'): (2,), (1, 197, 2, 64, 'bf16'): (3,), (1, 224, 2, 64, 'bf16'): (0, 1), (1, 225, 2, 64, 'bf16'): (0, 1), (1, 256, 2, 64, 'bf16'): (0, 1),
    (1, 257, 2, 64, 'bf16'): (0, 1), (1, 290, 2, 64, 'bf16'): (0, 2), (1, 97, 2, 72, 'bf16'): (3,), (1, 197, 2, 72, 'bf16'): (4,), (1, 224, 2, 72, 'bf16'): (0, 1),
    (1, 225, 2, 72, 'bf16'): (0, 1), (1, 256, 2, 72, 'bf16'): (0, 2), (1, 257, 2, 72, 'bf16'): (0, 2), (1, 290, 2, 72, 'bf16'): (0, 2), (1, 197, 2, 80, 'bf16'): (1,),
    (1, 224, 2, 80, 'bf16'): (0, 1), (1, 225, 2, 80, 'bf16'): (0, 1), (1, 256, 2, 80, 'bf16'): (4,), (1, 257, 2, 80, 'bf16'): (0, 1), (1, 290, 2, 80, 'bf16'): (0, 2),
}

_CASE = {}


def _seeds(B, N, H, hd, dtype):
    return DOUT_SEEDS.get((B, N, H, hd, "bf16" if dtype == BF else "fp16"), (0,))


def case(B, N, H, hd, dtype):
    """inputs, float64 reference, oracle bounds per dout seed -- computed once per (shape, head dim, format) and shared by the routes and backends; the sensitivity
    preconditions are asserted here, before any kernel runs"""
    key = (B, N, H, hd, dtype)
    if key not in _CASE:
        sc = hd ** -0.5
        per_seed = []
        for ds in _seeds(B, N, H, hd, dtype):
            qkv, dout, pi = rb.peaked_inputs(B, N, H, hd, dtype, SEED, dout_seed=ds)
            q, k, v = rb.split_heads(qkv, H)
            g = rb.heads_of(dout, H)
            ref = rb.reference64(q, k, v, g, sc)
            bnd = rb.bounds(ref, rb.oracle16(q, k, v, g, sc, dtype))
            per_seed.append({"qkv": qkv, "dout": dout, "inp": (q, k, v, g), "ref": ref, "bnd": bnd})
        qi, kj = rb.pairs_of(pi)
        rb.assert_sensitive([s["ref"] for s in per_seed], [s["inp"] for s in per_seed], sc, qi, kj, [s["bnd"] for s in per_seed], what=f"B{B} N{N} H{H} hd{hd} {dtype}")
        _CASE[key] = per_seed
    return _CASE[key]


def check_case(be, dev, B, N, H, hd, dtype, route):
    sc = hd ** -0.5
    what = f"[{route} hd{hd} {'bf16' if dtype == BF else 'fp16'} B{B} N{N} H{H}]"
    ratios = {}
    for n, s in enumerate(case(B, N, H, hd, dtype)):
        qkv, dout = s["qkv"], s["dout"]
        if hd == 72:
            o, lse, dqkv = run_hd(be, dev, qkv, dout, H)
        else:
            qd = qkv.to(dev)
            o, lse = ops.attention_fwd(qd, H, backend=be)
            dqkv = ops.attention_bwd(qd, o, dout.to(dev), lse, H, backend=be).cpu()          # the backward consumes the forward's own 16-bit o and lse
            o, lse = o.cpu(), lse.cpu()
        q, k = s["inp"][0], s["inp"][1]
        D = H * hd
        got = {"o": rb.heads_of(o, H), "dq": rb.heads_of(dqkv[..., :D], H), "dk": rb.heads_of(dqkv[..., D:2 * D], H), "dv": rb.heads_of(dqkv[..., 2 * D:], H)}
        if n == 0:
            ratios["lse"] = rb.check_lse(lse, q, k, sc, s["ref"], what)
        for kind in (rb.KINDS if n == 0 else rb.KINDS[1:]):
            r = rb.check_rows(kind, got[kind], s["ref"], s["bnd"][kind], what)
            ratios[kind] = max(r, ratios.get(kind, 0.0))
    print(f"rows {what} ratios: " + " ".join(f"{k}={v:.2f}" for k, v in ratios.items()))


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("hd", [64, 72, 80])
@pytest.mark.parametrize("B,N,H", SHAPES)
def test_attention_rows_default_routing(be, dev, B, N, H, hd, dtype, monkeypatch):
    for knob in ("VDK_ATTN_LONG_MIN", "VDK_ATTN_GRID", "VDK_ATTN_LEGACY"):
        monkeypatch.delenv(knob, raising=False)
    check_case(be, dev, B, N, H, hd, dtype, "default")


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,N,H", [s for s in SHAPES if s[1] <= 256])
def test_attention_rows_streaming_kernels_at_short_n(be, dev, B, N, H, dtype, monkeypatch):
    """VDK_ATTN_LONG_MIN=1: single-chunk sequences, chunks with whole tiles beyond N, a ragged last chunk at 97 and 225, groups with idle waves"""
    monkeypatch.setenv("VDK_ATTN_LONG_MIN", "1")
    check_case(be, dev, B, N, H, 64, dtype, "streaming")


@pytest.mark.parametrize("B,N,H", SHAPES)
def test_attention_rows_legacy_kernels(be, dev, B, N, H):
    """the flash-style kernels of csrc/attention.hip (bf16, head dim 64)"""
    be.lib.vdk_attention_force_legacy(1)
    try:
        check_case(be, dev, B, N, H, 64, BF, "legacy")
    finally:
        be.lib.vdk_attention_force_legacy(-1)


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("hd", [64, 72, 80])
@pytest.mark.parametrize("B,N,H", GRID_SHAPES)
def test_attention_rows_several_items_per_workgroup(be, dev, B, N, H, hd, dtype, monkeypatch):
    """VDK_ATTN_GRID=2: six (batch, head) items on a capped grid, so a workgroup's LDS arrays, prefetches and chunk buffers run on across item / unit boundaries"""
    monkeypatch.setenv("VDK_ATTN_GRID", "2")
    check_case(be, dev, B, N, H, hd, dtype, "grid2")
