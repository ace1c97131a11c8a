"""Guard-banded operands for the extent-isolation tests (plain module: no fixtures, no pytest settings).

Every operand a kernel sees lies inside ONE allocation that is filled with a byte pattern first: at least GUARD_ROWS rows of the padded pitch and at least GUARD_BYTES (flat
buffers: GUARD_FLAT bytes, whatever their length) before and after the logical window, and `pad_cols` elements between the rows.  After the call
  * every byte outside the logical windows must still hold the pattern (a stray WRITE changes it), and
  * the outputs must not depend on the pattern (a stray READ that reaches an output changes them; so does an output element the kernel never wrote, because the window of an
    output starts out as pattern too).
The patterns are BYTES, so one value serves every dtype: 0x00; 0xFF (NaN in f32 / bf16 / fp16, -1 in int32 / int64); 0x7B (a large finite number in the three float formats,
a large positive integer).  The guards are larger than any tile of the kernels, so an over-read by up to a whole tile stays inside its own allocation: these tests never hand
a kernel less memory than its contract asks for.
"""
from __future__ import annotations

import contextlib

import torch

FILLS = (0x00, 0xFF, 0x7B)
GUARD_ROWS = 256
GUARD_BYTES = 64 * 1024
GUARD_FLAT = 256 * 1024                    # flat buffers (workspaces, statistics, vectors): more than any tile of the kernels, and independent of the buffer's own length


def _guard_bytes(pitch_bytes: int, flat: bool) -> int:
    """2-D operands: at least GUARD_ROWS rows of the padded pitch and at least GUARD_BYTES; flat buffers have no pitch, their guard is a fixed GUARD_FLAT"""
    g = GUARD_FLAT if flat else max(GUARD_BYTES, GUARD_ROWS * pitch_bytes)
    return (g + 255) // 256 * 256          # the window keeps the allocation's alignment (row starts still shift with a pitch that is no multiple of the vector width)


class Region:
    """one guarded allocation: `big` (uint8, flat) and the logical window [rows, cols] of `dtype` at row pitch `pitch` elements that starts `front` bytes in"""

    def __init__(self, big, view, front, rows, cols_bytes, pitch_bytes, name):
        self.big, self.view, self.front, self.rows, self.cols_bytes, self.pitch_bytes, self.name = big, view, front, rows, cols_bytes, pitch_bytes, name

    def guards(self):
        """the parts of `big` outside the logical window, as (offset into big, uint8 tensor) pairs: the bytes in front, the bytes behind, the padding between the rows"""
        end = self.front + (self.rows - 1) * self.pitch_bytes + self.cols_bytes if self.rows else self.front
        parts = [(0, self.big[:self.front]), (end, self.big[end:])]
        if self.rows > 1 and self.pitch_bytes > self.cols_bytes:
            parts.append((self.front, self.big[self.front: self.front + (self.rows - 1) * self.pitch_bytes].view(self.rows - 1, self.pitch_bytes)[:, self.cols_bytes:]))
        return parts


def embed(x: torch.Tensor, *, pad_cols: int = 0, fill: int = 0, dev="cpu", name: str = "") -> tuple[Region, torch.Tensor]:
    """-> (region, view).  x is [rows, cols] (row pitch cols + pad_cols elements) or 1-D (a flat buffer).  One allocation filled with the byte `fill` holds x behind a guard of
    at least GUARD_ROWS rows of the pitch (2-D) or GUARD_FLAT bytes (1-D), and as much again behind it; `view` is the window whose data_ptr() / stride(0) go to the ABI."""
    flat = x.dim() == 1
    x2 = x.reshape(1, -1) if flat else x
    assert x2.dim() == 2
    rows, cols = x2.shape
    isz = x2.element_size()
    pitch = cols + pad_cols
    pitch_bytes, cols_bytes = pitch * isz, cols * isz
    g = _guard_bytes(pitch_bytes, flat)
    total = g + rows * pitch_bytes + g
    big = torch.full((total,), fill, dtype=torch.uint8, device=dev)
    body = big[g: g + rows * pitch_bytes].view(x2.dtype).view(rows, pitch)
    view = body[:, :cols]
    view.copy_(x2.to(dev))
    reg = Region(big, view, g, rows, cols_bytes, pitch_bytes, name)
    return reg, (view.reshape(-1) if flat else view)          # (one row: reshape of a contiguous slice is still a view of `big`)


def assert_guards_intact(reg: Region, fill: int) -> None:
    """every byte outside the logical window still equals `fill`, compared as uint8 (NaN != NaN, and the 16-bit formats round a float pattern)"""
    for off, part in reg.guards():
        bad = part != fill
        if bool(bad.any()):
            at = torch.nonzero(bad)[0].tolist()
            if len(at) == 2:
                where = f"row {at[0]}, byte {reg.cols_bytes + at[1]} of the pitch ({reg.cols_bytes} live)"
            else:
                rel = off + at[0] - reg.front
                where = f"{-rel} bytes before the window" if rel < 0 else f"{rel - ((reg.rows - 1) * reg.pitch_bytes + reg.cols_bytes)} bytes behind the window"
            raise AssertionError(f"stray write into the guard of `{reg.name}`: {int(bad.sum())} bytes changed (pattern 0x{fill:02X}), first at {where}")


def bits(t: torch.Tensor) -> torch.Tensor:
    """the tensor's values as integers, contiguous, on the CPU"""
    t = t.detach().contiguous()
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return (t if t.dtype == torch.bool else t.view(it)).cpu()


def assert_same_bits(results, what: str = "") -> None:
    """results: one dict name -> tensor per run; all runs equal as integers"""
    first = results[0]
    for i, r in enumerate(results[1:], 1):
        assert r.keys() == first.keys()
        for k in first:
            a, b = bits(first[k]), bits(r[k])
            assert a.shape == b.shape, (what, k)
            if not torch.equal(a, b):
                d = torch.nonzero(a != b)
                raise AssertionError(f"{what}: output `{k}` of run {i} differs from run 0 in {d.shape[0]} of {a.numel()} elements, first at {tuple(d[0].tolist())}")


@contextlib.contextmanager
def one_torch_thread():
    """the guard bookkeeping is hundreds of small fills and compares per test: with several pytest workers on one machine torch's intra-op thread pools (one per worker, each as wide
    as the machine) only fight over the cores.  One thread while an isolation test runs, the previous setting afterwards; the kernels under test do not run on torch's threads."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


class Arena:
    """the operands of one call.  fill = a byte: guarded, padded allocations; fill = None: plain contiguous tensors (the call every other test makes)."""

    def __init__(self, fill, dev):
        self.fill, self.dev, self.regions = fill, dev, []

    @property
    def plain(self) -> bool:
        return self.fill is None

    def put(self, x: torch.Tensor, pad: int = 0, name: str = "in") -> torch.Tensor:
        """an input (or in/out) operand holding x"""
        if self.plain:
            return x.to(self.dev).contiguous().clone()
        reg, view = embed(x, pad_cols=pad, fill=self.fill, dev=self.dev, name=name)
        self.regions.append(reg)
        return view

    def out(self, shape, dtype, pad: int = 0, name: str = "out") -> torch.Tensor:
        """an output operand: its window starts out as the pattern, so an element the kernel does not write shows up as a difference between the runs"""
        if self.plain:
            return torch.zeros(shape, dtype=dtype, device=self.dev)
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        x = torch.empty(shape, dtype=dtype)
        reg, view = embed(x, pad_cols=pad, fill=self.fill, dev=self.dev, name=name)
        reg.big[reg.front: reg.front + reg.rows * reg.pitch_bytes] = self.fill
        self.regions.append(reg)
        return view

    def check(self) -> None:
        for reg in self.regions:
            assert_guards_intact(reg, self.fill)


def run_isolated(case, dev, sync=None, same_as_plain=True, what: str = ""):
    """case(arena) -> dict of outputs.  Runs it once per pattern and once on plain tensors: I1 guards intact, I2 outputs bit-identical across the patterns, I3 (same_as_plain)
    the 0x00 run bit-identical to the plain contiguous call.  Returns (outputs of the 0x00 run, outputs of the plain run)."""
    with one_torch_thread():
        return _run_isolated(case, dev, sync, same_as_plain, what)


def _run_isolated(case, dev, sync, same_as_plain, what):
    results = []
    for fill in FILLS:
        ar = Arena(fill, dev)
        outs = case(ar)
        if sync is not None:
            sync()
        ar.check()
        results.append({k: bits(v) for k, v in outs.items() if v is not None})
        if fill == FILLS[0]:
            first = {k: v.detach().clone() for k, v in outs.items() if v is not None}
    assert_same_bits(results, what)
    pl = case(Arena(None, dev))
    if sync is not None:
        sync()
    pl = {k: v for k, v in pl.items() if v is not None}
    if same_as_plain:
        assert_same_bits([results[0], {k: bits(v) for k, v in pl.items()}], what + " (padded vs contiguous)")
    return first, pl
