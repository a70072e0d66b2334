"""Guarded device buffers for containment tests (tests/test_containment_gpu.py, tests/test_guarded_cpu.py).

Every buffer is a view inside one larger flat uint8 tensor that the test owns, so an access that strays past either end
of the view stays inside that allocation and is seen instead of faulting or landing in a neighbour.  Three roles:

    input      guard bytes 0xFF on both sides: NaN as bf16 and fp32, 255 as uint8, -1 as int32.  A read past the view that
               reaches arithmetic, even multiplied by zero, makes the result non-finite or different.
    output     guard bytes 0xA5 on both sides, compared BYTEWISE (a kernel that writes NaN into a guard is still seen); the
               payload is pre-filled with 0xFF, so an element the kernel never writes stays NaN.
    workspace  guards as for outputs; the payload is pre-filled with `fill` (0xFF in one run, 0x00 in another: the outputs
               must not depend on which).
    inout      (optimizer state, accumulators) guards as for outputs, the payload is a copy of the given tensor.

Guard size is a condition, not a measurement: each side holds at least 256 rows of the buffer's own row pitch for buffers
of two or more dimensions (one full tile of rows, so a store to row M + k lands in it), never under 4 KiB, a multiple of
16 bytes.  The view starts 16-byte aligned.
"""
import torch

IN_GUARD, OUT_GUARD, UNWRITTEN = 0xFF, 0xA5, 0xFF
GUARD_ROWS, GUARD_MIN_BYTES, ALIGN = 256, 4096, 16
_SIZE = {torch.uint8: 1, torch.bfloat16: 2, torch.float16: 2, torch.int32: 4, torch.float32: 4, torch.int64: 8, torch.float64: 8}


def guard_bytes(shape, dtype):
    """Bytes of guard on each side of a buffer of this shape: >= 256 rows of its row pitch (2-D and up), >= 4 KiB,
    a multiple of 16."""
    shape = tuple(int(s) for s in shape)
    pitch = shape[-1] * _SIZE[dtype] if len(shape) >= 2 else 0
    g = max(GUARD_MIN_BYTES, GUARD_ROWS * pitch)
    return (g + ALIGN - 1) // ALIGN * ALIGN


class Guarded:
    """One guarded buffer: `.t` is the typed view to hand to the code under test, `.flat` the whole allocation."""

    def __init__(self, name, shape, dtype, guard_fill, payload_fill=None, source=None, device="cuda"):
        self.name, self.dtype, self.fill = name, dtype, guard_fill
        self.shape = tuple(int(s) for s in shape)
        n = 1
        for s in self.shape:
            n *= s
        self.nbytes = n * _SIZE[dtype]
        self.guard = guard_bytes(self.shape, dtype)
        body = (self.nbytes + ALIGN - 1) // ALIGN * ALIGN          # the far guard starts at the payload's last byte + 1
        self.flat = torch.full((2 * self.guard + body,), guard_fill, dtype=torch.uint8, device=device)
        self.t = self.flat[self.guard:self.guard + self.nbytes].view(dtype).view(self.shape)
        assert self.t.data_ptr() % ALIGN == 0, "view start must be 16-byte aligned"
        if source is not None:
            assert tuple(source.shape) == self.shape and source.dtype == dtype, (name, tuple(source.shape), source.dtype)
            self.t.copy_(source)
        elif payload_fill is not None:
            self.flat[self.guard:self.guard + self.nbytes] = payload_fill

    def ptr(self):
        return self.t.data_ptr()

    def _guards(self):
        return self.flat[:self.guard], self.flat[self.guard + self.nbytes:]

    def violations(self):
        """Byte offsets relative to the view (negative = before its start, >= nbytes = past its end) of the guard bytes
        that no longer hold the guard pattern; at most eight of each side."""
        lo, hi = self._guards()
        bad_lo = (lo != self.fill).nonzero().flatten()[:8] - self.guard
        bad_hi = (hi != self.fill).nonzero().flatten()[:8] + self.nbytes
        return [int(v) for v in bad_lo.tolist() + bad_hi.tolist()]

    def intact(self):
        lo, hi = self._guards()
        return bool((lo == self.fill).all()) and bool((hi == self.fill).all())


def guarded_input(name, source, device="cuda"):
    """A copy of `source` between 0xFF guards."""
    return Guarded(name, source.shape, source.dtype, IN_GUARD, source=source, device=device)


def guarded_output(name, shape, dtype, device="cuda"):
    """An output between 0xA5 guards, every payload byte 0xFF (NaN) until written."""
    return Guarded(name, shape, dtype, OUT_GUARD, payload_fill=UNWRITTEN, device=device)


def guarded_workspace(name, nbytes, fill, device="cuda"):
    """Exactly `nbytes` of workspace (the library's own query, not one byte more) between 0xA5 guards, pre-filled with `fill`."""
    return Guarded(name, (int(nbytes),), torch.uint8, OUT_GUARD, payload_fill=fill, device=device)


def guarded_inout(name, source, device="cuda"):
    """A buffer the code both reads and writes (optimizer state, an accumulator): a copy of `source` between 0xA5 guards."""
    return Guarded(name, source.shape, source.dtype, OUT_GUARD, source=source, device=device)


def assert_guards_intact(bufs, what=""):
    """Every guard byte of every buffer still holds its pattern (call after synchronizing)."""
    for g in bufs:
        assert g.intact(), f"{what}: guard of '{g.name}' overwritten at byte offsets {g.violations()} (view of {g.nbytes} bytes)"


def assert_written(g, what=""):
    """Every element of a floating-point output was written with a finite value (the pre-fill is NaN)."""
    if g.dtype.is_floating_point:
        bad = (~torch.isfinite(g.t.float())).nonzero()
        assert bad.numel() == 0, f"{what}: '{g.name}' has {bad.shape[0]} unwritten or non-finite elements, first at {bad[0].tolist()}"
