"""Guard-banded buffers: a tensor of exactly the asked size inside memory the
test owns, with a poisoned band on either side.

    a = arena((E, Le), torch.float32, dev)      # a.view: contiguous [E, Le] float32
    a.view.copy_(table)
    ... a call that receives a.view.data_ptr() ...
    a.check()                                   # both bands still hold the fill byte
    a.unchanged(host_copy)                      # the interior is byte for byte host_copy

Layout.  The view starts BAND bytes into a uint8 backing tensor, moved up to
the next 256-byte boundary of the address space, plus `phase` bytes (a
multiple of 16: the row phase of a table inside a larger allocation); at least
BAND bytes follow it.  BAND = 64 KiB is a condition, not a measurement: an
access that misses a bound by less than that lands in the band — memory this
test owns — and is seen by check().

Fill.  The whole backing tensor, interior included, is filled before use:
float, int32 and workspace arenas with byte 0xFF (every float a NaN, every
int32 -1), index arenas (int64 ids and offsets) with byte 0x7F — an id far
above any entity count, so every range check of the library flags a read of
it, and never the "negative = padding" of a candidate list.  Inputs are then
copied into the interior; what a call must initialise itself is left poisoned.

No fixtures, no side effects: a helper module, also for CPU tensors.
"""
import math

import torch

BAND = 64 * 1024
FLOAT_FILL = 0xFF
INDEX_FILL = 0x7F


class Arena:
    def __init__(self, shape, dtype, device, *, phase=0, fill=None, name=""):
        if isinstance(shape, int):
            shape = (shape,)
        assert phase >= 0 and phase % 16 == 0 and phase < BAND, phase
        self.name = name or f"{tuple(shape)} {dtype}"
        self.fill = (INDEX_FILL if dtype == torch.int64 else FLOAT_FILL) if fill is None else fill
        self.nbytes = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
        assert self.nbytes > 0, f"arena {self.name}: empty"
        self.backing = torch.empty(2 * BAND + 256 + phase + self.nbytes, dtype=torch.uint8, device=device)
        self.backing.fill_(self.fill)
        base = self.backing.data_ptr()
        self.start = BAND + (-(base + BAND)) % 256 + phase
        self.end = self.start + self.nbytes
        self.bytes = self.backing[self.start:self.end]
        self.view = self.bytes.view(dtype).view(shape)
        assert self.view.is_contiguous() and self.view.data_ptr() == base + self.start
        assert self.view.data_ptr() % 256 == phase % 256
        assert self.start >= BAND and self.backing.numel() - self.end >= BAND

    def ptr(self):
        return self.view.data_ptr()

    def put(self, src):
        """Copy an input (tensor or numpy array of the view's shape and dtype) into the interior."""
        t = src if isinstance(src, torch.Tensor) else torch.from_numpy(src)
        assert t.dtype == self.view.dtype and tuple(t.shape) == tuple(self.view.shape), (self.name, t.dtype, t.shape)
        self.view.copy_(t)
        return self

    def host(self):
        """A host copy of the interior."""
        return self.view.detach().cpu().clone()

    def violations(self):
        """[(side, first offset, bytes that differ)]: side "before" with the offset relative to
        the interior's start (negative), side "after" relative to its end (0 = the first byte past it)."""
        out = []
        for side, band, origin in (("before", self.backing[:self.start], -self.start),
                                   ("after", self.backing[self.end:], 0)):
            bad = (band != self.fill).nonzero()
            if bad.numel():
                out.append((side, origin + int(bad[0, 0]), int(bad.shape[0])))
        return out

    def check(self):
        """Both bands still hold the fill byte everywhere."""
        v = self.violations()
        assert not v, "; ".join(f"arena {self.name}: {n} byte(s) written {side} the buffer, first at offset {off} "
                                f"(relative to the buffer's {'start' if side == 'before' else 'end'})"
                                for side, off, n in v)

    def poisoned(self):
        """The interior still holds the fill byte everywhere (a buffer a call must not write)."""
        bad = (self.bytes != self.fill).nonzero()
        assert not bad.numel(), (f"arena {self.name}: {bad.shape[0]} interior byte(s) written, first at "
                                 f"byte {int(bad[0, 0])}")

    def unchanged(self, host_copy):
        """The interior equals host_copy byte for byte (a buffer a call must not write)."""
        h = host_copy if isinstance(host_copy, torch.Tensor) else torch.from_numpy(host_copy)
        assert h.dtype == self.view.dtype and h.numel() == self.view.numel(), (self.name, h.dtype, h.shape)
        want = h.contiguous().reshape(-1).view(torch.uint8)
        got = self.bytes.cpu()
        bad = (got != want).nonzero()
        assert not bad.numel(), (f"arena {self.name}: interior changed in {bad.shape[0]} byte(s), first at "
                                 f"byte {int(bad[0, 0])}")


def arena(shape, dtype, device, *, phase=0, fill=None, name=""):
    return Arena(shape, dtype, device, phase=phase, fill=fill, name=name)


def arena_of(src, device, *, phase=0, fill=None, name=""):
    """An arena holding a copy of `src` (tensor or numpy array)."""
    t = src if isinstance(src, torch.Tensor) else torch.from_numpy(src)
    return Arena(tuple(t.shape), t.dtype, device, phase=phase, fill=fill, name=name).put(t)
