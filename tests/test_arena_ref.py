"""The guard-band helper (tests/arena.py) tested on CPU tensors, the stability
of the workspace-size queries tests/test_arena_gpu.py sizes its arenas from,
and ops._check_filter_shape (the host check of the filter arrays' length).
No GPU needed: the size queries are host-only arithmetic."""
import numpy as np
import pytest
import torch

import arena_cases as A
from arena import BAND, FLOAT_FILL, INDEX_FILL, arena, arena_of
from knowledgegraphembedding_amd import _lib, ops

CPU = torch.device("cpu")


# ------------------------------------------------------------------ helper
@pytest.mark.parametrize("dtype", [torch.float32, torch.int64, torch.int32, torch.uint8])
@pytest.mark.parametrize("phase", [0, 16, 240])
def test_arena_layout_and_fill(dtype, phase):
    a = arena((7, 3), dtype, CPU, phase=phase)
    assert a.view.data_ptr() % 256 == phase and a.view.is_contiguous()
    assert a.view.shape == (7, 3) and a.view.dtype == dtype
    assert a.start >= BAND and a.backing.numel() - a.end >= BAND
    assert a.nbytes == 21 * a.view.element_size() and a.end - a.start == a.nbytes
    want = INDEX_FILL if dtype == torch.int64 else FLOAT_FILL
    assert a.fill == want and bool((a.backing == want).all())
    if dtype == torch.float32:
        assert bool(torch.isnan(a.view).all())
    if dtype == torch.int32:
        assert bool((a.view == -1).all())
    if dtype == torch.int64:
        assert bool((a.view == 0x7F7F7F7F7F7F7F7F).all())  # far above any entity count, never negative
    a.check()
    a.poisoned()
    a.view.zero_()  # writing the whole interior touches no band
    a.check()
    with pytest.raises(AssertionError, match="interior byte"):
        a.poisoned()


def test_arena_reports_a_single_byte_in_either_band():
    for where, side, off in (("start - 1", "before", -1), ("end", "after", 0), ("first", "before", None),
                             ("last", "after", None)):
        a = arena(100, torch.float32, CPU, name="probe")
        n = a.backing.numel()
        pos = {"start - 1": a.start - 1, "end": a.end, "first": 0, "last": n - 1}[where]
        want = off if off is not None else (-a.start if where == "first" else n - 1 - a.end)
        a.backing[pos] = 0
        assert a.violations() == [(side, want, 1)], where
        with pytest.raises(AssertionError, match=rf"arena probe: 1 byte\(s\) written {side} the buffer, "
                                                 rf"first at offset {want} "):
            a.check()
    # both sides at once, several bytes: the first offset and the count of each
    a = arena(100, torch.float32, CPU)
    a.backing[a.start - 8:a.start - 4] = 1
    a.backing[a.end + 12:a.end + 15] = 1
    assert a.violations() == [("before", -8, 4), ("after", 12, 3)]
    # a write of the fill byte itself cannot be seen (0xFF over 0xFF): the fill is chosen so that
    # no float, id or count the library writes consists of it
    a = arena(4, torch.float32, CPU)
    a.backing[a.end] = FLOAT_FILL
    a.check()


def test_arena_unchanged_sees_one_bit():
    src = torch.arange(12, dtype=torch.float32).view(3, 4)
    a = arena_of(src, CPU)
    a.unchanged(src)
    a.unchanged(a.host())
    a.bytes[17] ^= 0x10
    with pytest.raises(AssertionError, match="changed in 1 byte.*first at byte 17"):
        a.unchanged(src)
    # NaN payloads are compared as bytes, not as floats
    b = arena((2,), torch.float32, CPU)
    h = b.host()
    b.unchanged(h)
    b.bytes[0] ^= 0x01
    with pytest.raises(AssertionError):
        b.unchanged(h)
    ids = arena_of(np.array([[1, 2, 3]], dtype=np.int64), CPU)
    ids.unchanged(np.array([[1, 2, 3]], dtype=np.int64))
    with pytest.raises(AssertionError):
        ids.unchanged(np.array([[1, 2, 4]], dtype=np.int64))


# ------------------------------------------------------------ size queries
def _desc(shape, shift=0):
    """A descriptor over host memory (the size queries dereference nothing)."""
    ent = arena((shape.E, shape.le), torch.float32, CPU, phase=0)
    rel = arena((shape.R, shape.lr), torch.float32, CPU)
    mod = arena((1, 1), torch.float32, CPU) if shape.name == "pRotatE" else None
    d = ops.make_desc(shape.name, ent.view, rel.view, A.GAMMA, 0.05, None if mod is None else mod.view)
    d.entity_embedding += shift
    return d, (ent, rel, mod)


@pytest.mark.parametrize("shape", A.ALL_SHAPES, ids=lambda s: s.id)
def test_workspace_queries_are_stable(shape):
    """Every *_workspace_bytes query of the GPU module's cases: the same value on two calls and
    with the entity table 256 bytes further on (the layouts are offsets relative to the
    workspace base and depend on shapes and on the tables' 16-byte alignment class only)."""
    lib = _lib.load()
    d, keep = _desc(shape)
    first = A.workspace_queries(lib, d)
    assert all(isinstance(v, int) and v > 0 for v in first.values()), first
    assert A.workspace_queries(lib, d) == first
    d2, keep2 = _desc(shape, shift=256)
    assert A.workspace_queries(lib, d2) == first


# ----------------------------------------------------- filter array length
def test_check_filter_shape():
    """The device reads filt_off at q, q + 1 (per-query lists) or at every query's key (whole
    index): an array of another length is refused on the host."""
    d = _lib.ModelDesc()
    d.nentity, d.nrelation = 257, 5
    nq = 65
    ops._check_filter_shape(d, nq, torch.zeros(nq + 1, dtype=torch.int64), False)
    ops._check_filter_shape(d, nq, torch.zeros(257 * 5 + 1, dtype=torch.int64), True)
    for off, table in ((torch.zeros(nq + 1, dtype=torch.int64), True),
                       (torch.zeros(257 * 5 + 1, dtype=torch.int64), False),
                       (torch.zeros(nq, dtype=torch.int64), False),
                       (torch.zeros(257 * 5, dtype=torch.int64), True),
                       (torch.zeros(nq + 1, 1, dtype=torch.int64), False),
                       (torch.zeros(1, 257 * 5 + 1, dtype=torch.int64), True)):
        with pytest.raises(ValueError, match="filter offsets"):
            ops._check_filter_shape(d, nq, off, table)
