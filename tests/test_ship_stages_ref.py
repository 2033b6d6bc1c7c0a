"""The input conditions tests/test_ship_stages_gpu.py relies on, asserted on the
committed inputs (CPU, no GPU), so that a change of seed cannot silently remove
them; and the cap on the two extra cases.

Shard patterns and the driver: tests/ship_cases.py.  Cases, inputs and the fp64
reference: tests/test_slot_matrix_ref.py, unchanged.
"""
import numpy as np
import pytest

from ship_cases import PATTERNS, WIDE_N, shard_of, shards, split_rows, starved_rows
from test_slot_matrix_ref import (ALL_SLOTS, B, CASES_B, CASES_D, MODES, NAMES, RHO_CAP, inputs, references,
                                  true_column)

D_SHIP = [c for c in CASES_D if c.kind in ("peaked", "saturated", "uneven")]


def test_patterns():
    """W1 one shard; W2 the D geometry; W3 a shard of one row and one of most of the table; W4
    an empty shard in the middle and uneven shards."""
    assert shards(PATTERNS["W1"]) == [(0, 40)]
    assert shards(PATTERNS["W2"]) == [(0, 20), (20, 40)]
    assert (39, 40) in shards(PATTERNS["W3"]) and (0, 33) in shards(PATTERNS["W3"])
    w4 = shards(PATTERNS["W4"])
    assert w4[1] == (5, 5) and 0 < 1 < len(w4) - 1 and len({hi - lo for lo, hi in w4}) == len(w4)
    assert shard_of(PATTERNS["W4"], [0, 4, 5, 22, 23, 39, 40, -1]).tolist() == [0, 0, 2, 2, 3, 3, -1, -1]


@pytest.mark.parametrize("pattern", ["W4", "W3"])
def test_every_instantiation_meets_the_shard_conditions(pattern):
    """Per (model, mode, (vec, ns)) over CASES_B: at least one case has a row whose h and t live
    in different shards (W4 only), one a row whose h and t live in the same shard, and one a row
    with no negative in some non-empty shard (that shard's -inf partial state)."""
    cuts = PATTERNS[pattern]
    seen = {}
    for case in CASES_B:
        inp = inputs(case)
        split = split_rows(inp.pos, cuts)
        for mode in MODES:
            s = seen.setdefault((case.name, mode) + case.slots, [False, False, False])
            s[0] |= bool(split.any())
            s[1] |= bool((~split).any())
            s[2] |= bool(starved_rows(inp.neg[mode], cuts).any())
    assert set(seen) == {(nm, mode) + sl for nm in NAMES for mode in MODES for sl in ALL_SLOTS}
    for key, (diff, same, starved) in seen.items():
        assert (diff or pattern == "W3") and same and starved, (pattern, key, diff, same, starved)


@pytest.mark.parametrize("case", D_SHIP, ids=lambda c: c.id)
def test_trained_regime_shard_geometry(case):
    """Under W2 the true entity's column (true_column) is the row's one negative in shard 0 and
    every random negative is in shard 1, so the dominant negative sits alone in its shard and
    every other shard's state is rescaled by exp(-spread) (saturated DistMult / ComplEx: column 1,
    the negative that scores -2.2 × the positive, is an entity below 20 and shares shard 0 with
    it); under W4 every row's h and t live in different shards."""
    inp = inputs(case)
    col = np.broadcast_to(true_column(case.n), (B,))
    fixed = case.kind == "saturated" and case.name in ("DistMult", "ComplEx")  # column 1: the -2.2 × negative
    for mode in (t.mode for t in inp.trains):
        own = shard_of(PATTERNS["W2"], inp.neg[mode])
        for i in range(B):
            in0 = set(np.flatnonzero(own[i] == 0).tolist())
            assert in0 == ({int(col[i]), 1} if fixed else {int(col[i])}), (mode, i, own[i])
            assert set(own[i].tolist()) == {0, 1}
    assert split_rows(inp.pos, PATTERNS["W4"]).all()


def test_rank_guards_see_what_they_are_there_for():
    """run_ship's per-rank record on CPU tensors: a write inside the owned rows of a sharded
    table or anywhere in an output passes; a byte changed in a band, in a read-only buffer or in
    a row outside [lo, hi) is counted, and explain() names the arena (and the row)."""
    import torch
    from ship_cases import _Rank
    full = np.arange(40 * 8, dtype=np.float32).reshape(40, 8)

    def rank():
        k = _Rank(torch.device("cpu"), 5, 23)
        k.rows("table", full, ro=True)
        k.rows("grad_entity", full, ro=False, copy=False)
        k.put("pos", np.zeros((5, 3), dtype=np.int64))
        k.out("q", (5, 8))
        k.seal()
        return k

    k = rank()
    assert torch.equal(k.arenas["table"].view[5:23], torch.from_numpy(full[5:23]))
    assert torch.isnan(k.arenas["table"].view[:5]).all() and torch.isnan(k.arenas["table"].view[23:]).all()
    k.arenas["grad_entity"].view[5:23] = 1.0
    k.arenas["q"].view.zero_()
    assert int(k.dirty()) == 0
    for name, hit, says in (("grad_entity", lambda a: a.view[4:5].zero_(), "row 4"),
                            ("grad_entity", lambda a: a.view[23:24].zero_(), "row 23"),
                            ("table", lambda a: a.view[7:8].zero_(), "row 7"),
                            ("pos", lambda a: a.view[0:1].fill_(7), "arena pos"),
                            ("q", lambda a: a.backing[a.end:a.end + 1].zero_(), "after the buffer"),
                            ("q", lambda a: a.backing[a.start - 1:a.start].zero_(), "before the buffer")):
        k = rank()
        hit(k.arenas[name])
        assert int(k.dirty()) > 0, (name, says)
        with pytest.raises(AssertionError, match=says):
            k.explain("stage")


@pytest.mark.parametrize("case", WIDE_N, ids=lambda c: c.id)
def test_wide_negative_cases(case):
    """n > 256: k_ship_merge's j loop strides; under W4 some shard owns more than 64 and fewer
    than 256 of every row's negatives; rho_case within the slot matrix's cap."""
    assert case.n > 256
    inp = inputs(case)
    for mode in MODES:
        own = shard_of(PATTERNS["W4"], inp.neg[mode])
        for i in range(B):
            counts = [int((own[i] == k).sum()) for k in range(len(PATTERNS["W4"]) - 1)]
            assert any(64 < c < 256 for c in counts) and sum(counts) == case.n, (mode, i, counts)
    assert references(case).rho <= RHO_CAP, references(case).rho
