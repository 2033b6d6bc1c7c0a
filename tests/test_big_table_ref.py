"""CPU checks of the big-table tests' reference construction (tests/big_table_cases.py);
nothing here runs a kernel.

1. The pooled reference is the reference: on a small expanded table (E = 5000,
   P = 256) that can be materialised, ranks and ties computed from pool scores
   and idx equal oracle.filtered_ranks on the table, and the expanded fp64
   scores equal topk_cases.oracle_scores on it, for all five models and both
   modes.
2. The cases can see a wrapped offset: for every GPU ranking and scoring case
   and each line its table crosses, the expected output recomputed with every
   id replaced by the row that an offset truncated at that line would address
   differs from the correct one in at least one query.
3. The sizes and lines of the issue's table (big_table_cases.check_sizes), and
   the shape of every id list.
"""
import numpy as np
import pytest
import torch

import big_table_cases as C
import topk_cases as T
from oracle import kge_oracle as O


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("name", C.NAMES)
def test_pooled_reference_is_the_reference(name, mode):
    sp = C.spec("small", name)
    ent, (_, rel), mod = C.materialise(sp), C.pool_of(sp), C.mod_of(sp)
    q = C.queries(sp)
    off, ids = C.filters(sp, mode)
    # the filter lists as an all_true_triples: query i's key is its own (r, t) / (h, r)
    keys = {(int(r), int(t)) if mode == "head-batch" else (int(h), int(r)) for h, r, t in q}
    assert len(keys) == len(q)
    true = [(int(e), int(r), int(t)) if mode == "head-batch" else (int(h), int(r), int(e))
            for i, (h, r, t) in enumerate(q) for e in ids[off[i]:off[i + 1]]]
    t = lambda a: None if a is None else torch.from_numpy(np.array(a))  # noqa: E731
    want = O.filtered_ranks(name, t(ent), t(rel), t(mod), q.tolist(), true, mode, C.GAMMA, sp.erange)
    ranks, ties = C.rank_reference(sp, mode)
    assert np.array_equal(ranks, want["rank_count"]) and np.array_equal(ties, want["ties"])
    assert ties.max() > 0 and ranks[C.ALL_FILTERED] == 1 and ties[C.ALL_FILTERED] == 0
    assert T.erange_of(sp.d) == sp.erange
    s64 = T.oracle_scores(name, ent, rel, mod, q, mode, d=sp.d)
    assert np.array_equal(C.pool_s64(sp, mode)[:, C.idx_of(sp)], s64)


def _differs(a, b):
    return any(not np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


RANK_LINES = [(sp, L) for sp in list(C.RANK_CASES) + [C.SENTINEL_CASE] for L in sp.table.lines]


@pytest.mark.parametrize("sp,line", RANK_LINES, ids=[f"{sp.id}-{L:#x}" for sp, L in RANK_LINES])
def test_ranking_cases_see_a_wrapped_offset(sp, line):
    for mode in C.MODES:
        good, bad = C.rank_reference(sp, mode), C.rank_reference(sp, mode, line)
        assert (good[1] > 0).sum() >= C.NQ - 1, "every query but the all-filtered one has exact ties"
        assert good[1].max() < 1024, "the near-tie lists stay under their cap"
        assert _differs(good, bad), (sp.id, mode, hex(line))


TOPK_LINES = [(sp, L) for sp in C.TOPK_CASES for L in sp.table.lines]


@pytest.mark.parametrize("sp,line", TOPK_LINES, ids=[f"{sp.id}-{L:#x}" for sp, L in TOPK_LINES])
def test_topk_cases_see_a_wrapped_offset(sp, line):
    for mode in C.MODES:
        good, bad = C.topk_reference(sp, mode, 10, nq=4), C.topk_reference(sp, mode, 10, line, nq=4)
        assert _differs(good, bad), (sp.id, mode, hex(line))


GATHER_LINES = [(sp, L) for sp in C.GATHER_CASES for L in sp.table.lines]


@pytest.mark.parametrize("sp,line", GATHER_LINES, ids=[f"{sp.id}-{L:#x}" for sp, L in GATHER_LINES])
def test_gather_cases_see_a_wrapped_offset(sp, line):
    for mode in ("single",) + C.MODES:
        assert _differs([C.score_reference(sp, mode)], [C.score_reference(sp, mode, line)]), (sp.id, mode)
    for mode in C.MODES:
        assert _differs(C.candidates_reference(sp, mode), C.candidates_reference(sp, mode, line)), (sp.id, mode)
    assert _differs(C.relations_reference(sp), C.relations_reference(sp, line)), sp.id


def test_sizes_lines_and_id_lists():
    C.check_sizes()
    for key, t in C.TABLES.items():
        for L in t.lines:  # the first row that starts at or past a line wraps to row 0, none before it wraps
            r = t.straddle(L)
            first = r if r * 4 * t.Le == L else r + 1  # (S8's rows are 4096 bytes: r_L starts on the line)
            w = C.wrapped_rows(t, L)
            assert w[first] == 0 and (w[:first] == np.arange(first)).all() and (w[first:] < first).all()
    for sp in list(C.RANK_CASES) + C.TOPK_CASES + C.GATHER_CASES:
        q = C.queries(sp)
        C.check_list(sp.table, q[:, 0]), C.check_list(sp.table, q[:, 2])
        assert len(q) == C.NQ
        for mode in C.MODES:
            off, ids = C.filters(sp, mode)
            assert off[C.ALL_FILTERED + 1] - off[C.ALL_FILTERED] == sp.table.E - 1
            assert ids.max() == sp.table.E - 1 and ids.min() == 0
    for sp in C.GATHER_CASES:
        C.check_list(sp.table, C.negatives(sp))
        for mode in C.MODES:
            c = C.candidates(sp, mode)
            assert c.shape == (C.NQ, C.NCAND) and (c == -1).sum() == 3
    hot = 0
    for tc in C.GRAD_CASES + C.STEP_CASES:
        pos, neg, w = C.train_batch(tc.spec, tc.n, tc.hot)
        assert pos.shape == (C.B, 3) and neg.shape == (C.B, tc.n) and w.shape == (C.B,)
        C.check_list(tc.spec.table, np.concatenate([pos[:, 0], pos[:, 2]]))
        if tc.n >= 16:
            C.check_list(tc.spec.table, neg)
        hot += int((neg == tc.spec.table.E - 1).sum() > 64)
    assert hot >= 1 and any(tc.n == 3 for tc in C.GRAD_CASES)
    # the sentinel case: +-3e38 in the 16 bytes at table offset 0x7FFFFFF0, nowhere else
    sp = C.SENTINEL_CASE
    row, col = divmod(C.SENTINEL // 4, sp.table.Le)
    pool, idx = C.pool_of(sp)[0], C.idx_of(sp)
    assert (np.abs(pool[idx[row], col:col + 4]) == np.float32(C.HUGE)).all()
    assert (np.abs(pool) > 1).sum() == 4 and (idx == sp.table.P - 1).sum() == 1
    assert row not in C.queries(sp)[:, [0, 2]]
