"""The expected values of the sharded candidate-list ranking tests, on the CPU:
per-shard counts from the oracle's scores restricted to the shard's ids sum,
over every world's shards, to rank_candidates_cases.reference; and the inputs
hold what the device tests rely on — chunks that mix owned and unowned
candidates, true ids listed as candidates whose owner is and is not the owner
of the query's fixed-side row, and no pRotatE query that could be excused.
"""
import numpy as np
import pytest

import rank_candidates_cases as K
import rank_candidates_shard_cases as X


@pytest.mark.parametrize("case", X.ALL_CASES, ids=[c.id for c in X.ALL_CASES])
def test_shard_counts_sum_to_reference(case):
    for mode in X.MODES:
        ranks, ties = K.reference(case, mode)
        for world in X.WORLDS:
            parts = [X.shard_counts(case, mode, b, e) for b, e in X.splits(case, world)]
            assert all(p.shape == (2, case.nq) and p.dtype == np.int64 for p in parts)
            tot = np.sum(parts, axis=0)
            assert np.array_equal(1 + tot[0], ranks), (case.id, mode, world)
            assert np.array_equal(tot[1], ties.astype(np.int64)), (case.id, mode, world)
            # an empty shard owns nothing
            for (b, e), p in zip(X.splits(case, world), parts):
                assert b < e or not p.any()


def test_own_case_is_new():
    assert not set(X.OWN) & set(K.ALL_CASES)


E301 = tuple(c for c in X.ALL_CASES if c.E == 301)


@pytest.mark.parametrize("world", ("w2", "w3", "w4"))
def test_inputs_cover_the_sharded_paths(world):
    """Every multi-rank world of the E = 301 cases has a chunk (of at most 1024 list places) with
    both owned and unowned candidates, and queries that list their true id whose true row is owned
    by the rank of the fixed side's row, and by another rank."""
    mixed = same = other = 0
    for case in E301:
        for mode in X.MODES:
            c, q, tid = K.cand(case, mode), K.queries(case), K.true_ids(case, mode)
            for b, e in X.splits(case, world):
                own = X.owned(case, mode, b, e)
                rest = (c >= 0) & ~own
                for j0 in range(0, case.C, X.CHUNK_MAX):
                    mixed += int((own[:, j0:j0 + X.CHUNK_MAX].any(1) & rest[:, j0:j0 + X.CHUNK_MAX].any(1)).sum())
            listed = (c == tid[:, None]).any(1)
            fixed = q[:, 2 if mode == "head-batch" else 0]
            o_true, o_fixed = X.owner(case, world, tid), X.owner(case, world, fixed)
            assert (o_true >= 0).all() and (o_fixed >= 0).all()
            same += int((listed & (o_true == o_fixed)).sum())
            other += int((listed & (o_true != o_fixed)).sum())
    print(f"{world}: {mixed} mixed (query, shard, chunk) units, true id listed: {same} on the fixed row's rank, "
          f"{other} on another")
    assert mixed > 0 and same > 0 and other > 0


@pytest.mark.parametrize("case", tuple(c for c in X.ALL_CASES if c.C >= 31 and c.E == 301), ids=lambda c: c.id)
def test_lists_span_the_shards(case):
    """With two and with four ranks every such case has a list split between ranks."""
    for world in ("w2", "w4"):
        for mode in X.MODES:
            n_own = np.stack([X.owned(case, mode, b, e).sum(1) for b, e in X.splits(case, world)])
            assert ((n_own > 0).sum(0) > 1).any(), (case.id, world, mode)


@pytest.mark.parametrize("case", K.PROTATE_CASES, ids=lambda c: c.id)
def test_protate_excuses_none(case):
    """pRotatE's cap: at most 5 % of the queries may be excused (a condition, not a measurement);
    these inputs excuse none, so the device tests ask for exact agreement."""
    for mode in X.MODES:
        ok = K.excusable(case, mode)
        assert ok.sum() <= 0.05 * case.nq
        assert not ok.any(), (case.id, mode, np.nonzero(ok)[0])
