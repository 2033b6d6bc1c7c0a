"""The expected values of the sharded filtered ranking tests, checked on the CPU
against the oracle's own filtered ranking: for every case of
tests/rank_shard_cases.py, mode and world, the per-shard counts of the fp32
reference-order oracle sum to oracle.filtered_ranks' rank_count − 1 and ties
(KGEModel.forward's scores with TestDataset's filter), the planted exact ties
land in the shards intended, both filter forms exclude the same ids, and the
pRotatE inputs excuse no query.

oracle.filtered_ranks loops over the queries in Python (a forward in fp32 and one
in fp64 each), so the 70,001-query case is compared on every 293rd query (239
of them, the first and the last included); its per-shard sums are still checked
for all queries against the one-shard world.
"""
import numpy as np
import pytest
import torch

import rank_shard_cases as S
from oracle import kge_oracle as O


def _subset(case):
    return np.arange(case.nq) if case.nq <= 1000 else np.unique(np.append(np.arange(0, case.nq, 293), case.nq - 1))


@pytest.mark.parametrize("case", S.ALL_CASES, ids=[c.id for c in S.ALL_CASES])
def test_shard_counts_sum_to_the_filtered_rank(case):
    ent, rel, mod, erange = S.tables(case)
    sub = _subset(case)
    for mode in S.MODES:
        whole = S.shard_counts(case, mode, 0, case.E)
        for world, shards in S.splits(case.E).items():
            assert shards[0][0] == 0 and shards[-1][1] == case.E
            assert all(a[1] == b[0] for a, b in zip(shards, shards[1:])), world  # the shards tile [0, E)
            tot = sum(S.shard_counts(case, mode, b, e) for b, e in shards)
            assert np.array_equal(tot, whole), (case.id, mode, world)
        ref = O.filtered_ranks(case.name, torch.from_numpy(ent.copy()), torch.from_numpy(rel.copy()),
                               None if mod is None else torch.from_numpy(mod.copy()), S.queries(case)[sub],
                               S.all_true(case), mode, S.GAMMA, erange)
        # (pRotatE: filtered_ranks takes torch's sin, the cases the correctly rounded one; no query of
        # these inputs has a near-tie for the last bit to decide, test_protate_inputs_excuse_no_query)
        assert np.array_equal(ref["rank_count"] - 1, whole[0][sub]), (case.id, mode)
        assert np.array_equal(ref["ties"], whole[1][sub]), (case.id, mode)


@pytest.mark.parametrize("case", [c for c in S.ALL_CASES if c.plant], ids=lambda c: c.id)
def test_planted_ties_land_in_their_shards(case):
    for world, shards in S.splits(case.E).items():
        plan = S.planned_tie_shard(case, world)
        assert len(plan) == len(S.PLANT_ROWS)
        for (j, mode), i in plan.items():
            b, e = shards[i]
            assert S.shard_counts(case, mode, b, e)[1][j] >= 1, (case.id, world, j, mode)
            # the exact copy is the query's only tie, but for its next-float copy, whose one moved
            # coordinate may round away in the sum
            nudge = (S.NUDGE_H if mode == "head-batch" else S.NUDGE_T) + j
            s = S.scores(case, mode)[j]
            total = sum(S.shard_counts(case, mode, bb, ee)[1][j] for bb, ee in shards)
            assert total == 1 + int(s[1 + nudge] == s[0]), (case.id, world, j, mode)
    # every shard boundary of every world has a planted row on either side
    for shards in S.splits(case.E).values():
        for b, e in shards:
            for p in (b - 1, b, e - 1, e):
                assert p in S.PLANT_ROWS or p < 0 or p >= case.E, (b, e, p)


@pytest.mark.parametrize("case", S.BASE + S.MANY, ids=lambda c: c.id)
def test_filter_forms_agree(case):
    for mode in S.MODES:
        off, ids = S.filter_lists(case, mode)
        toff, tids = S.filter_table(case, mode)
        assert off.shape == (case.nq + 1,) and toff.shape == (case.E * S.R + 1,) and toff[-1] == len(tids)
        tid = S.true_ids(case, mode)
        n = min(case.nq, 500)
        lens = np.diff(off)[:n]
        for j in range(n):
            l = ids[off[j]:off[j + 1]]
            assert set(l.tolist()) - {int(tid[j])} == set(np.nonzero(S.excluded(case, mode)[j])[0].tolist())
        assert any(tid[j] in ids[off[j]:off[j + 1]] for j in range(1, n, 5))
        if case.E == 301:  # lists that are empty, hold duplicates and span the shards
            assert (lens == 0).any()
            assert any(len(set(ids[off[j]:off[j + 1]].tolist())) < lens[j] for j in range(2, n, 5))
            longest = int(np.argmax(lens))
            l = ids[off[longest]:off[longest + 1]]
            assert l.min() < 76 and l.max() >= 228


@pytest.mark.parametrize("case", S.PROTATE_CASES, ids=lambda c: c.id)
def test_protate_inputs_excuse_no_query(case):
    for mode in S.MODES:
        assert not S.excusable(case, mode).any(), mode
