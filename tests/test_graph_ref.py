"""The second input set of every case of tests/test_graph_gpu.py, built on the
CPU (no GPU needed; run before the GPU module, the seeds are fixed here).

test_graph_gpu.py replays a captured graph after overwriting, in place, every
array the graph reads with a second set: the same Shape under another seed
(graph_cases.second), through test_arena_gpu's tables / batch / refs and the
rank_inputs / filters_of recipes.  Two things must hold for that replay to mean
anything, and neither needs a device:

  1. the second set's fp32 oracle is within test_slot_matrix_ref's cap of the
     fp64 one (refs() asserts rho_case <= RHO_CAP; a seed that misses it is
     replaced in graph_cases.SEEDS2, the cap stays);
  2. the second set differs from the first in every array that is overwritten
     (entity and relation tables, pos, neg of both modes, subsampling_weight,
     grad_scores of the three modes, queries, both filter forms of both
     directions, candidate lists, the relation ranking's filter), and has the
     first set's shapes, so a replay that ignored the new contents cannot meet
     the second set's reference.  pRotatE's [1, 1] modulus is 0.5 · the
     embedding range, a function of gamma and the span alone: it is the one
     input both sets share.
"""
import numpy as np
import pytest

import graph_cases as G
import rank_candidates_cases as RC
import rank_relations_cases as RR
import test_slot_matrix_ref as S
from test_arena_gpu import MODES, batch, filters_of, rank_inputs, refs, tables


def differ(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    assert not np.array_equal(a, b), f"{what}: the second set equals the first"


@pytest.mark.parametrize("shape", G.TRAIN_SHAPES, ids=lambda s: s.id)
def test_second_set_meets_the_cap_and_differs(shape):
    two = G.second(shape)
    r1, r2 = refs(shape, G.N), refs(two, G.N)  # (refs asserts rho <= S.RHO_CAP)
    print(f"{shape.id}: seed {shape.seed} rho {r1.rho:.3e}, seed {two.seed} rho {r2.rho:.3e}")
    assert r2.rho <= S.RHO_CAP and r2.rtol == max(8.0 * r2.rho, S.RTOL_MIN)
    (e1, l1, m1, g1), (e2, l2, m2, g2) = tables(shape), tables(two)
    differ(e1, e2, "entity")
    differ(l1, l2, "relation")
    assert g1 == g2 and (m1 is None) == (m2 is None)
    i1, i2 = batch(shape, G.N), batch(two, G.N)
    differ(i1.pos, i2.pos, "pos")
    differ(i1.w, i2.w, "subsampling_weight")
    for mode in MODES:
        differ(i1.neg[mode], i2.neg[mode], f"neg {mode}")
        assert not (i2.pos[:, 0] == i2.pos[:, 2]).any()
    for mode in ("single",) + MODES:
        differ(i1.gout[mode], i2.gout[mode], f"grad_scores {mode}")
    assert [t for t in i1.trains] == [t for t in i2.trains]
    # the fp64 references of the two sets are apart by far more than any bound used on them
    for (la, ga), (lb, gb) in zip(r1.train, r2.train):
        assert S.ratio_of(ga[0].astype(np.float32), gb[0], r2.rtol) > 1.0


@pytest.mark.parametrize("shape", G.E257 + (G.SINGLE,), ids=lambda s: s.id)
def test_second_set_of_the_ranking_inputs_differs(shape):
    two = G.second(shape)
    (q1, t1), (q2, t2) = rank_inputs(shape, G.NQ), rank_inputs(two, G.NQ)
    differ(q1, q2, "queries")
    assert len(t1) and len(t2)
    for mode in MODES:
        for table in (False, True):
            (o1, i1), (o2, i2) = filters_of(shape, G.NQ, mode, table), filters_of(two, G.NQ, mode, table)
            differ(o1, o2, f"filt_off {mode} table={table}")
            assert len(i1) and len(i2) and not np.array_equal(i1[:min(len(i1), len(i2))], i2[:min(len(i1), len(i2))])


@pytest.mark.parametrize("name", G.A.NAMES)
def test_second_set_of_the_candidate_and_relation_cases_differs(name):
    c1 = RC.Case(name, 36, E=257, nq=G.NQ, C=65, pad=True)
    c2 = G.second(c1)
    differ(RC.tables(c1)[0], RC.tables(c2)[0], "entity")
    differ(RC.queries(c1), RC.queries(c2), "queries")
    for mode in MODES:
        differ(RC.cand(c1, mode), RC.cand(c2, mode), f"cand {mode}")
    r1 = RR.Case(name, 36, R=65, E=257, nq=G.NQ)
    r2 = G.second(r1)
    differ(RR.tables(r1)[1], RR.tables(r2)[1], "relation")
    differ(RR.queries(r1), RR.queries(r2), "queries")
    # (the relation filter's list lengths depend on the query's number alone: the offsets are
    # the same in both sets, the listed ids are not)
    differ(RR.filt(r1)[1], RR.filt(r2)[1], "filt_ids")
