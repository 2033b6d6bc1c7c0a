"""CPU checks of the near-tie list cases (tests/rank_tie_cases.py): that every
table test_rank_ties_gpu.py ranks really holds what the device tests rely on —
the plants tie the true score exactly in the fp32 reference order, the nudged
rows fall on both sides of it, the filter leaves exactly p_j plants per query,
the ladder of p_j crosses the list cap whatever a path's window adds, and the
oracle row is the bit pattern of oracle.forward.
"""
import numpy as np
import pytest

import rank_tie_cases as T
from knowledgegraphembedding_amd.filters import FilterIndex

CASE_IDS = [c.id for c in T.ALL_CASES]


@pytest.mark.parametrize("case", T.ALL_CASES, ids=CASE_IDS)
def test_shape_and_ladder(case):
    p = T.ladder(case)
    assert case.E == T.C + case.n_other and case.E % 2 == 1 and case.E % 32 != 0
    assert len(p) % 4 != 0  # k_rank_exact's last block is partial
    assert set(T.SMALL_P) <= set(p.tolist())
    # listed = p + x with 1 <= x <= N_other (less the shelf): every x puts one query at the cap
    # and one just past it, at least 12 at or under it and some further past it
    assert set(range(T.CAP - case.n_loose, T.CAP + 7)) <= set(p.tolist())
    for x in (1, case.n_loose):
        listed = p + x
        assert (listed == T.CAP).any() and (listed == T.CAP + 1).any()
        assert (listed <= T.CAP).sum() >= 12 and (listed > T.CAP + 1).any()
    ent, rel, mod, _ = T.tables(case)
    assert ent.shape[0] == case.E and rel.shape[0] == len(p)
    assert (ent[:T.C] == ent[0]).all() and (ent[-1] == ent[0]).all() and (rel == rel[0]).all()
    q = T.queries(case)
    assert (q[:, [0, 2]] < T.C).all() and np.array_equal(q[:, 1], np.arange(len(p)))


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("case", T.ALL_CASES, ids=CASE_IDS)
def test_score_row(case, mode):
    s, st = T.score_row(case, mode)
    # every plant, and the last row, scores exactly the true score
    assert (s[:T.C] == st).all() and s[-1] == st
    # the oracle's forward gives the same bits
    assert np.array_equal(T.forward_row(case, mode).view(np.uint32), s.view(np.uint32))
    nud = s[T.C:T.C + case.U + case.D]
    if len(nud):
        above, below, equal = int((nud > st).sum()), int((nud < st).sum()), int((nud == st).sum())
        print(f"{case.id} {mode}: nudged rows {above} above, {equal} equal, {below} below")
        assert above >= 4 and below >= 4
    if case.name == "pRotatE":
        # (the last row is an exact copy: the same value under any sin)
        # twice what a 1-ulp sin difference per element, in the candidate's and
        # the true score, can move a score: the correctly rounded sin that ranks
        # a query with more than a list of undecided candidates counts the same
        mod = T.tables(case)[2]
        far = 8 * case.d * 2.0 ** -24 * abs(float(mod[0, 0]))
        gap = np.abs(s[T.C:-1].astype(np.float64) - float(st))
        assert gap.min() >= far, (gap.min(), far)
    if case.shelf:
        s0 = T.C + case.U + case.D
        sh = s[s0:s0 + case.shelf].astype(np.float64) - float(st)
        unit = 2.0 ** -24 * abs(float(T.tables(case)[2][0, 0]))
        assert (np.abs(sh) >= 0.45 * case.shelf_T * unit).all() and (np.abs(sh) <= 2.2 * case.shelf_T * unit).all()
        assert min((sh > 0).sum(), (sh < 0).sum()) >= case.shelf // 2 - 1


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("case", T.ALL_CASES, ids=CASE_IDS)
def test_filter_and_reference(case, mode):
    p, q = T.ladder(case), T.queries(case)
    index = FilterIndex(T.true_triples(case), case.E, len(q))
    off, ids = index.filter_csr(q, mode)
    assert np.array_equal(np.diff(off), T.C - 1 - p)
    mask = T.filtered_mask(case, mode)
    for j in (0, len(q) // 2, len(q) - 1):
        assert np.array_equal(np.sort(ids[off[j]:off[j + 1]]), np.nonzero(mask[j])[0])
    assert not mask[:, T.C:].any()  # only plants are filtered
    # not a prefix: filtered and unfiltered plants inside the same 32-bit word
    word = mask[len(q) - 1, :T.C - T.C % 32].reshape(-1, 32).sum(1)
    assert ((word > 0) & (word < 32)).sum() >= 8
    ranks, ties = T.reference(case, mode)
    s, st = T.score_row(case, mode)
    n_above = int((s[T.C:] > st).sum())  # non-plants are never filtered
    assert (ranks == 1 + n_above).all()
    assert np.array_equal(ties, p + int((s[T.C:] == st).sum())) and (ties >= p + 1).all()
