"""The top-k cases against the oracle alone (no device): the inputs that
test_topk_gpu.py checks are well formed, and enough of each case's queries
qualify for its exact-set check (d) that the GPU test cannot hide behind
skipped queries.
"""
import numpy as np
import pytest

import topk_cases as T


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("name", T.NAMES)
def test_qualification_share(name, mode):
    """At least 80 % of each case's queries have a clear fp64 gap between
    the k-th and (k+1)-th unexcluded score, k in {1, 10}, unfiltered and
    filtered."""
    s64 = T.s64_of(name, mode)
    assert s64.shape == (T.NQ, T.E) and np.isfinite(s64).all()
    none = np.zeros_like(T.mask_of(mode))
    for mask in (none, T.mask_of(mode)):
        for k in (1, 10):
            ok, top = T.qualifying(s64, mask, k)
            assert ok.mean() >= 0.8, f"{name} {mode} k={k}: only {ok.mean():.3f} of the queries qualify"
            assert top.shape == (T.NQ, k) and not np.take_along_axis(mask, top, 1).any()


@pytest.mark.parametrize("mode", T.MODES)
def test_filter_is_a_real_filter(mode):
    """Some lists are long, some empty, and the per-query lists equal what
    FilterIndex.filter_csr gives with -1 in the predicted column."""
    from knowledgegraphembedding_amd.filters import FilterIndex
    mask = T.mask_of(mode)
    per = mask.sum(1)
    assert per.max() >= 20 and per.min() <= 2 and per.sum() > 0
    q = T.queries().copy()
    q[:, 0 if mode == "head-batch" else 2] = -1
    off, ids = FilterIndex(T.true_triples(), T.E, T.R).filter_csr(q, mode)
    want_off, want_ids = T.csr_of(mask)
    assert np.array_equal(off, want_off)
    for i in range(T.NQ):
        assert np.array_equal(np.sort(ids[off[i]:off[i + 1]]), want_ids[off[i]:off[i + 1]])


def test_tie_rows_score_equal():
    """The tie table's five rows are copies, so the oracle scores them equal."""
    for name in T.NAMES:
        s = T.s64_of(name, "tail-batch", ties=True)
        for r in T.TIE_ROWS[1:]:
            assert np.array_equal(s[:, r], s[:, T.TIE_ROWS[0]])


def test_checker_rejects_wrong_answers():
    """check_result fails a result with a swapped-in worse candidate, a wrong
    score and a broken tie order."""
    s64 = T.s64_of("TransE", "tail-batch")
    mask = np.zeros(s64.shape, dtype=bool)
    k = 10
    order = np.argsort(-s64, axis=1, kind="stable")
    ids = order[:, :k].astype(np.int64)
    sc = np.take_along_axis(s64, ids, 1).astype(np.float32)
    T.check_result(ids, sc, s64, mask, k, exact=True)
    bad = ids.copy()
    bad[0, k - 1] = order[0, 500]
    bs = sc.copy()
    bs[0, k - 1] = s64[0, order[0, 500]]
    with pytest.raises(AssertionError):
        T.check_result(bad, bs, s64, mask, k, exact=False)
    bs = sc.copy()
    bs[3, 0] += 0.01
    with pytest.raises(AssertionError):
        T.check_result(ids, bs, s64, mask, k, exact=False)
    m2 = mask.copy()
    m2[5, ids[5, 2]] = True
    with pytest.raises(AssertionError):
        T.check_result(ids, sc, s64, m2, k, exact=False)
