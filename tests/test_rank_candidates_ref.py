"""The candidate-list cases' expectations are self-consistent (CPU): planted
copies of the true row give exactly the tie counts planned, padding and the
inputs' shape are what the GPU tests assume, and the pRotatE inputs have no
query the GPU test would have to excuse."""
import numpy as np
import pytest

import rank_candidates_cases as K
from knowledgegraphembedding_amd.sampler import true_lists_for

SMALL = [c for c in K.ALL_CASES if c.nq * c.C * c.d <= 200000]


@pytest.mark.parametrize("case", K.PLANTED, ids=[c.id for c in K.PLANTED])
@pytest.mark.parametrize("mode", K.MODES)
def test_planted_ties(case, mode):
    ranks, ties = K.reference(case, mode)
    n = K.N_TRUE // 2
    s, c = K.scores(case, mode), K.cand(case, mode)
    nud0 = K.N_TRUE + K.N_COPY * K.N_TRUE
    is_nudged = (c[:n] >= nud0) & (c[:n] < nud0 + K.N_NUDGE * K.N_TRUE)
    assert is_nudged.sum() == K.N_NUDGE * n
    # the exact copies (and the true id itself) tie as planned; a nudged copy is
    # a near-tie that may round onto the true score; nothing else ties
    eq = s[:n, 1:] == s[:n, :1]
    assert np.array_equal((eq & ~is_nudged).sum(1), K.planned_ties(case, mode))
    assert np.array_equal(ties[:n], K.planned_ties(case, mode) + (eq & is_nudged).sum(1))
    # near-ties of mixed outcome: within 1e-2 of the true score, not all equal to it
    d = np.abs(s[:n, 1:].astype(np.float64) - s[:n, :1])[is_nudged]
    assert (d > 0).any() and d.max() < 1e-2 * max(1.0, float(np.abs(s[:n, 0]).max()))
    # an exact copy scores the true score bit for bit
    is_copy = (c[:n] >= K.N_TRUE) & (c[:n] < nud0)
    own = is_copy & ((c[:n] - K.N_TRUE) // K.N_COPY == K.true_ids(case, mode)[:n, None])
    assert (s[:n, 1:][own] == np.broadcast_to(s[:n, :1], own.shape)[own]).all()


@pytest.mark.parametrize("case", K.PROTATE_CASES, ids=[c.id for c in K.PROTATE_CASES])
@pytest.mark.parametrize("mode", K.MODES)
def test_protate_inputs_excuse_no_query(case, mode):
    assert not K.excusable(case, mode).any()
    # copies of the true id are there, and they are exact ties
    _, ties = K.reference(case, mode)
    has_copy = (K.cand(case, mode) == K.true_ids(case, mode)[:, None]).sum(1)
    assert has_copy.sum() >= case.nq // 3 and np.array_equal(ties, has_copy)


@pytest.mark.parametrize("case", K.PADDED, ids=[c.id for c in K.PADDED])
@pytest.mark.parametrize("mode", K.MODES)
def test_padding_rows(case, mode):
    c = K.cand(case, mode)
    ranks, ties = K.reference(case, mode)
    assert (c[0, :5] == -1).all() and (c[2, -9:] == -1).all() and (c[4] == -1).all()
    assert c[1, 0] >= 0 and c[1, case.C // 2] == -1 and c[1, -1] >= 0
    assert ranks[4] == 1 and ties[4] == 0
    # padding is skipped, not scored as entity 0: masking changes the counts somewhere
    unmasked = K.count(K.scores(case, mode), np.ones_like(c, dtype=bool))
    assert (unmasked[0] >= ranks).all() and (unmasked[0] != ranks).any()


@pytest.mark.parametrize("case", SMALL, ids=[c.id for c in SMALL])
def test_inputs(case):
    for mode in K.MODES:
        c, q = K.cand(case, mode), K.queries(case)
        assert c.shape == (case.nq, case.C) and c.dtype == np.int64 and c.max() < case.E and c.min() >= -1
        assert q.shape == (case.nq, 3) and q.min() >= 0 and q[:, 1].max() < K.R
        ranks, ties = K.reference(case, mode)
        assert ranks.dtype == np.int64 and ties.dtype == np.int32
        assert ranks.min() >= 1 and (ranks + ties <= 1 + (c >= 0).sum(1)).all()
        if case.C >= 31 and case.nq >= 5 and not case.plant:
            # drawn with replacement: duplicates, and copies of the true id (exact ties)
            assert any(len(np.unique(r[r >= 0])) < (r >= 0).sum() for r in c)
            assert ((c == K.true_ids(case, mode)[:, None]).sum(1) <= ties).all() and ties.max() >= 1


def test_cases_cover_every_path():
    """Slots per row on both sides of each prefetch depth (128 / 256 / 512), of
    both slot kinds, and rows on both sides of the LDS staging threshold."""
    from conftest import dims

    def slots(c):
        le = dims(c.name, c.d)[0]
        span = le // 2 if c.name in ("ComplEx", "RotatE") else le
        v4 = span % 4 == 0 and c.aligned
        return ("v4" if v4 else "f"), (le // 4 if v4 else le), le

    seen = {("v4", 0): 0, ("v4", 1): 0, ("v4", 2): 0, ("v4", 3): 0, ("f", 0): 0, ("f", 1): 0, ("f", 2): 0, ("f", 3): 0,
            "in_place": 0}
    for c in K.ALL_CASES:
        kind, n, le = slots(c)
        if ((le + 3) & ~3) * 2 + 1028 > 16384:
            seen["in_place"] += 1
        else:
            seen[(kind, 0 if n <= 128 else 1 if n <= 256 else 2 if n <= 512 else 3)] += 1
    assert all(v > 0 for v in seen.values()), seen
    assert max(c.nq for c in K.ALL_CASES) > 65535
    # ... and a row of exactly the last slot count of each depth and of the next
    # one up (four floats on for the widest single-float rows), between the three
    # case tables whose kernels share the walk
    import rank_relations_cases as KR
    import rank_shard_cases as KS
    exact = {slots(c)[:2] for c in K.ALL_CASES + KR.ALL_CASES + KS.ALL_CASES}
    want = {(k, n) for k in ("v4", "f") for n in (128, 129, 256, 257, 512)} | {("v4", 513), ("f", 516)}
    assert want <= exact, want - exact


def test_true_lists_lookup():
    """true_lists_for: TrueLists' grouping looked up per query."""
    g = np.random.default_rng(2)
    tr = np.stack([g.integers(0, 30, 500), g.integers(0, 4, 500), g.integers(0, 30, 500)], 1).astype(np.int64)
    q = np.concatenate([tr[:40], [[29, 3, 0], [0, 0, 29]]])
    for mode, kcol, mcol in (("head-batch", (1, 2), 0), ("tail-batch", (0, 1), 2)):
        off, ln, ids = true_lists_for(tr, q, mode, 30, 4)
        for i, row in enumerate(q):
            want = sorted({int(t[mcol]) for t in tr if t[kcol[0]] == row[kcol[0]] and t[kcol[1]] == row[kcol[1]]})
            assert ids[off[i]:off[i] + ln[i]].tolist() == want
