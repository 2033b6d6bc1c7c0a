"""The relation-prediction cases' expectations are self-consistent (CPU): the
oracle's 'single'-mode reference-order scores are the torch forward's bits,
planted copies of the true relation row give exactly the tie counts planned and
the filter removes exactly the planned ones, the pRotatE inputs have no query
the GPU test would have to excuse, and FilterIndex.relation_csr equals a
brute-force lookup."""
import numpy as np
import pytest
import torch

import rank_relations_cases as K
from knowledgegraphembedding_amd.filters import FilterIndex

FORWARD = tuple(c for c in K.BASE if c.name != "pRotatE") + (K.WIDTHS[0],)


@pytest.mark.parametrize("case", FORWARD, ids=[c.id for c in FORWARD])
def test_oracle_single_scores_equal_forward(case):
    """(h, r', t) for every r' through the reference's forward(mode='single') as
    torch evaluates it on the CPU (oracle.forward): the oracle's reference-order
    [nq, R] scores bit for bit (TransE 37, DistMult 40, ComplEx 20, RotatE 20 at
    R = 61; RotatE 1000 at R = 9)."""
    ent, rel, mod, erange = K.tables(case)
    tr = torch.from_numpy(K.all_relation_triples(K.queries(case), case.R))
    with torch.no_grad():
        s = K.O.forward(case.name, torch.from_numpy(ent.copy()), torch.from_numpy(rel.copy()), None, tr, "single",
                        K.GAMMA, erange).numpy().reshape(case.nq, case.R)
    assert s.dtype == np.float32
    assert np.array_equal(s.view(np.int32), K.scores(case).view(np.int32))


@pytest.mark.parametrize("case", K.PLANTED, ids=[c.id for c in K.PLANTED])
def test_planted_ties(case):
    n = K.N_PLANTED_Q
    s, q = K.scores(case), K.queries(case)
    r = q[:n, 1]
    assert np.array_equal(r, np.arange(n) % K.N_TRUE)
    st = s[np.arange(n), r][:, None]
    eq = s[:n] == st
    ids = np.arange(case.R)[None, :]
    nud0 = K.N_TRUE + K.N_COPY * K.N_TRUE
    own_copy = (ids >= K.N_TRUE) & (ids < nud0) & ((ids - K.N_TRUE) // K.N_COPY == r[:, None])
    own_nudge = (ids >= nud0) & (ids < K.BG0) & ((ids - nud0) // K.N_NUDGE == r[:, None])
    assert (own_copy.sum(1) == K.N_COPY).all() and (own_nudge.sum(1) == K.N_NUDGE).all()
    # an exact copy scores the true score bit for bit; besides the true relation
    # itself only the copies and, possibly, a nudged copy tie
    assert eq[own_copy].all()
    assert not (eq & ~own_copy & ~own_nudge & (ids != r[:, None])).any()
    raw_rank, raw_ties = K.reference(case, False)
    assert np.array_equal(raw_ties[:n], K.N_COPY + (eq & own_nudge).sum(1))
    # near-ties of mixed outcome: within 1e-2 of the true score, not all equal to it
    d = np.abs(s[:n].astype(np.float64) - st)[own_nudge]
    assert (d > 0).any() and d.max() < 1e-2 * max(1.0, float(np.abs(st).max()))
    # the filter removes exactly the planned copies from the tie count
    f_rank, f_ties = K.reference(case, True)
    excl = K.excluded(case)
    for j in range(n):
        planned = K.planted_excluded(j)
        assert len(planned) == 1 + j % 3 and excl[j, planned].all()
        assert not excl[j, K.N_TRUE:K.BG0][~np.isin(np.arange(K.N_TRUE, K.BG0), planned)].any()
        assert f_ties[j] == raw_ties[j] - len(planned)
    assert (f_rank <= raw_rank).all() and (f_rank < raw_rank).any()


@pytest.mark.parametrize("case", K.ALL_CASES, ids=[c.id for c in K.ALL_CASES])
def test_inputs(case):
    q = K.queries(case)
    off, ids = K.filt(case)
    assert q.shape == (case.nq, 3) and q[:, 1].max() < case.R and q[:, 1].min() >= (-1 if case.pred else 0)
    assert off.shape == (case.nq + 1,) and off[-1] == len(ids) and (np.diff(off) >= 0).all()
    assert off[case.nq // 2] == off[case.nq // 2 + 1]  # an empty list
    own = lambda j: ids[off[j]:off[j + 1]]
    for j in (0, 1, case.nq - 1):
        assert (own(j) >= case.R).sum() == 1  # one id outside [0, R)
        assert q[j, 1] < 0 or q[j, 1] in own(j)  # the true r itself
    if case.R > 8:
        assert len(own(0)) > len(np.unique(own(0)))  # an id twice
    for filtered in (False, True):
        ranks, ties = K.reference(case, filtered)
        assert ranks.dtype == np.int64 and ties.dtype == np.int32
        has = q[:, 1] >= 0
        assert (ranks[has] >= 1).all() and (ranks[~has] == 0).all() and (ties[~has] == 0).all()
        assert (ranks + ties <= case.R).all()
    if case.R == 1:
        assert (K.reference(case, False)[0] == 1).all() and (K.reference(case, False)[1] == 0).all()
    if case.pred:
        assert (q[(2, 5), 1] == -1).all() and (q[:, 1] >= 0).sum() == case.nq - 2


@pytest.mark.parametrize("case", K.PROTATE_CASES, ids=[c.id for c in K.PROTATE_CASES])
def test_protate_inputs_excuse_no_query(case):
    ok = K.excusable(case)
    assert ok.sum() <= 0.05 * case.nq
    assert not ok.any()


def test_cases_cover_every_path():
    """Slots per row on both sides of each prefetch depth (128 / 256 / 512), of
    both slot kinds, rows on both sides of the LDS staging threshold, relation
    counts of one and of several chunks, and more queries than 65,535."""
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
        if ((le + 3) & ~3) * 3 + 1028 + 32 > 16384:  # h, t and one slot, the scores and the bitmap
            seen["in_place"] += 1
        else:
            seen[(kind, 0 if n <= 128 else 1 if n <= 256 else 2 if n <= 512 else 3)] += 1
    assert all(v > 0 for v in seen.values()), seen
    assert {1, 2, 7, 61, 64, 65, 130, 1500} <= {c.R for c in K.ALL_CASES}
    assert max(c.nq for c in K.ALL_CASES) > 65535


def test_relation_csr_against_brute_force():
    E, R = 12, 9
    g = np.random.default_rng(4)
    tr = np.stack([g.integers(0, E, 400), g.integers(0, R, 400), g.integers(0, E, 400)], 1).astype(np.int64)
    tr = np.concatenate([tr, [[11, 3, 0]], tr[:25]])  # (11, 0) holds relation 3 only; listed triples repeat
    tr = tr[~((tr[:, 0] == 11) & (tr[:, 2] == 0) & (tr[:, 1] != 3))]
    known = {}
    for h, r, t in tr.tolist():
        known.setdefault((h, t), set()).add(r)
    assert known[(11, 0)] == {3} and max(len(v) for v in known.values()) >= 3
    q = np.concatenate([tr[:60], tr[:10],                      # repeated (h, t) pairs
                        [[11, 3, 0]],                          # a pair with no other relation
                        [[11, 5, 0]],                          # ... queried with another r: relation 3 is listed
                        [[0, 2, 0]] if (0, 0) not in known else [[5, 2, 5]],
                        [[11, -1, 0], [3, -1, 4]]])            # no true relation: every known one
    for index in (FilterIndex(tr, E, R), FilterIndex([tuple(x) for x in tr.tolist()], E, R)):
        before = [index.filter_csr(q[:60], m) for m in ("head-batch", "tail-batch")]
        assert "_rel_index" not in index.__dict__
        for _ in range(2):  # (built lazily, then cached)
            off, ids = index.relation_csr(q)
            assert off.dtype == np.int64 and ids.dtype == np.int64 and off.shape == (len(q) + 1,) and off[0] == 0
            assert off[-1] == len(ids)
            for i, (h, r, t) in enumerate(q.tolist()):
                want = sorted(known.get((h, t), set()) - {r})
                assert ids[off[i]:off[i + 1]].tolist() == want, (i, h, r, t)
    i = 70
    assert q[i].tolist() == [11, 3, 0] and off[i] == off[i + 1]
    assert ids[off[i + 1]:off[i + 2]].tolist() == [3]
    # the existing index is untouched by it
    after = [index.filter_csr(q[:60], m) for m in ("head-batch", "tail-batch")]
    assert all(np.array_equal(a, b) for x, y in zip(before, after) for a, b in zip(x, y))
    off0, ids0 = FilterIndex(np.zeros((0, 3), np.int64), E, R).relation_csr(q[:3])
    assert off0.tolist() == [0, 0, 0, 0] and len(ids0) == 0
