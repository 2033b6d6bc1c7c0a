"""kge_rank_relations on the device against the fp32 reference-order oracle:
ranks, tie counts and every score bit equal the oracle's for TransE, DistMult,
ComplEx and RotatE (RotatE with relation_trig = ops.reference_rotation, the
torch CPU cos / sin the oracle uses), raw and filtered, over the cases of
tests/rank_relations_cases.py — every staging variant of k_rank_rel, relation
counts of one and of many chunks, planted exact and near ties, unaligned
tables, rows read in place, r = -1 rows, and one call of 70,001 queries.

pRotatE: the oracle takes sin as the float64 sin rounded once to fp32 (the
device's sin_rn), and every score bit is held to it like the other models'.
A query's rank may differ from the oracle only if the oracle has
another relation within 4 ulp of the true score, and at most 5 % of a case's
queries may; the inputs are ones where the oracle excuses none
(test_rank_relations_ref.py), so agreement is exact there too.
"""
from argparse import Namespace

import numpy as np
import pytest
import torch

import rank_relations_cases as K
from knowledgegraphembedding_amd import KGEModel, ops
from knowledgegraphembedding_amd.filters import FilterIndex
from test_gpu_parity import DEV, build_model
from test_slot_matrix_gpu import unaligned

pytestmark = pytest.mark.gpu


def make(case):
    ent, rel, mod, _ = K.tables(case)
    m, _, _, mod0, _ = build_model(case.name, case.E, case.R, case.d, K.GAMMA, case.seed)
    assert mod is None or float(mod0[0, 0]) == float(mod[0, 0])
    with torch.no_grad():
        m.entity_embedding.copy_(torch.from_numpy(ent.copy()))
        m.relation_embedding.copy_(torch.from_numpy(rel.copy()))
    if not case.aligned:
        m.entity_embedding.data = unaligned(m.entity_embedding.data)
        m.relation_embedding.data = unaligned(m.relation_embedding.data)
    assert (m.entity_embedding.data_ptr() % 16 == 0) == case.aligned
    assert (m.relation_embedding.data_ptr() % 16 == 0) == case.aligned
    return m


def run(m, case, filtered, scores=False, q=None, trig="model"):
    q = torch.from_numpy((K.queries(case) if q is None else q).copy())
    filt = tuple(torch.from_numpy(x.copy()) for x in K.filt(case)) if filtered else None
    trig = m._rank_rotation(DEV) if trig == "model" else trig
    out = ops.rank_relations(m.desc(), q, DEV, filt=filt, relation_trig=trig, scores=scores)
    return tuple(t.cpu().numpy() for t in out)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def check(case, filtered, ranks, ties, what):
    r_rank, r_ties = K.reference(case, filtered)
    bad = np.nonzero((ranks != r_rank) | (ties != r_ties))[0]
    print(f"{what}: {len(bad)} of {case.nq} queries differ from the oracle")
    if case.name == "pRotatE":
        ok = K.excusable(case)
        assert ok.sum() <= 0.05 * case.nq, what
        bad = bad[~ok[bad]]
    assert not len(bad), (f"{what}: queries {bad[:8]}: ranks {ranks[bad[:8]]} vs {r_rank[bad[:8]]}, "
                          f"ties {ties[bad[:8]]} vs {r_ties[bad[:8]]}")


@pytest.mark.parametrize("case", K.ALL_CASES, ids=[c.id for c in K.ALL_CASES])
def test_vs_oracle(case):
    m = make(case)
    for filtered in (False, True):
        ranks, ties, s = run(m, case, filtered, scores=True)
        assert ranks.dtype == np.int64 and ties.dtype == np.int32 and ranks.shape == ties.shape == (case.nq,)
        assert s.dtype == np.float32 and s.shape == (case.nq, case.R)
        check(case, filtered, ranks, ties, f"{case.id} filtered={filtered}")
        differ = bits(s) != bits(K.scores(case))
        print(f"{case.id}: {int(differ.sum())} of {s.size} scores differ in a bit")
        # every model, pRotatE too: the oracle's sin is the float64 sin rounded once,
        # the device's sin_rn, so the operation order shows in the bits
        assert not differ.any(), np.argwhere(differ)[:8]
        # the same counts without the scores buffer
        r2, t2 = run(m, case, filtered)
        assert np.array_equal(r2, ranks) and np.array_equal(t2, ties)
    ops.raise_on_device_error(DEV)


def test_model_methods_raw_and_filtered():
    """KGEModel.rank_relations: raw without all_true_triples, filtered with —
    the lists FilterIndex.relation_csr builds from the true triples."""
    case = K.PLANTED[1]
    m = make(case)
    q = K.queries(case)
    ranks, ties = m.rank_relations(q)
    assert ranks.dtype == np.int64 and ties.dtype == np.int32
    assert np.array_equal(ranks, K.reference(case, False)[0]) and np.array_equal(ties, K.reference(case, False)[1])
    # true triples: every query's own, plus (h, r', t) for its in-range listed ids
    excl = K.excluded(case)
    qi, rid = np.nonzero(excl)
    true = np.concatenate([q, np.stack([q[qi, 0], rid, q[qi, 2]], 1)])
    want = K.count(K.scores(case), q[:, 1], _known(true, q, case.R))
    for all_true in ([tuple(x) for x in true.tolist()], FilterIndex(true, case.E, case.R)):
        ranks, ties = m.rank_relations([tuple(x) for x in q.tolist()], all_true)
        assert np.array_equal(ranks, want[0]) and np.array_equal(ties, want[1])


def _known(true, q, R):
    """[nq, R] bool: (h, r', t) is a listed true triple (brute force)."""
    known = set(map(tuple, np.asarray(true).tolist()))
    return np.array([[(h, r, t) in known for r in range(R)] for h, _, t in np.asarray(q).tolist()], dtype=bool)


@pytest.mark.parametrize("case", (K.COUNTS[7], K.PLANTED[3]), ids=lambda c: c.id)
def test_deterministic_and_geometry_independent(case, monkeypatch):
    m = make(case)
    a = run(m, case, True, scores=True)
    b = run(m, case, True, scores=True)
    assert all(np.array_equal(x, y) for x, y in zip(a[:2], b[:2])) and np.array_equal(bits(a[2]), bits(b[2]))
    for chunk in ("1", "7", "64"):  # relations per chunk (a diagnostic switch): other grids, the same counts
        monkeypatch.setenv("KGE_RANK_REL_CHUNK", chunk)
        g = run(m, case, True, scores=True)
        assert np.array_equal(a[0], g[0]) and np.array_equal(a[1], g[1]), chunk
        assert np.array_equal(bits(a[2]), bits(g[2])), chunk
    ops.raise_on_device_error(DEV)


def test_rotate_device_trig():
    """relation_trig = None: correctly rounded cos / sin from the workspace table."""
    for case in (K.BASE[3], K.UNALIGNED[1], K.WIDTHS[6]):
        m = make(case)
        ranks, ties, s = run(m, case, False, scores=True, trig=None)
        ref = K.scores(case)
        err = np.abs(s.astype(np.float64) - ref)
        print(f"{case.id}: max |Δ| {err.max():.3e}, {(bits(s) != bits(ref)).sum()} of {s.size} scores differ in a bit")
        assert np.all(err <= 1e-4 * np.maximum(np.abs(ref), 1.0))
        # its own scores' counts
        want = K.count(s, K.queries(case)[:, 1])
        assert np.array_equal(ranks, want[0]) and np.array_equal(ties, want[1])
    ops.raise_on_device_error(DEV)


@pytest.mark.parametrize("col,bad", [(0, 10 ** 6), (0, -1), (1, 61), (1, -2), (2, 301), (2, -1)])
def test_query_out_of_range(col, bad):
    case = K.BASE[0]
    m = make(case)
    q = K.queries(case).copy()
    q[5, col] = bad
    with pytest.raises(IndexError):
        m.rank_relations(q)
    ranks, ties, s = run(m, case, True, scores=True, q=q)
    with pytest.raises(IndexError):
        ops.raise_on_device_error(DEV)
    r_rank, r_ties = (x.copy() for x in K.reference(case, True))
    r_rank[5], r_ties[5] = 0, 0
    assert np.array_equal(ranks, r_rank) and np.array_equal(ties, r_ties)
    assert np.isnan(s[5]).all()
    keep = np.arange(case.nq) != 5
    assert np.array_equal(bits(s[keep]), bits(K.scores(case)[keep]))
    ops.raise_on_device_error(DEV)  # (cleared)


@pytest.mark.parametrize("case", K.PRED, ids=lambda c: c.id)
def test_no_true_relation(case):
    m = make(case)
    for filtered in (False, True):
        ranks, ties, s = run(m, case, filtered, scores=True)
        assert (ranks[[2, 5]] == 0).all() and (ties[[2, 5]] == 0).all()
        assert np.array_equal(bits(s), bits(K.scores(case)))
        check(case, filtered, ranks, ties, case.id)
    ops.raise_on_device_error(DEV)  # no error raised


def test_bad_shapes():
    case = K.BASE[1]
    m = make(case)
    q = torch.from_numpy(K.queries(case).copy())
    with pytest.raises(ValueError):
        ops.rank_relations(m.desc(), q[:, :2], DEV)
    off, ids = (torch.from_numpy(x.copy()) for x in K.filt(case))
    with pytest.raises(ValueError):
        ops.rank_relations(m.desc(), q, DEV, filt=(off[:-1], ids))
    r = make(K.BASE[3])
    with pytest.raises(ValueError):
        ops.rank_relations(r.desc(), q, DEV, relation_trig=torch.zeros(61, 2, 19, device=DEV))


# ------------------------------------------------------ predict_relations
@pytest.mark.parametrize("case", (K.PLANTED[1], K.BASE[3], K.COUNTS[2]), ids=lambda c: c.id)
def test_predict_relations(case, monkeypatch):
    m = make(case)
    q = K.queries(case)
    s = K.scores(case)
    R = case.R
    for k in (1, min(10, R), R):
        ids, sc = m.predict_relations(q[:, (0, 2)], k=k)
        w_ids, w_sc = K.topk_reference(s, k)
        assert ids.dtype == np.int64 and sc.dtype == np.float32 and ids.shape == sc.shape == (case.nq, k)
        assert np.array_equal(ids, w_ids) and np.array_equal(bits(sc), bits(w_sc)), k
    # [nq, 3] rows: r is not read
    ids3, _ = m.predict_relations(q, k=1)
    assert np.array_equal(ids3, K.topk_reference(s, 1)[0])
    # filtered: the known relations of (h, t) are excluded; padding where fewer than k remain
    excl = K.excluded(case).copy()
    excl[3, 0], excl[3, 1:] = False, True  # query 3 keeps relation 0 alone
    qi, rid = np.nonzero(excl)
    true = np.stack([q[qi, 0], rid, q[qi, 2]], 1)
    known = _known(true, q, R)
    monkeypatch.setattr(KGEModel, "REL_SCORE_BYTES", 4 * R * 7)  # several launches of 7 queries
    for k in (1, R):
        ids, sc = m.predict_relations(q[:, (0, 2)], k=k, all_true_triples=[tuple(x) for x in true.tolist()])
        w_ids, w_sc = K.topk_reference(s, k, known)
        assert np.array_equal(ids, w_ids) and np.array_equal(bits(sc), bits(w_sc)), k
    if R > 1:
        assert (ids[3, 1:] == -1).all() and np.isneginf(sc[3, 1:]).all() and ids[3, 0] >= 0
    for k in (0, R + 1):
        with pytest.raises(ValueError):
            m.predict_relations(q[:, (0, 2)], k=k)
    ops.raise_on_device_error(DEV)


# ------------------------------------------------- test_step, KGE_EVAL_RELATIONS
def test_test_step_relation_metrics(monkeypatch):
    E, R = 120, 9
    m, ent, rel, mod, erange = build_model("DistMult", E, R, 24, K.GAMMA, 17)
    g = np.random.default_rng(8)
    true = np.unique(np.stack([g.integers(0, 30, 2000), g.integers(0, R, 2000), g.integers(0, 30, 2000)],
                              1).astype(np.int64), axis=0)
    test = true[g.permutation(len(true))[:100]]
    args = Namespace(countries=False, nentity=E, nrelation=R, test_batch_size=16, cpu_num=2, test_log_steps=10 ** 9,
                     cuda=True)
    test_l, true_l = [tuple(x) for x in test.tolist()], [tuple(x) for x in true.tolist()]
    monkeypatch.delenv("KGE_EVAL_RELATIONS", raising=False)
    monkeypatch.delenv("KGE_EVAL_CANDIDATES", raising=False)
    plain = KGEModel.test_step(m, test_l, true_l, args)
    assert list(plain) == ["MRR", "MR", "HITS@1", "HITS@3", "HITS@10"]
    monkeypatch.setenv("KGE_EVAL_RELATIONS", "0")
    assert KGEModel.test_step(m, test_l, true_l, args) == plain
    monkeypatch.setenv("KGE_EVAL_RELATIONS", "1")
    got = KGEModel.test_step(m, test_l, true_l, args)
    assert list(got) == list(plain) + ["REL_MRR", "REL_MR", "REL_HITS@1", "REL_HITS@3", "REL_HITS@10"]
    assert {k: got[k] for k in plain} == plain
    # the oracle's filtered relation ranks of the same triples
    from oracle import kge_oracle as O
    s = O.ref_order_scores("DistMult", ent, rel, mod, torch.from_numpy(K.all_relation_triples(test, R)), "single",
                           K.GAMMA, erange)
    s = np.asarray(s, dtype=np.float32).reshape(len(test), R)
    ranks, _ = K.count(s, test[:, 1], _known(true, test, R))
    assert len(set(ranks.tolist())) > 2 and (_known(true, test, R).sum(1) > 1).any()
    ranks = ranks.tolist()
    want = {"REL_MRR": sum(1.0 / r for r in ranks) / len(ranks), "REL_MR": sum(float(r) for r in ranks) / len(ranks)}
    for k in (1, 3, 10):
        want["REL_HITS@%d" % k] = sum(1.0 if r <= k else 0.0 for r in ranks) / len(ranks)
    assert {k: got[k] for k in want} == want
    monkeypatch.delenv("KGE_EVAL_RELATIONS")
    assert KGEModel.test_step(m, test_l, true_l, args) == plain
