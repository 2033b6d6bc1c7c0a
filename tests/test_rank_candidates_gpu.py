"""kge_rank_candidates on the device against the fp32 reference-order oracle:
ranks and tie counts equal the oracle's exactly for TransE, DistMult, ComplEx
and RotatE (RotatE with relation_trig = ops.reference_rotation, the torch CPU
cos / sin the oracle uses), over the cases of tests/rank_candidates_cases.py —
every staging variant of k_rank_cand, lists of one and of many chunks, -1
padding, planted exact and near ties, an unaligned table, rows read in place,
and one call of 70,001 queries.

pRotatE: the oracle takes sin as the float64 sin rounded once to fp32 (the
device's sin_rn).  A query may differ from the oracle only if the oracle has a
candidate, other than a copy of the true id, within 4 ulp of the true score,
and at most 5 % of the queries may; the inputs are ones where the oracle
excuses none (test_rank_candidates_ref.py), so agreement is exact there too.
"""
from argparse import Namespace

import numpy as np
import pytest
import torch

import rank_candidates_cases as K
from knowledgegraphembedding_amd import KGEModel, ops
from test_gpu_parity import DEV, build_model
from test_slot_matrix_gpu import unaligned

pytestmark = pytest.mark.gpu


def make(case):
    ent, rel, mod, _ = K.tables(case)
    m, _, _, mod0, _ = build_model(case.name, case.E, K.R, case.d, K.GAMMA, case.seed)
    assert mod is None or float(mod0[0, 0]) == float(mod[0, 0])
    with torch.no_grad():
        m.entity_embedding.copy_(torch.from_numpy(ent.copy()))
        m.relation_embedding.copy_(torch.from_numpy(rel.copy()))
    if not case.aligned:
        m.entity_embedding.data = unaligned(m.entity_embedding.data)
    assert (m.entity_embedding.data_ptr() % 16 == 0) == case.aligned
    return m


def check(case, mode, ranks, ties, what):
    r_rank, r_ties = K.reference(case, mode)
    bad = np.nonzero((ranks != r_rank) | (ties != r_ties))[0]
    print(f"{what}: {len(bad)} of {case.nq} queries differ from the oracle")
    if case.name == "pRotatE":
        ok = K.excusable(case, mode)
        assert ok.sum() <= 0.05 * case.nq, what
        bad = bad[~ok[bad]]
    assert not len(bad), (f"{what}: queries {bad[:8]}: ranks {ranks[bad[:8]]} vs {r_rank[bad[:8]]}, "
                          f"ties {ties[bad[:8]]} vs {r_ties[bad[:8]]}")


@pytest.mark.parametrize("case", K.ALL_CASES, ids=[c.id for c in K.ALL_CASES])
def test_vs_oracle(case):
    m = make(case)
    for mode in K.MODES:
        ranks, ties = m.rank_candidates(K.queries(case), K.cand(case, mode), mode)
        assert ranks.dtype == np.int64 and ties.dtype == np.int32 and ranks.shape == ties.shape == (case.nq,)
        check(case, mode, ranks, ties, f"{case.id} {mode}")


@pytest.mark.parametrize("case", (K.LENGTHS[5], K.BASE[3]), ids=lambda c: c.id)
def test_deterministic_and_geometry_independent(case, monkeypatch):
    m = make(case)
    mode = "tail-batch"
    trig = m._rank_rotation(DEV)
    q, c = torch.from_numpy(K.queries(case).copy()).to(DEV), torch.from_numpy(K.cand(case, mode).copy()).to(DEV)
    a = ops.rank_candidates(m.desc(), mode, q, c, DEV, relation_trig=trig)
    b = ops.rank_candidates(m.desc(), mode, q, c, DEV, relation_trig=trig)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for chunk in ("7", "64", "1000"):  # candidates per chunk (a diagnostic switch): other grids, the same counts
        monkeypatch.setenv("KGE_RANK_CAND_CHUNK", chunk)
        g = ops.rank_candidates(m.desc(), mode, q, c, DEV, relation_trig=trig)
        assert torch.equal(a[0], g[0]) and torch.equal(a[1], g[1]), chunk
    ops.raise_on_device_error(DEV)


def test_candidate_out_of_range():
    case, mode = K.BASE[1], "head-batch"
    m = make(case)
    c = K.cand(case, mode).copy()
    c[3, 11] = case.E        # skipped; the rest of query 3 proceeds
    c[7, 0] = case.E + 12345
    with pytest.raises(IndexError):
        m.rank_candidates(K.queries(case), c, mode)
    ranks, ties = ops.rank_candidates(m.desc(), mode, torch.from_numpy(K.queries(case).copy()), torch.from_numpy(c), DEV)
    ranks, ties = ranks.cpu().numpy(), ties.cpu().numpy()
    with pytest.raises(IndexError):
        ops.raise_on_device_error(DEV)
    want = K.count(K.scores(case, mode), (c >= 0) & (c < case.E))
    assert np.array_equal(ranks, want[0]) and np.array_equal(ties, want[1])
    ops.raise_on_device_error(DEV)  # (cleared)


@pytest.mark.parametrize("col,bad", [(0, 10 ** 6), (0, -1), (1, K.R), (2, 301)])
def test_query_out_of_range(col, bad):
    case, mode = K.BASE[0], "tail-batch"
    m = make(case)
    q = K.queries(case).copy()
    q[5, col] = bad
    with pytest.raises(IndexError):
        m.rank_candidates(q, K.cand(case, mode), mode)
    ranks, ties = ops.rank_candidates(m.desc(), mode, torch.from_numpy(q), torch.from_numpy(K.cand(case, mode).copy()),
                                      DEV)
    ranks, ties = ranks.cpu().numpy(), ties.cpu().numpy()
    with pytest.raises(IndexError):
        ops.raise_on_device_error(DEV)
    r_rank, r_ties = (x.copy() for x in K.reference(case, mode))
    r_rank[5], r_ties[5] = 0, 0
    assert np.array_equal(ranks, r_rank) and np.array_equal(ties, r_ties)


def test_bad_shapes():
    case = K.BASE[1]
    m = make(case)
    q = torch.from_numpy(K.queries(case).copy())
    for c in (torch.zeros(case.nq, 0, dtype=torch.int64), torch.zeros(case.nq, dtype=torch.int64),
              torch.zeros(case.nq + 1, 4, dtype=torch.int64)):
        with pytest.raises(ValueError):
            ops.rank_candidates(m.desc(), "tail-batch", q, c, DEV)
    with pytest.raises(ValueError):
        ops.rank_candidates(m.desc(), "single", q, torch.zeros(case.nq, 4, dtype=torch.int64), DEV)
    r = make(K.BASE[3])
    with pytest.raises(ValueError):
        ops.rank_candidates(r.desc(), "tail-batch", q, torch.zeros(case.nq, 4, dtype=torch.int64), DEV,
                            relation_trig=torch.zeros(K.R, 2, 19, device=DEV))


# ------------------------------------------------- sampled evaluation
E_EVAL, R_EVAL, N_EVAL = 400, 9, 50


def _eval_setup():
    m, *_ = build_model("RotatE", E_EVAL, R_EVAL, 24, K.GAMMA, 17)
    g = np.random.default_rng(8)
    true = np.unique(np.stack([g.integers(0, E_EVAL, 3000), g.integers(0, R_EVAL, 3000), g.integers(0, E_EVAL, 3000)],
                              1).astype(np.int64), axis=0)
    test = true[g.permutation(len(true))[:150]]
    args = Namespace(countries=False, nentity=E_EVAL, nrelation=R_EVAL, test_batch_size=16, cpu_num=2,
                     test_log_steps=10 ** 9, cuda=True)
    return m, [tuple(x) for x in test.tolist()], [tuple(x) for x in true.tolist()], args, test, true


def test_sampled_test_step(monkeypatch):
    m, test_l, true_l, args, test, true = _eval_setup()
    monkeypatch.delenv("KGE_EVAL_CANDIDATES", raising=False)
    monkeypatch.delenv("KGE_EVAL_SEED", raising=False)
    full = KGEModel.test_step(m, test_l, true_l, args)
    monkeypatch.setenv("KGE_EVAL_CANDIDATES", "0")
    assert KGEModel.test_step(m, test_l, true_l, args) == full  # 0: the untouched path
    monkeypatch.setenv("KGE_EVAL_CANDIDATES", str(N_EVAL))
    a = KGEModel.test_step(m, test_l, true_l, args)
    b = KGEModel.test_step(m, test_l, true_l, args)
    assert a == b and set(a) == {"MRR", "MR", "HITS@1", "HITS@3", "HITS@10"}
    assert a != full and a["MR"] <= N_EVAL + 1
    # by hand, from KGEModel.rank_candidates on the same drawn candidates
    true_heads, true_tails = {}, {}
    for h, r, t in true_l:
        true_heads.setdefault((r, t), set()).add(h)
        true_tails.setdefault((h, r), set()).add(t)
    ranks, blocks = [], 0
    for mode, q, cand in m.sampled_eval_blocks(test_l, true_l, N_EVAL):
        c = cand.cpu().numpy()
        assert c.shape == (len(q), N_EVAL) and c.min() >= 0 and c.max() < E_EVAL
        for (h, r, t), row in zip(q.tolist(), c):
            known = true_heads[(r, t)] if mode == "head-batch" else true_tails[(h, r)]
            assert not known.intersection(row.tolist())  # no drawn candidate is a known true answer
        ranks.extend(m.rank_candidates(q, cand, mode)[0].tolist())
        blocks += 1
    assert blocks == 2 and len(ranks) == 2 * len(test_l)
    want = {"MRR": sum(1.0 / r for r in ranks) / len(ranks), "MR": sum(float(r) for r in ranks) / len(ranks)}
    for k in (1, 3, 10):
        want["HITS@%d" % k] = sum(1.0 if r <= k else 0.0 for r in ranks) / len(ranks)
    assert a == want
    # the key comes from KGE_EVAL_SEED (else 0): another seed draws other candidates
    mode, q, cand = next(iter(m.sampled_eval_blocks(test_l, true_l, N_EVAL)))
    assert mode == "head-batch"
    monkeypatch.setenv("KGE_EVAL_SEED", "5")
    _, _, cand5 = next(iter(m.sampled_eval_blocks(test_l, true_l, N_EVAL)))
    assert not torch.equal(cand, cand5)
    _, _, cand5b = next(iter(m.sampled_eval_blocks(test_l, true_l, N_EVAL, seed=5)))
    assert torch.equal(cand5, cand5b)
    monkeypatch.delenv("KGE_EVAL_SEED")
    # variable unset again: the untouched path's result
    monkeypatch.delenv("KGE_EVAL_CANDIDATES")
    assert KGEModel.test_step(m, test_l, true_l, args) == full


def test_sampled_test_step_refuses_too_many(monkeypatch):
    m, test_l, true_l, args, _, _ = _eval_setup()
    monkeypatch.setenv("KGE_EVAL_CANDIDATES", str(E_EVAL))
    with pytest.raises(ValueError):
        KGEModel.test_step(m, test_l, true_l, args)


def test_sampled_test_step_sampler_error(monkeypatch):
    """A query whose known answers leave no entity to draw raises as in training."""
    E = 40
    m, *_ = build_model("TransE", E, 2, 8, K.GAMMA, 3)
    true_l = [(h, 0, 1) for h in range(E)] + [(1, 1, 2)]  # every head is a true head of (0, 1)
    args = Namespace(countries=False, nentity=E, nrelation=2, test_batch_size=4, cpu_num=2, test_log_steps=10 ** 9,
                     cuda=True)
    monkeypatch.setenv("KGE_EVAL_CANDIDATES", "5")
    with pytest.raises(RuntimeError, match="negative sampler"):
        KGEModel.test_step(m, [(0, 0, 1)], true_l, args)
