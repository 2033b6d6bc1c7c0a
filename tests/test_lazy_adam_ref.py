"""Lazy entity Adam without a GPU: the rule's plain-torch restatement
(lazy_adam_cases.lazy_adam_ref, the GPU tests' independent reference) on
hand-made gradients, KGELazyAdam's state-dict compatibility with KGEAdam, the
configurations KGEModel refuses for it, and run.py's choice of the class."""
import math
from argparse import Namespace

import pytest
import torch

import lazy_adam_cases as L
from knowledgegraphembedding_amd import KGEAdam, KGELazyAdam, KGEModel, run
from oracle.kge_oracle import adam_steps

LR = L.LR


def _table(rows=6, width=5, seed=3):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(rows, width, generator=g) - 0.5
    grads = [torch.randn(rows, width, generator=g) * 0.1 for _ in range(3)]
    return p, grads


def test_untouched_row_keeps_param_and_moments():
    p, grads = _table()
    all_rows = torch.arange(6)
    skip2 = torch.tensor([0, 1, 3, 4, 5])  # row 2 is touched at steps 1 and 3 only
    p1, m1, v1 = L.lazy_adam_ref(p, grads[:1], [all_rows])
    p2, m2, v2 = L.lazy_adam_ref(p, grads[:2], [all_rows, skip2])
    for a, b in ((p1, p2), (m1, m2), (v1, v2)):
        assert L.same_bits(a[2], b[2])
    assert not L.same_bits(p1[0], p2[0]) and not L.same_bits(m1[0], m2[0])


def test_returning_row_uses_the_global_step():
    p, grads = _table()
    all_rows = torch.arange(6)
    skip2 = torch.tensor([0, 1, 3, 4, 5])
    p2, m2, v2 = L.lazy_adam_ref(p, grads[:2], [all_rows, skip2])
    p3, m3, v3 = L.lazy_adam_ref(p, grads, [all_rows, skip2, all_rows])
    # row 2 at step 3, by hand in double: its moments are step 1's, the bias corrections t = 3's
    b1, b2 = L.BETAS
    g = grads[2][2].double()
    m = m2[2].double() + (1 - b1) * (g - m2[2].double())
    v = v2[2].double() * b2 + (1 - b2) * g * g
    want = p2[2].double() - (LR / (1 - b1 ** 3)) * (m / (v.sqrt() / math.sqrt(1 - b2 ** 3) + L.EPS))
    torch.testing.assert_close(p3[2].double(), want, rtol=2e-6, atol=1e-7)
    # a per-row count (t = 2 for this row) would give another step: the two differ by far more than the tolerance
    per_row = p2[2].double() - (LR / (1 - b1 ** 2)) * (m / (v.sqrt() / math.sqrt(1 - b2 ** 2) + L.EPS))
    assert (per_row - want).abs().max() > 100 * (2e-6 * want.abs().max() + 1e-7)


def test_touched_row_with_zero_gradient_decays_its_moments():
    p, grads = _table()
    grads[1][4] = 0.0
    all_rows = torch.arange(6)
    _, m1, v1 = L.lazy_adam_ref(p, grads[:1], [all_rows])
    p1 = L.lazy_adam_ref(p, grads[:1], [all_rows])[0]
    p2, m2, v2 = L.lazy_adam_ref(p, grads[:2], [all_rows, all_rows])
    torch.testing.assert_close(m2[4], m1[4] * L.BETAS[0], rtol=2e-6, atol=1e-7)
    torch.testing.assert_close(v2[4], v1[4] * L.BETAS[1], rtol=2e-6, atol=1e-7)
    assert (m2[4].abs() < m1[4].abs()).all() and (v2[4] < v1[4]).all()
    assert not L.same_bits(p1[4], p2[4])  # ... and the row still moves by them


def test_all_rows_touched_equals_torch_adam():
    p, grads = _table(rows=9, width=7, seed=4)
    all_rows = torch.arange(9)
    got = L.lazy_adam_ref(p, grads, [all_rows] * 3)
    (ref_p,), ((ref_m, ref_v),) = adam_steps([p], [[g] for g in grads], LR)
    for a, b in zip(got, (ref_p, ref_m, ref_v)):
        torch.testing.assert_close(a, b, rtol=2e-6, atol=1e-7)


def test_touched_ids_drops_out_of_range():
    pos = torch.tensor([[3, 0, 9], [3, 1, -1]])
    neg = torch.tensor([[5, 10], [0, 5]])
    assert L.touched_ids(pos, neg, 10).tolist() == [0, 3, 5, 9]


# ------------------------------------------------------------- optimizer
def _stepped(cls):
    torch.manual_seed(1)
    ps = [torch.nn.Parameter(torch.rand(4, 3)), torch.nn.Parameter(torch.rand(2, 3))]
    opt = cls(ps, lr=2e-3, betas=(0.8, 0.95), eps=1e-6)
    for p in ps:  # two steps' worth of state without a device
        for _ in range(2):
            st, _ = opt._advance(p, opt.param_groups[0])
        st["exp_avg"].copy_(torch.rand(p.shape))
        st["exp_avg_sq"].copy_(torch.rand(p.shape))
    return ps, opt


@pytest.mark.parametrize("src,dst", [(KGEAdam, KGELazyAdam), (KGELazyAdam, KGEAdam)])
def test_state_dict_round_trip(src, dst):
    _, a = _stepped(src)
    sd = a.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    ps = [torch.nn.Parameter(torch.zeros(4, 3)), torch.nn.Parameter(torch.zeros(2, 3))]
    b = dst(ps, lr=1.0)
    b.load_state_dict(sd)
    sd2 = b.state_dict()
    assert sd2["param_groups"] == sd["param_groups"]
    assert sd2["state"].keys() == sd["state"].keys()
    for k in sd["state"]:
        for f in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(sd2["state"][k][f], sd["state"][k][f])
    # and on into the reference's optimizer, whose layout both share
    t = torch.optim.Adam([torch.nn.Parameter(torch.zeros(4, 3)), torch.nn.Parameter(torch.zeros(2, 3))], lr=1.0)
    t.load_state_dict(sd2)
    assert t.state_dict()["param_groups"][0]["lr"] == 2e-3


def test_lazy_adam_is_a_kgeadam_with_the_same_configuration():
    assert issubclass(KGELazyAdam, KGEAdam) and KGELazyAdam.lazy_entity and not KGEAdam.lazy_entity
    p = torch.nn.Parameter(torch.zeros(2, 2))
    assert KGELazyAdam([p]).defaults == KGEAdam([p]).defaults
    with pytest.raises(ValueError):
        KGELazyAdam([p], weight_decay=0.1)


# ------------------------------------------------------------ KGEModel
class _NoBatch:
    def __next__(self):
        raise AssertionError("a batch was drawn: the refusal must come first")


def _lazy_setup(**args):
    torch.manual_seed(0)
    m = KGEModel("TransE", 12, 3, 8, 12.0)
    opt = KGELazyAdam([m.entity_embedding, m.relation_embedding], lr=1e-3)
    a = dict(negative_adversarial_sampling=True, adversarial_temperature=1.0, uni_weight=False, regularization=0.0,
             dp_group=None)
    a.update(args)
    return m, opt, Namespace(**a)


@pytest.mark.parametrize("what,match", [("partition", "row partition"), ("dp", "data-parallel"),
                                        ("unfused", "fuse_optimizer"), ("reg", "regulariser")])
def test_train_step_refuses_before_any_launch(what, match):
    m, opt, args = _lazy_setup(**(dict(regularization=1e-3) if what == "reg" else
                                  dict(dp_group=object()) if what == "dp" else {}))
    if what == "partition":
        m.row_partition = object()
    if what == "unfused":
        m.fuse_optimizer = False
    with pytest.raises(ValueError, match=match):
        KGEModel.train_step(m, opt, _NoBatch(), args)
    # the same from compute_train_grads, before the tables' device is even looked at (they are on the CPU here)
    pos, neg, w = torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 4, dtype=torch.int64), torch.ones(2)
    with pytest.raises(ValueError, match=match):
        m.compute_train_grads(pos, neg, w, "tail-batch", args, optimizer=opt)
    assert m.entity_embedding.grad is None and len(opt.state) == 0


def test_dense_optimizer_is_not_refused_by_the_lazy_checks():
    m, _, args = _lazy_setup(regularization=1e-3)
    assert m._check_lazy(KGEAdam([m.entity_embedding], lr=1e-3), args) is False
    assert m._check_lazy(None, args) is False


# -------------------------------------------------------------- run.py
def test_run_picks_the_class_from_the_environment(monkeypatch):
    monkeypatch.delenv("KGE_ENTITY_ADAM", raising=False)
    assert run.adam_class() is KGEAdam
    monkeypatch.setenv("KGE_ENTITY_ADAM", "dense")
    assert run.adam_class() is KGEAdam
    monkeypatch.setenv("KGE_ENTITY_ADAM", "lazy")
    assert run.adam_class() is KGELazyAdam
    for bad in ("Lazy", "sparse", ""):
        monkeypatch.setenv("KGE_ENTITY_ADAM", bad)
        with pytest.raises(ValueError, match="KGE_ENTITY_ADAM"):
            run.adam_class()

