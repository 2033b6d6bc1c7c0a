"""The Adagrad rules' numpy restatement (tests/adagrad_cases.py) against
torch.optim.Adagrad on the CPU, one step from equal state, within the derived
bounds; zero-gradient rows; the row-wise rule against double precision; the
optimizer's and run.py's host-side behaviour.  No GPU."""
import numpy as np
import pytest
import torch

import adagrad_cases as A

f32 = np.float32


def _inputs(seed, shape, gscale, sscale):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(shape).astype(f32)
    g = (rng.standard_normal(shape) * gscale).astype(f32)
    s = (rng.random(shape) * sscale).astype(f32)
    return p, g, s


@pytest.mark.parametrize("lr,gscale,sscale", [(3e-2, 1.0, 0.0), (1e-2, 1e-3, 1e-6), (1.0, 30.0, 1e3), (1e-4, 1e-6, 1e-2)])
def test_elementwise_rule_against_torch_adagrad(lr, gscale, sscale):
    p, g, s = _inputs(1, (257, 63), gscale, sscale)
    g[5] = 0.0  # (a zero-gradient row among them)
    p1, s1 = A.adagrad_elem_ref(p, g, s, lr=lr)
    tp, ts = A.torch_adagrad_step(p, g, s, lr=lr)
    s64 = s.astype(np.float64) + g.astype(np.float64) ** 2
    std = np.sqrt(s64) + float(f32(A.EPS))
    dp, ds = np.abs(p1.astype(np.float64) - tp), np.abs(s1.astype(np.float64) - ts)
    bp, bs = A.p_bound(tp.astype(np.float64), g.astype(np.float64), std, lr), A.sum_bound(s64)
    print("max |dp| / bound", float((dp / np.maximum(bp, 1e-300)).max()), "max |dsum| / bound",
          float((ds / np.maximum(bs, 1e-300)).max()))
    assert (dp <= bp).all() and (ds <= bs).all()
    assert p1.dtype == f32 and s1.dtype == f32


def test_zero_gradient_rows_keep_their_bits():
    """s + 0·0 = s and p + (-lr)·(0 / std) = p for every finite p, s >= 0 and eps > 0: -0.0, denormals, s = 0."""
    p = np.array([[0.0, -0.0, 1e-40, -3.5, 1e30, 7.0]], dtype=f32).repeat(3, 0)
    s = np.array([[0.0], [1e-30], [4.0]], dtype=f32).repeat(p.shape[1], 1)
    g = np.zeros_like(p)
    p1, s1 = A.adagrad_elem_ref(p, g, s)
    assert np.array_equal(p1.view(np.int32), p.view(np.int32)) and np.array_equal(s1.view(np.int32), s.view(np.int32))
    q1, G1 = A.adagrad_row_ref(p, g, s[:, 0])
    assert np.array_equal(q1.view(np.int32), p.view(np.int32)) and np.array_equal(G1.view(np.int32), s[:, 0].view(np.int32))


@pytest.mark.parametrize("Le", [63, 64, 2000])
def test_rowwise_rule_against_double(Le):
    p, g, _ = _inputs(2, (40, Le), 0.3, 0.0)
    G = np.random.default_rng(3).random(40).astype(f32) * f32(0.05)
    G[:4] = 0.0
    p1, G1 = A.adagrad_row_ref(p, g, G)
    p64, G64 = A.adagrad_row_f64(p, g, G)
    assert (np.abs(G1 - G64) <= A.rowsum_bound(G64, Le)).all()
    # p': the element-wise bound plus the state's error carried through the square root:
    # d(std)/std <= d(G')/(2 G'), i.e. (Le + 4) 2^-25 relative on the move
    std = np.sqrt(G64) + float(f32(A.EPS))
    move = float(f32(A.LR)) * np.abs(g) / std[:, None]
    bound = A.p_bound(p64, g.astype(np.float64), std[:, None]) + (Le + 4) * 2.0 ** -25 * move
    assert (np.abs(p1 - p64) <= bound).all()
    # given the state, the move is the element-wise rule's: same bits
    assert np.array_equal(A.adagrad_move_ref(p, g, G1), p1)


# ------------------------------------------------------------ the optimizer
def _params():
    torch.manual_seed(0)
    return [torch.nn.Parameter(torch.randn(6, 8)), torch.nn.Parameter(torch.randn(3, 8))]


def test_optimizer_refuses_other_configurations():
    from knowledgegraphembedding_amd import KGEAdagrad
    for kw in (dict(lr_decay=0.1), dict(weight_decay=0.1), dict(initial_accumulator_value=0.1), dict(eps=0.0),
               dict(eps=float("nan")), dict(lr=-1.0), dict(lr=float("inf"))):
        with pytest.raises(ValueError):
            KGEAdagrad(_params(), **kw)
    opt = KGEAdagrad(_params())
    assert opt.lazy_entity and opt.defaults["lr"] == 1e-2 and opt.defaults["eps"] == 1e-10


def test_prepare_fused_builds_the_descriptor_and_the_state():
    from knowledgegraphembedding_amd import KGEAdagrad, _lib
    for rowwise in (False, True):
        ent, rel = _params()
        opt = KGEAdagrad([ent, rel], lr=0.5, eps=1e-6, rowwise_entity=rowwise)
        d = opt.prepare_fused(ent, rel, None, write_grad=False)
        assert isinstance(d, _lib.AdagradDesc) and d.struct_size == __import__("ctypes").sizeof(_lib.AdagradDesc)
        assert (d.lr, d.eps, d.entity_rowwise, d.write_grad) == (0.5, f32(1e-6), int(rowwise), 0)
        assert set(opt.state[ent]) == {"step", "sum"} and float(opt.state[ent]["step"]) == 1.0
        assert tuple(opt.state[ent]["sum"].shape) == ((6,) if rowwise else (6, 8))
        assert tuple(opt.state[rel]["sum"].shape) == (3, 8)
        assert d.entity.param == ent.data_ptr() and d.entity.state_sum == opt.state[ent]["sum"].data_ptr()
        assert d.relation.state_sum == opt.state[rel]["sum"].data_ptr() and not d.modulus.param
        opt.step()  # (both tables were fused: nothing to do, no library call)
        if rowwise:  # a dense gradient of the row-wise table has no rule
            ent.grad = torch.zeros_like(ent)
            with pytest.raises(ValueError, match="row-wise"):
                opt.step()
    other = torch.nn.Parameter(torch.randn(2, 2))
    assert KGEAdagrad(_params()).prepare_fused(other, other) is None  # not this optimizer's tensors


def test_state_dict_round_trips_with_torch_adagrad():
    from knowledgegraphembedding_amd import KGEAdagrad
    ent, rel = _params()
    ours = KGEAdagrad([ent, rel], lr=0.5, eps=1e-6)
    ours.prepare_fused(ent, rel)
    ours.state[ent]["sum"].add_(2.0)
    theirs = torch.optim.Adagrad(_params(), lr=0.1)
    theirs.load_state_dict(ours.state_dict())
    st = theirs.state[theirs.param_groups[0]["params"][0]]
    assert torch.equal(st["sum"], ours.state[ent]["sum"]) and float(st["step"]) == 1.0
    assert theirs.param_groups[0]["lr"] == 0.5 and theirs.param_groups[0]["eps"] == 1e-6
    p = theirs.param_groups[0]["params"][0]
    p.grad = torch.ones_like(p)
    theirs.step()  # (the loaded state is one torch can step from)
    back = KGEAdagrad(_params(), lr=0.3)
    back.load_state_dict(theirs.state_dict())
    q = back.param_groups[0]["params"][0]
    assert torch.equal(back.state[q]["sum"], st["sum"]) and float(back.state[q]["step"]) == 2.0
    assert back.param_groups[0]["lr"] == 0.5


def test_model_refusals_name_the_optimizer_passed():
    """KGEModel._check_lazy before anything is launched: the four refused configurations."""
    from argparse import Namespace
    from knowledgegraphembedding_amd import KGEAdagrad, KGELazyAdam, KGEModel
    m = KGEModel("TransE", 10, 2, 4, 6.0)
    ok = Namespace(regularization=0.0)
    for cls, who in ((KGEAdagrad, r"KGEAdagrad \(fused lazy Adagrad\)"), (KGELazyAdam, r"KGELazyAdam \(lazy entity Adam\)")):
        opt = cls(list(m.parameters()))
        assert m._check_lazy(opt, ok) is True
        with pytest.raises(ValueError, match=who + " takes no regulariser"):
            m._check_lazy(opt, Namespace(regularization=1e-3))
        with pytest.raises(ValueError, match=who + " does not run with a data-parallel group"):
            m._check_lazy(opt, Namespace(regularization=0.0, dp_group=object()))
        m.row_partition = object()
        with pytest.raises(ValueError, match=who + " does not run with a row partition"):
            m._check_lazy(opt, ok)
        m.row_partition = None
        m.fuse_optimizer = False
        with pytest.raises(ValueError, match=who + " exists only fused"):
            m._check_lazy(opt, ok)
        m.fuse_optimizer = True


def test_run_picks_the_optimizer_from_the_environment(monkeypatch):
    from knowledgegraphembedding_amd import KGEAdagrad, KGEAdam, KGELazyAdam, run
    monkeypatch.delenv("KGE_OPTIMIZER", raising=False)
    monkeypatch.delenv("KGE_ENTITY_ADAM", raising=False)
    assert run.optimizer_class() is KGEAdam
    monkeypatch.setenv("KGE_ENTITY_ADAM", "lazy")
    monkeypatch.setenv("KGE_OPTIMIZER", "adam")
    assert run.optimizer_class() is KGELazyAdam
    for kind in ("adagrad", "adagrad_rowwise"):
        monkeypatch.setenv("KGE_OPTIMIZER", kind)
        with pytest.raises(ValueError, match="KGE_ENTITY_ADAM"):
            run.optimizer_class()
    monkeypatch.setenv("KGE_ENTITY_ADAM", "dense")
    monkeypatch.setenv("KGE_OPTIMIZER", "adagrad")
    assert run.optimizer_class() is KGEAdagrad
    monkeypatch.setenv("KGE_OPTIMIZER", "adagrad_rowwise")
    opt = run.optimizer_class()(_params(), lr=0.25)
    assert isinstance(opt, KGEAdagrad) and opt.rowwise_entity and opt.defaults["lr"] == 0.25
    monkeypatch.setenv("KGE_OPTIMIZER", "sgd")
    with pytest.raises(ValueError, match="KGE_OPTIMIZER"):
        run.optimizer_class()
