"""Lazy entity Adam on the GPU (kge_train_step_lazy through KGELazyAdam): tables,
moments, relation table and losses compared as raw bits against the dense
fused step where the two must agree, against a reference composed from parts
tested elsewhere where they must not, and against the rule's plain-torch
restatement (tests/lazy_adam_cases.py)."""
import pytest
import torch

import lazy_adam_cases as L
from knowledgegraphembedding_amd import KGEAdam, KGELazyAdam, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
E, R = 3000, 7


def _opt(cls, m):
    return cls(L.params_of(m), lr=L.LR, betas=L.BETAS, eps=L.EPS)


def _run(cls, name, batches, d=64, nent=E, modes=L.MODES3, **model):
    m = L.make_model(name, nent, R, d, DEV, **model)
    opt = _opt(cls, m)
    snap = L.run_steps(m, opt, batches, DEV, modes)
    return m, opt, snap


# 1 ------------------------------------------------------ step 1 equals dense
@pytest.mark.parametrize("slices", [None, 0, 1, 2])
@pytest.mark.parametrize("mode", ["head-batch", "tail-batch"])
@pytest.mark.parametrize("name", L.NAMES)
def test_first_step_equals_dense(monkeypatch, name, mode, slices):
    """From zero moments an untouched row's dense update is p + (-step)·(0 / eps) = p."""
    if slices is not None:
        monkeypatch.setenv("KGE_ENT_SLICES", str(slices))
    batches, _ = L.staleness_batches(E, R)
    _, _, dense = _run(KGEAdam, name, batches[:1], modes=(mode,))
    m, _, lazy = _run(KGELazyAdam, name, batches[:1], modes=(mode,))
    ops.raise_on_device_error(DEV)
    L.assert_same(lazy, dense, f"{name} {mode} slices={slices}")
    assert m.entity_embedding.grad is None


# 2 ---------------------------------------- every row touched: dense, every step
def _all_rows_batches(nent, B=32, n=48, seed=3):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(3):
        pos = torch.stack([torch.randint(0, nent, (B,), generator=g), torch.randint(0, R, (B,), generator=g),
                           torch.randint(0, nent, (B,), generator=g)], 1)
        neg = torch.randint(0, nent, (B, n), generator=g)
        neg[0, :nent] = torch.arange(nent)
        out.append((pos, neg, torch.rand(B, generator=g) + 0.2))
    return out


@pytest.mark.parametrize("name", L.NAMES)
def test_all_rows_touched_equals_dense_every_step(name):
    """The U = E branch of the entity launch's bound: min(E, B·n + 2B) = E = 40."""
    batches = _all_rows_batches(40)
    assert all(len(L.touched_ids(p, n, 40)) == 40 for p, n, _ in batches)
    _, _, dense = _run(KGEAdam, name, batches, nent=40)
    _, _, lazy = _run(KGELazyAdam, name, batches, nent=40)
    ops.raise_on_device_error(DEV)
    L.assert_same(lazy, dense, name)


# 3 ------------------------------------------ staleness, composed reference
def _check_composed(name, batches, d=64, modes=L.MODES3, **model):
    """The lazy run equals, bit for bit, the run composed from the dense gradients
    and ops.adam_step on the touched rows; returns both and the composition's parts."""
    m, opt, lazy = _run(KGELazyAdam, name, batches, d=d, modes=modes, **model)
    twin = L.make_model(name, E, R, d, DEV, **model)
    ref, grads, touched = L.composed_reference(twin, batches, DEV, modes)
    ops.raise_on_device_error(DEV)
    L.assert_same(lazy, ref, f"{name} lazy vs composed")
    assert m.entity_embedding.grad is None
    return lazy, ref, grads, touched


@pytest.mark.parametrize("name", L.NAMES)
def test_staleness_against_composed_reference(name):
    batches, marked = L.staleness_batches(E, R)
    marked = marked.to(DEV)
    lazy, ref, grads, touched = _check_composed(name, batches)
    for k, ids in enumerate(touched):  # entity 0 and E - 1: touched in steps 1 and 3, untouched in step 2
        assert bool(torch.isin(marked, ids).all()) == (k != 1) and bool(torch.isin(marked, ids).any()) == (k != 1)
    # the dense fused run moves the marked rows at step 2 (it decays their moments): it must differ there
    _, _, dense2 = _run(KGEAdam, name, batches[:2])
    _, _, lazy2 = _run(KGELazyAdam, name, batches[:2])
    ops.raise_on_device_error(DEV)
    for k in ("entity", "entity.m", "entity.v"):
        diff = (L.bits(dense2[k])[marked] != L.bits(lazy2[k])[marked]).any(dim=1)
        assert diff.all(), f"{name}: dense and lazy agree on marked rows of {k} after step 2"
    # independently: the plain-torch restatement of the rule, fed the same GPU gradients
    p0 = L.make_model(name, E, R, 64, DEV).entity_embedding.detach()
    want = L.lazy_adam_ref(p0, grads, touched)
    for k, w in zip(("entity", "entity.m", "entity.v"), want):
        torch.testing.assert_close(lazy[k], w, rtol=2e-6, atol=1e-7, msg=lambda s: f"{name} {k}: {s}")


# 4 ----------------------------------------------------------------- geometry
@pytest.mark.parametrize("nrows", [96, 97, 99])
@pytest.mark.parametrize("name", L.NAMES)
def test_partly_filled_last_block(name, nrows):
    """nrows % 4 of 0, 1 and 3: the last block of row places holds 4, 1 and 3 rows."""
    assert nrows % 4 in (0, 1, 3)
    _check_composed(name, L.exact_rows_batches(E, R, nrows))


@pytest.mark.parametrize("name", L.NAMES)
def test_single_touched_row(name):
    batches = L.single_row_batches(E, R)
    assert all(len(L.touched_ids(p, n, E)) == 1 for p, n, _ in batches)
    _check_composed(name, batches)


@pytest.mark.parametrize("name,d,model", [
    ("RotatE", 1000, {}),                 # 4 column slices of 63 slots, q read slice-major
    ("TransE", 63, {}),                   # single-float slots (VEC = 1)
    ("RotatE", 64, dict(off16=True)),     # a table one float past a 16-byte boundary
    ("ComplEx", 256, {}),
])
def test_row_geometries(name, d, model):
    batches, _ = L.staleness_batches(E, R)
    _check_composed(name, batches, d=d, **model)


@pytest.mark.parametrize("switch", ["KGE_CSR_SERIAL", "KGE_FIN_SEPARATE"])
@pytest.mark.parametrize("name,d", [("RotatE", 1000), ("pRotatE", 64)])
def test_host_switches_keep_the_bits(monkeypatch, name, d, switch):
    """KGE_CSR_SERIAL=1 builds the CSR — and behind it the touched-row list — on the caller's
    stream instead of the side stream; KGE_FIN_SEPARATE=1 launches the loss finalisation on
    its own.  Also keep_grads off (no relation gradient stream).  Same bits."""
    batches, _ = L.staleness_batches(E, R)
    snaps = []
    for on in (False, True):
        if on:
            monkeypatch.setenv(switch, "1")
        m = L.make_model(name, E, R, d, DEV)
        m.keep_grads = not on
        snaps.append(L.run_steps(m, _opt(KGELazyAdam, m), batches, DEV))
    ops.raise_on_device_error(DEV)
    L.assert_same(snaps[1], snaps[0], f"{name} {switch}")


# 5 ------------------------------------------------- untouched means untouched
_PATTERN = [0x7fc00001, -0x80000000, -0x3edcbb, 0x12345678, 0x7f800001, 0x00000001]  # NaNs, -0.0, a denormal


@pytest.mark.parametrize("name", L.NAMES)
def test_untouched_rows_are_neither_read_nor_written(name):
    batches, _ = L.staleness_batches(E, R)
    m = L.make_model(name, E, R, 64, DEV)
    opt = _opt(KGELazyAdam, m)
    ent = m.entity_embedding
    st = opt.state[ent]
    st["step"] = torch.tensor(0.0)
    st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(ent.data), torch.zeros_like(ent.data)
    untouched = torch.ones(E, dtype=torch.bool, device=DEV)
    for pos, neg, _ in batches:
        untouched[L.touched_ids(pos, neg, E).to(DEV)] = False
    assert untouched.sum() > E // 2
    pat = torch.tensor(_PATTERN, dtype=torch.int32, device=DEV).repeat(ent.shape[1] // len(_PATTERN) + 1)[:ent.shape[1]]
    tensors = (ent.data, st["exp_avg"], st["exp_avg_sq"])
    for k, t in enumerate(tensors):
        t.view(torch.int32)[untouched] = pat.roll(k)
    before = [t.view(torch.int32)[untouched].clone() for t in tensors]
    assert torch.isnan(ent.data[untouched]).any()
    snap = L.run_steps(m, opt, batches, DEV)
    ops.raise_on_device_error(DEV)
    for t, b in zip(tensors, before):
        assert torch.equal(t.view(torch.int32)[untouched], b)
    assert torch.isfinite(snap["losses"]).all() and torch.isfinite(ent.data[~untouched]).all()


# 6 --------------------------------------------------------------- determinism
@pytest.mark.parametrize("name", L.NAMES)
def test_deterministic_and_no_dense_entity_gradient(name):
    batches, _ = L.staleness_batches(E, R)
    m, _, a = _run(KGELazyAdam, name, batches)
    _, _, b = _run(KGELazyAdam, name, batches)
    ops.raise_on_device_error(DEV)
    L.assert_same(a, b, name)
    assert m.entity_embedding.grad is None and m.relation_embedding.grad is not None
    shape = tuple(m.entity_embedding.shape)
    assert all(t is None or tuple(t.shape) != shape for t in m._grad_bufs)


# 7 -------------------------------------------------------- handled index error
@pytest.mark.parametrize("mode", ["head-batch", "tail-batch"])
@pytest.mark.parametrize("name", L.NAMES)
def test_out_of_range_negative_raises_like_the_dense_step(name, mode):
    """A refusal the kernels already implement (the id reaches no bucket and no row; the
    error flag is set): IndexError at the next sync, the tables as the dense step leaves them."""
    batches, _ = L.staleness_batches(E, R)
    pos, neg, w = batches[0]
    neg = neg.clone()
    neg[3, 2] = E
    snaps = []
    for cls in (KGEAdam, KGELazyAdam):
        m = L.make_model(name, E, R, 64, DEV)
        opt = _opt(cls, m)
        snaps.append(L.run_steps(m, opt, [(pos, neg, w)], DEV, (mode,)))
        with pytest.raises(IndexError):
            ops.raise_on_device_error(DEV)
        ops.raise_on_device_error(DEV)  # (cleared)
    L.assert_same(snaps[1], snaps[0], f"{name} {mode}")


# ----------------------------------------------------- KGEModel.train_step
def test_train_step_runs_the_lazy_step():
    """The reference's entry (model.py:252-312) with a lazy optimizer: the same tables,
    moments and logged losses as the steps queued by hand."""
    from knowledgegraphembedding_amd import KGEModel
    batches, _ = L.staleness_batches(E, R)
    _, _, want = _run(KGELazyAdam, "RotatE", batches)
    m = L.make_model("RotatE", E, R, 64, DEV)
    opt = _opt(KGELazyAdam, m)
    it = iter([(p, n, w, mode) for (p, n, w), mode in zip(batches, L.MODES3)])
    logs = [KGEModel.train_step(m, opt, it, L.train_args()) for _ in batches]
    got = L.snapshot(m, opt, [want["losses"][k] for k in range(3)])
    L.assert_same(got, want, "train_step")
    for k, log in enumerate(logs):
        assert [log[key] for key in ("positive_sample_loss", "negative_sample_loss", "loss")] == \
            want["losses"][k, :3].tolist()
    assert m.entity_embedding.grad is None


# ------------------------------------------------------------------ run.py
def test_run_creates_the_lazy_optimizer_at_the_start_and_at_the_decay(tmp_path, monkeypatch):
    """run.py under KGE_ENTITY_ADAM=lazy: the optimizer comes from run.adam_class() both at the
    start and when the learning rate decays (step 5 of 12 here), and trains with it."""
    from knowledgegraphembedding_amd import run
    data = L.write_dataset(str(tmp_path / "data"))
    monkeypatch.setenv("KGE_ENTITY_ADAM", "lazy")
    made, pick = [], run.adam_class

    def counted():
        made.append(pick())
        return made[-1]

    monkeypatch.setattr(run, "adam_class", counted)
    torch.manual_seed(0)
    save = str(tmp_path / "save")
    run.main(run.parse_args(["--cuda", "--do_train", "--device_sampler", "--data_path", data, "--model", "RotatE",
                             "-de", "-n", "16", "-b", "32", "-d", "16", "-g", "6.0", "-adv", "-lr", "0.01",
                             "--max_steps", "12", "--warm_up_steps", "5", "--log_steps", "4",
                             "--save_checkpoint_steps", "100", "-save", save, "-cpu", "1"]))
    assert made == [KGELazyAdam, KGELazyAdam]
    ckpt = torch.load(save + "/checkpoint", map_location="cpu", weights_only=True)
    assert ckpt["current_learning_rate"] == pytest.approx(0.001) and ckpt["warm_up_steps"] == 15
    assert set(ckpt["optimizer_state_dict"]["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
