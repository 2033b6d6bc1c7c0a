"""The fused lazy Adagrad step on the GPU (kge_train_step_adagrad through
KGEAdagrad): tables, states and losses compared as raw bits against the rule
applied in numpy to EVERY row of the dense gradient (tests/adagrad_cases.py) —
the step touches only its batch's rows, and that must be the dense update —
and within derived bounds against torch.optim.Adagrad on the CPU."""
import numpy as np
import pytest
import torch

import adagrad_cases as A
import lazy_adam_cases as L
from knowledgegraphembedding_amd import KGEAdagrad, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
E, R = 3000, 7


def _check_dense(name, batches, d=64, rowwise=False, modes=L.MODES3, **model):
    """Three fused steps against the composed dense reference, compared after every step.
    Row-wise: the reference moves the entity table by the rule evaluated with the device's
    own G', and G' itself is held to rowsum_bound against double precision.
    Returns the final snapshot."""
    m = L.make_model(name, E, R, d, DEV, **model)
    opt = A.make_opt(m, rowwise)
    per_step = []
    snap = A.run_steps(m, opt, batches, DEV, modes, after_step=lambda k, m_, o_: per_step.append(_tables(m_, o_)))
    losses = snap["losses"]
    twin = L.make_model(name, E, R, d, DEV, **model)
    state = (lambda k: per_step[k]["entity.sum"].cpu().numpy()) if rowwise else None
    G_prev = np.zeros(E, dtype=np.float64)
    Le = m.entity_embedding.shape[1]
    for k, ref in enumerate(A.dense_reference_steps(twin, batches, DEV, modes, rowwise_state=state)):
        got = dict(per_step[k], losses=losses[:k + 1])
        want = {key: ref[key] for key in got}
        A.same_keys_same_bits(got, want, f"{name} d={d} rowwise={rowwise} step {k + 1}")
        if rowwise:
            g = ref["grad.entity"].double().cpu().numpy()
            G64 = G_prev + (g * g).sum(1) / Le
            G1 = got["entity.sum"].double().cpu().numpy()
            err, bound = np.abs(G1 - G64), A.rowsum_bound(G64, Le)
            print(f"{name} d={d} step {k + 1}: max |G' - G'_f64| / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
            assert (err <= bound).all()
            G_prev = G1  # (the next step accumulates onto the device's own fp32 state)
    ops.raise_on_device_error(DEV)
    assert m.entity_embedding.grad is None
    return snap


def _tables(m, opt):
    out = {}
    for k, p in zip(("entity", "relation", "modulus"), L.params_of(m)):
        out[k] = p.detach().clone()
        out[k + ".sum"] = opt.state[p]["sum"].clone()
    return out


# 1 ------------------------------------------- bit-exact against the dense rule
@pytest.mark.parametrize("name", L.NAMES)
def test_equals_the_dense_rule_every_step(name):
    """Rows sit out steps here (staleness_batches): unlike the lazy Adam, nothing differs for them."""
    batches, _ = L.staleness_batches(E, R)
    _check_dense(name, batches)


# 2 ------------------------------------------------- untouched means untouched
_PATTERN = [0x7fc00001, -0x80000000, -0x3edcbb, 0x12345678, 0x7f800001, 0x00000001]  # NaNs, -0.0, a denormal


def _poisoned_run(name, rowwise):
    batches, _ = L.staleness_batches(E, R)
    m = L.make_model(name, E, R, 64, DEV)
    opt = A.make_opt(m, rowwise)
    ent = m.entity_embedding
    st = opt.state[ent]
    st["step"] = torch.tensor(0.0)
    st["sum"] = torch.zeros(E, device=DEV) if rowwise else torch.zeros_like(ent.data)
    untouched = torch.ones(E, dtype=torch.bool, device=DEV)
    for pos, neg, _ in batches:
        untouched[L.touched_ids(pos, neg, E).to(DEV)] = False
    assert untouched.sum() > E // 2
    Le = ent.shape[1]
    pat = torch.tensor(_PATTERN, dtype=torch.int32, device=DEV).repeat(Le // len(_PATTERN) + 1)[:Le]
    ent.data.view(torch.int32)[untouched] = pat
    if rowwise:
        rows = torch.tensor(_PATTERN, dtype=torch.int32, device=DEV).repeat(E // len(_PATTERN) + 1)[:E]
        st["sum"].view(torch.int32)[untouched] = rows[untouched]
    else:
        st["sum"].view(torch.int32)[untouched] = pat.roll(1)
    tensors = (ent.data, st["sum"])
    before = [t.view(torch.int32)[untouched].clone() for t in tensors]
    assert torch.isnan(ent.data[untouched]).any() and torch.isnan(st["sum"][untouched]).any()
    snap = A.run_steps(m, opt, batches, DEV)
    ops.raise_on_device_error(DEV)
    for t, b in zip(tensors, before):
        assert torch.equal(t.view(torch.int32)[untouched], b)
    assert torch.isfinite(snap["losses"]).all() and torch.isfinite(ent.data[~untouched]).all()
    assert torch.isfinite(st["sum"][~untouched]).all()


@pytest.mark.parametrize("name", L.NAMES)
def test_untouched_rows_are_neither_read_nor_written(name):
    _poisoned_run(name, rowwise=False)


# 3 ----------------------------------------------------------------- geometry
@pytest.mark.parametrize("name,d,model", [
    ("RotatE", 1000, {}),                 # 4 column slices of 63 slots, q read slice-major
    ("TransE", 63, {}),                   # single-float slots (VEC = 1)
    ("RotatE", 64, dict(off16=True)),     # a table one float past a 16-byte boundary
    ("ComplEx", 256, {}),
])
def test_row_geometries(name, d, model):
    batches, _ = L.staleness_batches(E, R)
    _check_dense(name, batches, d=d, **model)


@pytest.mark.parametrize("nrows", [96, 97, 99])
@pytest.mark.parametrize("name", ["RotatE", "pRotatE"])
def test_partly_filled_last_block(name, nrows):
    """nrows % 4 of 0, 1 and 3: the last block of row places holds 4, 1 and 3 rows."""
    _check_dense(name, L.exact_rows_batches(E, R, nrows))


@pytest.mark.parametrize("name", ["RotatE", "TransE"])
def test_single_touched_row(name):
    batches = L.single_row_batches(E, R)
    assert all(len(L.touched_ids(p, n, E)) == 1 for p, n, _ in batches)
    _check_dense(name, batches)


@pytest.mark.parametrize("name", L.NAMES)
def test_slice_overrides_keep_the_bits(monkeypatch, name):
    """KGE_ENT_SLICES unset, 0 (the row-per-wave pass), 1 and 2 (the sliced pass): the element-wise
    step on k_entity and on k_entity_sl gives the bits test 1 pins."""
    batches, _ = L.staleness_batches(E, R)
    snaps = []
    for slices in (None, 0, 1, 2):
        if slices is not None:
            monkeypatch.setenv("KGE_ENT_SLICES", str(slices))
        m = L.make_model(name, E, R, 64, DEV)
        snaps.append(A.run_steps(m, A.make_opt(m), batches, DEV))
    ops.raise_on_device_error(DEV)
    for s, slices in zip(snaps[1:], (0, 1, 2)):
        L.assert_same(s, snaps[0], f"{name} KGE_ENT_SLICES={slices}")


# 4 --------------------------------------------- torch.optim.Adagrad on the CPU
@pytest.mark.parametrize("name", ["RotatE", "pRotatE", "TransE"])
def test_against_torch_adagrad_on_the_cpu(name):
    """Each step from the device's own pre-step tables and state: the dense gradient there (a twin
    model holding those tables), one torch.optim.Adagrad step on the CPU, the bounds of
    tests/test_adagrad_ref.py."""
    batches, _ = L.staleness_batches(E, R)
    m = L.make_model(name, E, R, 64, DEV)
    twin = L.make_model(name, E, R, 64, DEV)
    opt = A.make_opt(m)
    keys = ("entity", "relation", "modulus")[:len(L.params_of(m))]
    for (pos, neg, w), mode in zip(batches, L.MODES3):
        pre = _tables(m, opt) if opt.state[m.entity_embedding] else \
            {**{k: p.detach().clone() for k, p in zip(keys, L.params_of(m))},
             **{k + ".sum": torch.zeros_like(p) for k, p in zip(keys, L.params_of(m))}}
        with torch.no_grad():
            for k, p in zip(keys, L.params_of(twin)):
                p.copy_(pre[k])
        twin.compute_train_grads(pos.to(DEV), neg.to(DEV), w.to(DEV), mode, L.train_args())
        A.run_steps(m, opt, [(pos, neg, w)], DEV, (mode,))
        post = _tables(m, opt)
        for k, p in zip(keys, L.params_of(twin)):
            g = p.grad.detach().cpu().numpy()
            tp, ts = A.torch_adagrad_step(pre[k].cpu().numpy(), g, pre[k + ".sum"].cpu().numpy())
            s64 = pre[k + ".sum"].double().cpu().numpy() + g.astype(np.float64) ** 2
            std = np.sqrt(s64) + float(np.float32(A.EPS))
            dp = np.abs(post[k].double().cpu().numpy() - tp)
            ds = np.abs(post[k + ".sum"].double().cpu().numpy() - ts)
            bp, bs = A.p_bound(tp.astype(np.float64), g.astype(np.float64), std), A.sum_bound(s64)
            print(f"{name} {k}: max |dp| / bound {float((dp / np.maximum(bp, 1e-300)).max()):.3f}, "
                  f"max |dsum| / bound {float((ds / np.maximum(bs, 1e-300)).max()):.3f}")
            assert (dp <= bp).all() and (ds <= bs).all(), f"{name} {k}"
    ops.raise_on_device_error(DEV)
    # the state moves to torch.optim.Adagrad and back
    theirs = torch.optim.Adagrad([torch.nn.Parameter(p.detach().clone()) for p in L.params_of(m)], lr=0.5)
    theirs.load_state_dict(opt.state_dict())
    for p, q in zip(L.params_of(m), theirs.param_groups[0]["params"]):
        assert L.same_bits(theirs.state[q]["sum"], opt.state[p]["sum"]) and float(theirs.state[q]["step"]) == 3.0
    back = A.make_opt(L.make_model(name, E, R, 64, DEV))
    back.load_state_dict(theirs.state_dict())
    for p, q in zip(L.params_of(m), back.param_groups[0]["params"]):
        assert L.same_bits(back.state[q]["sum"], opt.state[p]["sum"]) and float(back.state[q]["step"]) == 3.0
    assert back.param_groups[0]["lr"] == A.LR


# 5 ------------------------------------------------------------------ row-wise
@pytest.mark.parametrize("name,d", [(n, 64) for n in L.NAMES] + [("RotatE", 1000)])
def test_rowwise(name, d):
    """One state float per entity row.  G' within (Le + 4)·2^-24·G' of G + Σg²/Le in double from the
    dense gradient's bits; p' the numpy rule with the device's own G', bit for bit; the relation table
    and the modulus element-wise, bit for bit; two runs agree.  d = 1000 would take 4 column slices
    element-wise: the row-wise step has no sliced kernel (its launcher refuses one), so passing here
    is the row-per-wave pass."""
    batches, _ = L.staleness_batches(E, R)
    a = _check_dense(name, batches, d=d, rowwise=True)
    m = L.make_model(name, E, R, d, DEV)
    b = A.run_steps(m, A.make_opt(m, True), batches, DEV)
    ops.raise_on_device_error(DEV)
    L.assert_same(b, a, f"{name} d={d} second run")
    assert tuple(a["entity.sum"].shape) == (E,)


@pytest.mark.parametrize("name", ["RotatE", "TransE"])
def test_rowwise_untouched_rows_are_neither_read_nor_written(name):
    _poisoned_run(name, rowwise=True)


# 6 ------------------------------------------------------- errors and plumbing
@pytest.mark.parametrize("rowwise", [False, True])
@pytest.mark.parametrize("mode", ["head-batch", "tail-batch"])
def test_out_of_range_negative_raises_like_the_dense_step(mode, rowwise):
    from knowledgegraphembedding_amd import KGEAdam
    batches, _ = L.staleness_batches(E, R)
    pos, neg, w = batches[0]
    neg = neg.clone()
    neg[3, 2] = E
    m = L.make_model("RotatE", E, R, 64, DEV)
    L.run_steps(m, KGEAdam(L.params_of(m), lr=L.LR), [(pos, neg, w)], DEV, (mode,))
    with pytest.raises(IndexError):
        ops.raise_on_device_error(DEV)
    m = L.make_model("RotatE", E, R, 64, DEV)
    snap = A.run_steps(m, A.make_opt(m, rowwise), [(pos, neg, w)], DEV, (mode,))
    with pytest.raises(IndexError):
        ops.raise_on_device_error(DEV)
    ops.raise_on_device_error(DEV)  # (cleared)
    assert torch.isfinite(snap["entity"]).all()


def test_train_step_runs_the_fused_step():
    from knowledgegraphembedding_amd import KGEModel
    batches, _ = L.staleness_batches(E, R)
    m0 = L.make_model("RotatE", E, R, 64, DEV)
    want = A.run_steps(m0, A.make_opt(m0), batches, DEV)
    m = L.make_model("RotatE", E, R, 64, DEV)
    opt = A.make_opt(m)
    it = iter([(p, n, w, mode) for (p, n, w), mode in zip(batches, L.MODES3)])
    logs = [KGEModel.train_step(m, opt, it, L.train_args()) for _ in batches]
    got = A.snapshot(m, opt, [want["losses"][k] for k in range(3)])
    L.assert_same(got, want, "train_step")
    for k, log in enumerate(logs):
        assert [log[key] for key in ("positive_sample_loss", "negative_sample_loss", "loss")] == \
            want["losses"][k, :3].tolist()
    assert m.entity_embedding.grad is None and m.relation_embedding.grad is not None


def test_adagrad_step_op_is_the_rule():
    """ops.adagrad_step (kge_adagrad_step): the element-wise rule's bits, a tail that is no multiple of 4."""
    rng = np.random.default_rng(4)
    n = 4 * 1031 + 3
    p, g = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    s = rng.random(n).astype(np.float32)
    g[::7] = 0.0
    tp, tg, ts = (torch.from_numpy(x).to(DEV) for x in (p, g, s))
    ops.adagrad_step(tp, tg, ts, lr=A.LR, eps=A.EPS)
    p1, s1 = A.adagrad_elem_ref(p, g, s)
    assert np.array_equal(tp.cpu().numpy().view(np.int32), p1.view(np.int32))
    assert np.array_equal(ts.cpu().numpy().view(np.int32), s1.view(np.int32))
    with pytest.raises(ValueError):
        ops.adagrad_step(tp, tg, ts, lr=A.LR, eps=0.0)


def test_step_updates_a_parameter_the_fused_step_left():
    """KGEAdagrad.step() on a parameter with a dense .grad: kge_adagrad_step, state keys 'step' and 'sum'."""
    torch.manual_seed(1)
    p = torch.nn.Parameter(torch.randn(33, 8, device=DEV))
    opt = KGEAdagrad([p], lr=A.LR, eps=A.EPS)
    p0 = p.detach().cpu().numpy()
    p.grad = torch.randn(33, 8, device=DEV)
    opt.step()
    p1, s1 = A.adagrad_elem_ref(p0, p.grad.cpu().numpy(), np.zeros_like(p0))
    assert np.array_equal(p.detach().cpu().numpy().view(np.int32), p1.view(np.int32))
    assert set(opt.state[p]) == {"step", "sum"} and float(opt.state[p]["step"]) == 1.0
    assert np.array_equal(opt.state[p]["sum"].cpu().numpy().view(np.int32), s1.view(np.int32))


@pytest.mark.parametrize("kind", ["adagrad", "adagrad_rowwise"])
def test_run_creates_the_optimizer_at_the_start_and_at_the_decay(tmp_path, monkeypatch, kind):
    from knowledgegraphembedding_amd import run
    data = L.write_dataset(str(tmp_path / "data"))
    monkeypatch.setenv("KGE_OPTIMIZER", kind)
    monkeypatch.delenv("KGE_ENTITY_ADAM", raising=False)
    made, pick = [], run.optimizer_class

    def counted():
        factory = pick()

        def make(*a, **k):
            made.append(factory(*a, **k))
            return made[-1]
        return make

    monkeypatch.setattr(run, "optimizer_class", counted)
    torch.manual_seed(0)
    save = str(tmp_path / "save")
    run.main(run.parse_args(["--cuda", "--do_train", "--device_sampler", "--data_path", data, "--model", "RotatE",
                             "-de", "-n", "16", "-b", "32", "-d", "16", "-g", "6.0", "-adv", "-lr", "0.01",
                             "--max_steps", "12", "--warm_up_steps", "5", "--log_steps", "4",
                             "--save_checkpoint_steps", "100", "-save", save, "-cpu", "1"]))
    assert len(made) == 2 and all(isinstance(o, KGEAdagrad) for o in made)
    assert all(o.rowwise_entity == (kind == "adagrad_rowwise") for o in made)
    assert [o.defaults["lr"] for o in made] == [0.01, pytest.approx(0.001)]
    ckpt = torch.load(save + "/checkpoint", map_location="cpu", weights_only=True)
    assert ckpt["current_learning_rate"] == pytest.approx(0.001) and ckpt["warm_up_steps"] == 15
    st = ckpt["optimizer_state_dict"]["state"][0]
    assert set(st) == {"step", "sum"}
    assert tuple(st["sum"].shape) == ((40,) if kind == "adagrad_rowwise" else (40, 32))
    assert float(st["step"]) == 6.0  # steps 6..11 with the optimizer made at the decay (zero state there)


@pytest.mark.parametrize("config", ["row partition", "data-parallel group", "unfused", "regulariser"])
def test_refused_configurations(config):
    from argparse import Namespace
    from knowledgegraphembedding_amd import KGEModel
    batches, _ = L.staleness_batches(E, R)
    m = L.make_model("TransE", E, R, 64, DEV)
    opt = A.make_opt(m)
    args = L.train_args()
    if config == "row partition":
        m.row_partition = object()
    elif config == "data-parallel group":
        args = Namespace(**vars(args), dp_group=object())
    elif config == "unfused":
        m.fuse_optimizer = False
    else:
        args.regularization = 1e-3
    before = m.entity_embedding.detach().clone()
    it = iter([(p, n, w, mode) for (p, n, w), mode in zip(batches, L.MODES3)])
    with pytest.raises(ValueError, match="KGEAdagrad"):
        KGEModel.train_step(m, opt, it, args)
    assert L.same_bits(m.entity_embedding, before) and not opt.state[m.entity_embedding]
