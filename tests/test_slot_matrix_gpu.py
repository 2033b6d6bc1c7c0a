"""Every row-slot instantiation, unaligned tables and trained-regime inputs
through the HIP kernels, against the oracle in double (GPU box).

The case table, the fp64 reference (ref64) and the per-row criterion are
tests/test_slot_matrix_ref.py's (its docstring has the definitions):

    scores, losses:  |Δ| <= score_tol(ref64)
    gradient rows:   max|got[r] - ref64[r]| <= rtol_case · max|ref64[r]| + 1e-20 · max|ref64|
    rtol_case = max(8 · rho_case, 32 · 2^-24), rho_case the fp32 oracle's own distance from ref64

Per case of B (all ten (vec, ns) instantiations at both edges, five models)
and C (tables 4 bytes past a 16-byte boundary: single-float slots with every
lane full; RotatE / DistMult also with only one of the two tables unaligned):
forward() in its three modes, the fused train step in both modes, the
backward of forward() under a non-constant upstream gradient, one fused Adam
step bit-identical to KGEAdam.step() on the same gradients, and filtered
ranks equal to the oracle's (not pRotatE, whose device sin is correctly
rounded: test_rank_parity_gpu; not span 4: the refinement's ATen-order sum
takes 8 elements or more).  D (trained regime, spans 64 and 63): the fused
train step on a peaked adversarial softmax (spread of T·s in [30, 80], the
positive's true entity among the negatives), without the softmax, with
uni_weight, on saturated log_sigmoid / sigmoid arguments, on elements of
exactly zero distance, and with n = 2, 3, 5 negatives for k_row's four waves.

C has no bit-identity check against an aligned table: the same span in an
aligned table runs float4 slots, whose lane-local sums run in another order
(DESIGN §3 fixes the summation order per (vec, ns), not across them), so the
fp64 criterion alone holds there.

Recorded on an MI355X (worst over the model's cases; ratio = err / (rtol_case
· rowmax + floor), the criterion is ratio <= 1):

    model      worst rho_case   worst kernel ratio
    TransE     1.53e-05         0.136  (span 9, train head-batch, entity)
    DistMult   1.18e-06         0.148  (unaligned span 128, train tail-batch, entity)
    ComplEx    3.18e-06         0.170  (span 127, train head-batch, entity)
    RotatE     3.44e-05         0.315  (span 260, backward head-batch, entity)
    pRotatE    8.54e-06         0.813  (span 4, backward head-batch, modulus: rtol_case at its
                                        floor 32·2^-24, one sum of 140 |sin| terms)

Sensitivity (scratch builds, not committed).  load_row's upper-half select
keeping the loaded value instead of 0 (real parts only): 110 of the 175 tests
here fail — every case with a partial slot; the cases with every lane full
cannot see it.  k_row's V not rescaled when the running maximum rises: 155
fail, the peaked cases among them only because the dominant negative is not
the first of its wave and the others score near 0 (true_column, PEAKED).
test_gpu_parity.py / test_edge_gpu.py catch both as well (73 and 23 failures).
"""
import math
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import score_tol
from knowledgegraphembedding_amd import KGEAdam, _lib, ops
from oracle import kge_oracle as O
from test_gpu_parity import DEV, build_model
from test_slot_matrix_ref import (ALL_SLOTS, CASES_B, CASES_C, CASES_D, E, MODES, NAMES, R, Case, expected_slots,
                                  inputs, ratio_of, references, _seed)

pytestmark = pytest.mark.gpu

WORST = {}   # model -> [worst rho_case, worst kernel ratio, the case and tensor it was seen in]
COVERED = set()  # (model, mode, vec, ns) whose train step ran and met the criterion


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nslot matrix: model, worst rho_case, worst kernel ratio (where)")
    for nm in NAMES:
        if nm in WORST:
            print("slot matrix: %-9s %.3e  %.3f  (%s)" % (nm, *WORST[nm]))


def _note(case, rho, ratio, where):
    w = WORST.setdefault(case.name, [0.0, 0.0, ""])
    w[0] = max(w[0], rho)
    if ratio > w[1]:
        w[1], w[2] = ratio, f"{case.id} {where}"


def unaligned(t):
    """A contiguous copy of t one float into a larger buffer: data_ptr() % 16 == 4."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def make_model(inp):
    """build_model's KGEModel holding the case's tables (B: the very tables build_model makes),
    each at the case's alignment."""
    c = inp.case
    m, *_ = build_model(c.name, E, R, c.span, inp.gamma, _seed(c))
    assert m._host_scalars() == (inp.g32, inp.erange)
    for p, arr, al in ((m.entity_embedding, inp.ent, c.ent_aligned), (m.relation_embedding, inp.rel, c.rel_aligned)):
        t = torch.from_numpy(arr).to(DEV)
        if c.kind == "init":
            assert torch.equal(p.data, t)
        p.data = t if al else unaligned(t)
        assert (p.data_ptr() % 16 == 0) == al
    if inp.mod is not None:
        m.modulus.data = torch.from_numpy(inp.mod).to(DEV)
    return m


def _dev(inp, mode):
    return (torch.from_numpy(inp.pos).to(DEV), None if mode == "single" else torch.from_numpy(inp.neg[mode]).to(DEV))


def _grads_of(m):
    return [m.entity_embedding.grad, m.relation_embedding.grad, m.modulus.grad if hasattr(m, "modulus") else None]


def check_scores(m, ref, fails):
    inp = ref.inp
    with torch.no_grad():
        for mode, s64 in ref.forward.items():
            P, N = _dev(inp, mode)
            s = (m(P) if mode == "single" else m((P, N), mode)).cpu().numpy()
            ops.raise_on_device_error(DEV)
            bad = np.abs(s - s64) > score_tol(s64)
            if bad.any() or not np.isfinite(s).all():
                fails.append(f"forward {mode}: max|Δ| {np.abs(s - s64).max():.3e}")


def check_grads(case, got, g64, ref, where, fails):
    for g, r, nm in zip(got, g64, ("entity", "relation", "modulus")):
        if r is None:
            continue
        g = g.detach().cpu().numpy()
        ratio = ratio_of(g, r, ref.rtol) if np.isfinite(g).all() else math.inf
        _note(case, ref.rho, ratio, f"{where} {nm}")
        print(f"{case.id} {where} {nm}: rho_case {ref.rho:.3e} rtol_case {ref.rtol:.3e} ratio {ratio:.3f}")
        if not ratio <= 1.0:
            fails.append(f"{where} grad_{nm}: ratio {ratio:.3f} (rtol_case {ref.rtol:.3e})")


def check_train(m, ref, fails):
    inp, case = ref.inp, ref.inp.case
    W = torch.from_numpy(inp.w).to(DEV)
    for tr, (l64, g64) in zip(inp.trains, ref.train):
        P, N = _dev(inp, tr.mode)
        args = Namespace(negative_adversarial_sampling=tr.adversarial, adversarial_temperature=tr.temperature,
                         uni_weight=tr.uni_weight, regularization=tr.regularization)
        losses = m.compute_train_grads(P, N, W, tr.mode, args).cpu().numpy()
        ops.raise_on_device_error(DEV)
        where = f"train {tr.mode} adv={tr.adversarial} T={tr.temperature} uni={tr.uni_weight}"
        if not (np.isfinite(losses[:3]).all() and np.all(np.abs(losses[:3] - l64) <= score_tol(l64))):
            fails.append(f"{where} losses {losses[:3]} vs {l64}")
        before = len(fails)
        check_grads(case, _grads_of(m), g64, ref, where, fails)
        if len(fails) == before:
            COVERED.add((case.name, tr.mode) + case.slots)


def check_backward(m, ref, fails):
    inp, case = ref.inp, ref.inp.case
    for mode, (s64, g64) in ref.backward.items():
        for p in m.parameters():
            p.grad = None
        P, N = _dev(inp, mode)
        s = m(P) if mode == "single" else m((P, N), mode)
        s.backward(torch.from_numpy(inp.gout[mode]).to(DEV))
        ops.raise_on_device_error(DEV)
        check_grads(case, _grads_of(m), g64, ref, f"backward {mode}", fails)


def check_fused_adam(ref, fails):
    """One fused Adam step (inside the gradient passes, on the tables at the case's alignment)
    against KGEAdam.step() on the same gradients: parameters, moments and .grad bit for bit.
    The unfused step runs on aligned copies (kge_adam_step takes aligned tensors only)."""
    inp = ref.inp
    tr = inp.trains[-1]
    args = Namespace(negative_adversarial_sampling=tr.adversarial, adversarial_temperature=tr.temperature,
                     uni_weight=tr.uni_weight, regularization=tr.regularization)
    P, N = _dev(inp, tr.mode)
    W = torch.from_numpy(inp.w).to(DEV)
    names = ["entity_embedding", "relation_embedding"] + (["modulus"] if inp.mod is not None else [])
    mf = make_model(inp)
    of = KGEAdam([getattr(mf, k) for k in names], lr=3e-3)
    mf.compute_train_grads(P, N, W, tr.mode, args, optimizer=of)
    of.step()
    mu = make_model(inp)
    mu.compute_train_grads(P, N, W, tr.mode, args)
    ops.raise_on_device_error(DEV)
    ps = [torch.nn.Parameter(getattr(mu, k).detach().clone()) for k in names]
    for p, k in zip(ps, names):
        p.grad = getattr(mu, k).grad.clone()
    ou = KGEAdam(ps, lr=3e-3)
    ou.step()
    for p, k in zip(ps, names):
        f = getattr(mf, k)
        same = (torch.equal(f.detach(), p.detach()) and torch.equal(f.grad, p.grad)
                and torch.equal(of.state[f]["exp_avg"], ou.state[p]["exp_avg"])
                and torch.equal(of.state[f]["exp_avg_sq"], ou.state[p]["exp_avg_sq"]))
        if not same:
            fails.append(f"fused Adam differs from KGEAdam.step() on {k}")


def _oracle_ranks(inp, mode):
    t = lambda a: None if a is None else torch.from_numpy(a)  # noqa: E731
    tri = inp.pos.tolist()
    return O.filtered_ranks(inp.case.name, t(inp.ent), t(inp.rel), t(inp.mod), tri, tri, mode, inp.g32,
                            inp.erange)["rank_count"]


def check_ranks(m, ref, fails):
    inp, case = ref.inp, ref.inp.case
    if case.name == "pRotatE" or case.span == 4:
        return
    tri = inp.pos.tolist()
    trigs = [None]
    if case.name == "RotatE" and case.sec == "C":
        # the reference's cos | sin table, aligned and not (read with the row's slot geometry)
        trig = ops.reference_rotation(m.relation_embedding, inp.erange).to(DEV)
        trigs = [trig, unaligned(trig)]
    for mode in MODES:
        want = _oracle_ranks(inp, mode)
        for trig in trigs:
            ranks, _ = m.rank_queries(tri, tri, mode, relation_trig=trig)
            if not np.array_equal(ranks, want):
                fails.append(f"ranks {mode} {ranks} vs {want}" + ("" if trig is None else
                                                                  f" (trig at % 16 = {trig.data_ptr() % 16})"))


@pytest.mark.parametrize("case", CASES_B + CASES_C, ids=lambda c: c.id)
def test_slot_matrix(case):
    ref = references(case)
    m = make_model(ref.inp)
    fails = []
    check_scores(m, ref, fails)
    check_train(m, ref, fails)
    check_backward(m, ref, fails)
    check_fused_adam(ref, fails)
    check_ranks(m, ref, fails)
    assert not fails, "\n".join([case.id + f" (vec, ns) = {case.slots}"] + fails)


@pytest.mark.parametrize("case", CASES_D, ids=lambda c: c.id)
def test_trained_regime(case):
    ref = references(case)
    m = make_model(ref.inp)
    fails = []
    check_scores(m, ref, fails)
    check_train(m, ref, fails)
    assert not fails, "\n".join([case.id] + fails)


def test_zz_every_instantiation_ran():
    """The fused train step of every model ran, and met the criterion, in both modes at all ten
    (vec, ns) pairs that check_model can pick for rows of up to 2048 floats.  (After the matrix
    in file order; a B case that has not run in this session, say under -k, runs here.)"""
    for case in CASES_B:
        if any((case.name, mode) + case.slots not in COVERED for mode in MODES):
            ref = references(case)
            check_train(make_model(ref.inp), ref, [])
    for nm in NAMES:
        for mode in MODES:
            got = {(v, s) for (n_, m_, v, s) in COVERED if n_ == nm and m_ == mode}
            assert got == ALL_SLOTS, (nm, mode, sorted(ALL_SLOTS - got))


# --------------------------------------------------- ranking, unaligned table
@pytest.mark.parametrize("name", NAMES)
def test_unaligned_entity_table_rank_paths(name):
    """An entity table that is not 16-byte aligned is ranked by the wave scan (path "auto":
    the oracle's ranks, in test_slot_matrix's C cases); an explicit request for a fast pass
    that reads 16 bytes at a time is refused on the host (KGE_ERR_ARG) before any launch."""
    case = Case("C", name, 256, ent_aligned=False, rel_aligned=True)
    inp = inputs(case)
    assert expected_slots(256, False, True) == (1, 4)
    m = make_model(inp)
    tri = inp.pos.tolist()
    for path in ("mfma", "mfma32", "tile"):
        with pytest.raises(_lib.KGEHipError, match="status 4"):
            m.rank_queries(tri, tri, "tail-batch", path=path)
    ops.raise_on_device_error(DEV)
    if name != "pRotatE":
        ranks, _ = m.rank_queries(tri, tri, "tail-batch", path="scan")
        assert np.array_equal(ranks, _oracle_ranks(inp, "tail-batch"))


def test_unaligned_rotation_table_needs_single_float_slots():
    """RotatE's relation_trig is read with the row's slot geometry: with float4 slots (aligned
    tables, span 256) an unaligned one is refused (KGE_ERR_ARG), an aligned one ranks."""
    inp = inputs(Case("B", "RotatE", 256))
    m = make_model(inp)
    tri = inp.pos.tolist()
    trig = ops.reference_rotation(m.relation_embedding, inp.erange).to(DEV)
    with pytest.raises(_lib.KGEHipError, match="status 4"):
        m.rank_queries(tri, tri, "head-batch", relation_trig=unaligned(trig))
    ranks, _ = m.rank_queries(tri, tri, "head-batch", relation_trig=trig)
    assert np.array_equal(ranks, _oracle_ranks(inp, "head-batch"))
