"""kge_ship_step stage by stage in one process, against the oracle in double
(GPU box).

tests/ship_cases.py's run_ship plays every rank of a query-shipping step in
turn on one stream, with the collectives between the five stages emulated as
fp32 sums in rank order, every device pointer the view of an exactly sized
guard-banded arena, and each rank's entity table, grad_entity and Adam moments a
full [E, Le] arena at its fill with only the owned rows copied in (its docstring
has the layout and what is checked after every stage of every rank: status,
err_flag, bands, read-only buffers, rows outside [lo, hi)).  The case table,
inputs, fp64 reference (ref64) and the per-row criterion are
tests/test_slot_matrix_ref.py's, unchanged:

    losses:          |Δ| <= score_tol(ref64)
    gradient rows:   max|got[r] - ref64[r]| <= rtol_case · max|ref64[r]| + 1e-20 · max|ref64|
    rtol_case = max(8 · rho_case, 32 · 2^-24), rho_case the fp32 oracle's own distance from ref64

Nothing here is compared against kge_train_step_grads.  Cases: every CASES_B case
(all ten (vec, ns) row-slot instantiations at both edges, five models) under the
shard patterns W4 and W3; the two wide-negative cases (n = 300, 257: k_ship_merge's
j loop strides) under W4; every CASES_D case under W2 (the dominant negative alone
in its shard), W4 and W1; RotatE's and DistMult's both-unaligned CASES_C spans
under W4 in test_slot_matrix_gpu.unaligned tables (values only).  Every case runs
every Train of its inputs: both modes, adversarial on and off, uni_weight, and
regularization 1e-4 for DistMult / ComplEx.

After the step: (1) the union of the ranks' owned grad_entity rows, the
rank-order sum of grad_relation and every rank's grad_modulus meet the criterion
(the per-row floor from the whole table's maximum) and are finite; (2) every
rank's losses[0], losses[1] are within score_tol of ref64's, and so is the step's
loss (l0 + l1) / 2 + reg with reg the rank-order fp32 sum of the ranks'
losses[3], itself within score_tol of the oracle's 'regularization' (a rank's own
losses[2] holds its own part of reg only, as partition.py's all-reduce of
losses[3] expects; without regularisation it is compared as it stands);
(3) row_stats after CHAIN, losses[0], losses[1] and pRotatE's grad_modulus are
bit-identical across the emulated ranks; (4) after MERGE each rank's g is finite
wherever it owns the negative.  test_ship_fused_adam: per CASES_B case under W4
with the case's last Train, the step again with adam != NULL from random non-zero
moments at step count 3: owned rows of param / exp_avg / exp_avg_sq bit-identical
to ops.adam_step on the adam == NULL run's gradient rows, .grad bit-identical
between the runs, pRotatE's modulus and its moments identical across ranks and
equal to ops.adam_step on grad_modulus, and with write_grad = 0 grad_entity all
fill.  test_ship_index_errors: an id of E or -1 in one positive's h, or in one
negative: every stage KGE_OK, KGE_DEVERR_INDEX on every rank after the step,
no band and no row outside [lo, hi) written; values are not compared.

Recorded on an MI355X (worst over the model's cases and patterns; ratio = err /
(rtol_case · rowmax + floor), the criterion is ratio <= 1; no tensor needed an
rtol of its own, every rtol is the slot matrix's rtol_case):

    model      worst kernel ratio
    TransE     0.136  (span 9, W4, head-batch, entity)
    DistMult   0.151  (span 260, W4, tail-batch, entity)
    ComplEx    0.170  (span 127, W4, head-batch, entity)
    RotatE     0.282  (span 260, W4, head-batch, entity)
    pRotatE    0.148  (span 255, W4, head-batch, entity)

270 tests, 34 s for the module; the slowest is the first, test_ship_stages
[B-TransE-4-init] at 1.3 s (it loads the library), every other test under 0.5 s.
All pass on the committed library: no stage reads or writes a row outside
[own_begin, own_end), a band, or a byte of a read-only buffer.

Sensitivity (scratch builds, not committed, each run once through this module;
both change arithmetic, not addressing).  k_ship_merge taking the own shard's f
as 1 (no cross-shard rescale of V): 138 of the 270 fail — 101 of the 105
test_ship_stages, both wide-negative cases, 11 of the 12 unaligned, the coverage
test and 23 of the 29 trained-regime cases, all ten peaked ones among them, each
under W2 (where shard 1's V must shrink by exp(-spread)) and none under W1 (one
shard: f is 1).  The 6 saturated distance-model cases pass it.  k_ship_chain
head-batch dropping the positive's relation share (dra = rna): 130 fail, every
one at a head-batch grad_relation — all 105 test_ship_stages, the wide-negative
and unaligned cases, the coverage test and 10 trained-regime cases (peaked
DistMult / ComplEx, the six zero cases); the fitted positives of the other
trained-regime cases score above +20, where the positive's sigmoid(-s) of 1e-9
or less puts its whole share below rtol_case.  test_ship_fused_adam and
test_ship_index_errors compare no value with ref64 and pass both builds.
"""
import math
import time

import numpy as np
import pytest
import torch

from conftest import score_tol
from knowledgegraphembedding_amd import _lib, ops
from oracle import kge_oracle as O
from ship_cases import BETAS, EPS, LR, PATTERNS, WIDE_N, Fused, is_fill, run_ship, shard_of
from test_gpu_parity import DEV
from test_slot_matrix_gpu import unaligned
from test_slot_matrix_ref import (ALL_SLOTS, CASES_B, CASES_C, CASES_D, E, MODES, NAMES, Case, inputs, ratio_of,
                                  references)

pytestmark = pytest.mark.gpu

WORST = {}       # model -> [worst ratio, where]
COVERED = set()  # (model, mode, vec, ns): the shipped step ran under W4 and met the criterion
TIMES = {}       # test id -> seconds
CASES_U = [c for c in CASES_C if not c.ent_aligned and not c.rel_aligned and c.name in ("RotatE", "DistMult")]


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.perf_counter()
    yield
    print("\nship stages: model, worst kernel ratio (where)")
    for nm in NAMES:
        if nm in WORST:
            print("ship stages: %-9s %.3f  (%s)" % (nm, *WORST[nm]))
    if TIMES:
        slow = max(TIMES, key=TIMES.get)
        print("ship stages: %d tests, %.1f s for the module; slowest %s at %.2f s" %
              (len(TIMES), time.perf_counter() - t0, slow, TIMES[slow]))


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.perf_counter()
    yield
    TIMES[request.node.name] = time.perf_counter() - t0


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def oracle_reg(inp, tr):
    """The oracle's 'regularization' in double (ref_train drops it)."""
    t = lambda a: None if a is None else torch.from_numpy(a).to(torch.float64)  # noqa: E731
    log, *_ = O.train_grads(inp.case.name, t(inp.ent), t(inp.rel), t(inp.mod), torch.from_numpy(inp.pos),
                            torch.from_numpy(inp.neg[tr.mode]), t(inp.w), tr.mode, adversarial=tr.adversarial,
                            temperature=tr.temperature, uni_weight=tr.uni_weight, regularization=tr.regularization,
                            gamma=inp.g32, erange=inp.erange)
    return log["regularization"]


def check_step(ref, tr, l64, g64, pattern, outs, fails, what):
    """The after-the-step checks 1-4 of the module docstring; True if the gradients met the criterion."""
    inp, case = ref.inp, ref.inp.case
    cuts = PATTERNS[pattern]
    # 1. gradients: the union of the owned rows is the table
    ge = torch.cat([o.grad_entity[o.lo:o.hi] for o in outs]).numpy()
    assert ge.shape == g64[0].shape
    got = [("entity", ge, g64[0]), ("relation", outs[0].grad_relation.numpy(), g64[1])]
    got += [(f"modulus@{r}", o.grad_modulus.numpy(), g64[2]) for r, o in enumerate(outs) if g64[2] is not None]
    met = True
    for nm, g, r64 in got:
        ratio = ratio_of(g, r64, ref.rtol) if np.isfinite(g).all() else math.inf
        w = WORST.setdefault(case.name, [0.0, ""])
        if ratio > w[0]:
            w[0], w[1] = ratio, f"{case.id} {pattern} {what} {nm}"
        print(f"{case.id} {pattern} {what} {nm}: rho_case {ref.rho:.3e} rtol_case {ref.rtol:.3e} ratio {ratio:.3f}")
        if not ratio <= 1.0:
            met = False
            fails.append(f"{pattern} {what} grad_{nm}: ratio {ratio:.3f} (rtol_case {ref.rtol:.3e})")
    for r, o in enumerate(outs):
        if not same(o.grad_relation, outs[0].grad_relation):
            fails.append(f"{pattern} {what}: rank {r} holds another grad_relation sum")
        if not is_fill(torch.cat([o.grad_entity[:o.lo], o.grad_entity[o.hi:]])):
            fails.append(f"{pattern} {what}: rank {r} wrote grad_entity rows outside [{o.lo}, {o.hi})")
    # 2. losses
    reg = torch.zeros((), dtype=torch.float32)
    for o in outs:
        reg = reg + o.losses[3]
    reg = float(reg)
    for r, o in enumerate(outs):
        ls = o.losses.numpy()
        k = 3 if tr.regularization == 0.0 else 2
        if not (np.isfinite(ls[:4]).all() and np.all(np.abs(ls[:k] - l64[:k]) <= score_tol(l64[:k]))):
            fails.append(f"{pattern} {what} rank {r} losses {ls[:4]} vs {l64}")
        if ls[4] != 0.0:
            fails.append(f"{pattern} {what} rank {r} losses[4] {ls[4]}")
    if tr.regularization != 0.0:
        reg64 = oracle_reg(inp, tr)
        if not abs(reg - reg64) <= score_tol(reg64):
            fails.append(f"{pattern} {what} regularization {reg} vs {reg64}")
    else:
        if any(float(o.losses[3]) != 0.0 for o in outs):
            fails.append(f"{pattern} {what}: losses[3] non-zero without a regulariser")
    l0, l1 = np.float32(outs[0].losses[0]), np.float32(outs[0].losses[1])
    loss = float((l0 + l1) / np.float32(2) + np.float32(reg))
    if not abs(loss - l64[2]) <= score_tol(l64[2]):
        fails.append(f"{pattern} {what} loss {loss} vs {l64[2]}")
    # 3. the same bits on every rank
    for r, o in enumerate(outs[1:], 1):
        if not same(o.row_stats, outs[0].row_stats):
            fails.append(f"{pattern} {what}: row_stats of rank {r} differ from rank 0's after CHAIN")
        if not same(o.losses[:2], outs[0].losses[:2]):
            fails.append(f"{pattern} {what}: losses[0:2] of rank {r} differ from rank 0's")
        if o.grad_modulus is not None and not same(o.grad_modulus, outs[0].grad_modulus):
            fails.append(f"{pattern} {what}: grad_modulus of rank {r} differs from rank 0's")
    if not np.isfinite(outs[0].row_stats.numpy()).all():
        fails.append(f"{pattern} {what}: row_stats not finite")
    # 4. g after MERGE, wherever the rank owns the negative
    own = shard_of(cuts, inp.neg[tr.mode])
    for r, o in enumerate(outs):
        if not np.isfinite(o.g_merge.numpy()[own == r]).all():
            fails.append(f"{pattern} {what}: g of rank {r} not finite at a negative it owns")
    return met


def where(tr):
    return f"{tr.mode} adv={tr.adversarial} T={tr.temperature} uni={tr.uni_weight}"


def run_case(case, patterns, *, place=None):
    ref = references(case)
    inp = ref.inp
    fails = []
    for pattern in patterns:
        for tr, (l64, g64) in zip(inp.trains, ref.train):
            outs = run_ship(inp, tr, PATTERNS[pattern], place=place, dev=DEV)
            met = check_step(ref, tr, l64, g64, pattern, outs, fails, where(tr))
            if met and pattern == "W4" and case in CASES_B:
                COVERED.add((case.name, tr.mode) + case.slots)
    assert not fails, "\n".join([case.id + f" (vec, ns) = {case.slots}"] + fails)


@pytest.mark.parametrize("case", CASES_B, ids=lambda c: c.id)
def test_ship_stages(case):
    run_case(case, ("W4", "W3"))


@pytest.mark.parametrize("case", WIDE_N, ids=lambda c: c.id)
def test_ship_wide_negatives(case):
    run_case(case, ("W4",))


@pytest.mark.parametrize("case", CASES_D, ids=lambda c: c.id)
def test_ship_trained_regime(case):
    run_case(case, ("W2", "W4", "W1"))


@pytest.mark.parametrize("case", CASES_U, ids=lambda c: c.id)
def test_ship_unaligned_tables(case):
    """Tables 4 bytes past a 16-byte boundary (single-float slots with every lane full): an
    arena's phase is a multiple of 16, so these tables are test_slot_matrix_gpu.unaligned's and
    only the values are checked for them."""
    run_case(case, ("W4",), place=lambda t: unaligned(t.to(DEV)))


def test_zz_every_shipped_instantiation_ran():
    """The shipped step of every model ran under W4, and met the criterion, in both modes at all
    ten (vec, ns) pairs.  (After test_ship_stages in file order; a B case that has not run in this
    session, say under -k, runs here.)"""
    for case in CASES_B:
        if any((case.name, mode) + case.slots not in COVERED for mode in MODES):
            run_case(case, ("W4",))
    for nm in NAMES:
        for mode in MODES:
            got = {(v, s) for (n_, m_, v, s) in COVERED if n_ == nm and m_ == mode}
            assert got == ALL_SLOTS, (nm, mode, sorted(ALL_SLOTS - got))


# ------------------------------------------------------------------ fused Adam
def _adam_rows(p, g, m, v, step):
    """ops.adam_step on device copies of host rows; returns the updated (p, m, v) on the host."""
    p, g, m, v = (t.clone().contiguous().to(DEV) for t in (p, g, m, v))
    ops.adam_step(p, g, m, v, step=step, lr=LR, beta1=BETAS[0], beta2=BETAS[1], eps=EPS)
    return p.cpu(), m.cpu(), v.cpu()


@pytest.mark.parametrize("case", CASES_B, ids=lambda c: c.id)
def test_ship_fused_adam(case):
    inp = inputs(case)
    tr = inp.trains[-1]
    cuts = PATTERNS["W4"]
    rng = np.random.default_rng(1000 + CASES_B.index(case))
    fu = dict(m0=(1e-3 * rng.standard_normal(inp.ent.shape)).astype(np.float32),
              v0=(1e-6 * rng.random(inp.ent.shape) + 1e-9).astype(np.float32))
    if inp.mod is not None:
        fu.update(mod_m0=np.array([[2e-3]], dtype=np.float32), mod_v0=np.array([[3e-6]], dtype=np.float32))
    plain = run_ship(inp, tr, cuts, dev=DEV)
    fused = run_ship(inp, tr, cuts, fused=Fused(write_grad=1, **fu), dev=DEV)
    quiet = run_ship(inp, tr, cuts, fused=Fused(write_grad=0, **fu), dev=DEV)
    ent, m0, v0 = (torch.from_numpy(a) for a in (inp.ent, fu["m0"], fu["v0"]))
    fails = []
    for r, (a, f, q) in enumerate(zip(plain, fused, quiet)):
        lo, hi = a.lo, a.hi
        assert (f.lo, f.hi, q.lo, q.hi) == (lo, hi, lo, hi)
        if not same(f.grad_entity, a.grad_entity):
            fails.append(f"rank {r}: grad_entity differs between adam == NULL and write_grad = 1")
        if not same(f.grad_relation, a.grad_relation) or not same(q.grad_relation, a.grad_relation):
            fails.append(f"rank {r}: grad_relation differs between the runs")
        if not is_fill(q.grad_entity):
            fails.append(f"rank {r}: write_grad = 0 wrote grad_entity")
        if not same(a.table[lo:hi], ent[lo:hi]):
            fails.append(f"rank {r}: adam == NULL changed the table")
        for o, nm in ((f, "write_grad = 1"), (q, "write_grad = 0")):
            outside = [torch.cat([t[:lo], t[hi:]]) for t in (o.table, o.moments["entity.m"], o.moments["entity.v"])]
            if not all(is_fill(t) for t in outside):
                fails.append(f"rank {r} {nm}: rows outside [{lo}, {hi}) of the table or the moments written")
            if hi > lo:
                want = _adam_rows(ent[lo:hi], a.grad_entity[lo:hi], m0[lo:hi], v0[lo:hi], 3)
                got = (o.table[lo:hi], o.moments["entity.m"][lo:hi], o.moments["entity.v"][lo:hi])
                for g_, w_, k in zip(got, want, ("param", "exp_avg", "exp_avg_sq")):
                    if not same(g_, w_):
                        fails.append(f"rank {r} {nm}: {k} rows differ from ops.adam_step on the gradient rows")
            if inp.mod is not None:
                want = _adam_rows(torch.from_numpy(inp.mod), a.grad_modulus, torch.from_numpy(fu["mod_m0"]),
                                  torch.from_numpy(fu["mod_v0"]), 3)
                got = (o.modulus, o.moments["modulus.m"], o.moments["modulus.v"])
                for g_, w_, k in zip(got, want, ("modulus", "its exp_avg", "its exp_avg_sq")):
                    if not same(g_, w_):
                        fails.append(f"rank {r} {nm}: {k} differs from ops.adam_step on grad_modulus")
                if not same(o.grad_modulus, a.grad_modulus):
                    fails.append(f"rank {r} {nm}: grad_modulus differs from the adam == NULL run's")
    if inp.mod is not None:
        for o in fused[1:]:
            if not (same(o.modulus, fused[0].modulus) and same(o.moments["modulus.m"], fused[0].moments["modulus.m"])
                    and same(o.moments["modulus.v"], fused[0].moments["modulus.v"])):
                fails.append("the modulus or its moments differ across ranks")
    assert not fails, "\n".join([case.id + f" {where(tr)}"] + fails)


# ---------------------------------------------------------------- index errors
@pytest.mark.parametrize("which", ["positive", "negative"])
@pytest.mark.parametrize("bad", [E, -1], ids=["E", "minus1"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["TransE", "ComplEx"])
def test_ship_index_errors(name, mode, bad, which):
    """The documented error path: rows are skipped, nothing is clamped.  Every stage returns
    KGE_OK, KGE_DEVERR_INDEX is set on every rank after the step (k_ship_q and the shipped k_row
    flag an id outside [0, E) whoever owns what), and run_ship's per-stage checks hold: no band
    and no row outside [lo, hi) written.  Values are not compared: the single-process path scores
    entity 0 in place of a bad negative and the shipped path skips it.  At span 64 (rows of 256
    and 512 bytes) even a dereference of row E or -1 would land inside a 64 KiB band."""
    inp = inputs(Case("B", name, 64))
    tr = next(t for t in inp.trains if t.mode == mode)
    pos, neg = inp.pos.copy(), inp.neg[mode].copy()
    if which == "positive":
        pos[2, 0] = bad
    else:
        neg[1, 3] = bad
    outs = run_ship(inp, tr, PATTERNS["W4"], pos=pos, neg=neg, err_ok=True, dev=DEV)
    for r, o in enumerate(outs):
        assert o.err & _lib.DEVERR_INDEX, (r, o.err)
        assert is_fill(torch.cat([o.grad_entity[:o.lo], o.grad_entity[o.hi:]])), r
