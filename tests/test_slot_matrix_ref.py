"""The slot matrix's case table, its fp64 reference and its per-row criterion,
and the CPU check that the criterion can be met by correct fp32 arithmetic.

tests/test_slot_matrix_gpu.py runs the HIP kernels on the cases built here;
this module needs no GPU.  Three groups of cases (E = 40, R = 3, B = 5, n = 7
unless a case says otherwise):

  B  every (vec, ns) row-slot instantiation, at its lower edge
     (S = 32·ns + 1 slots: load_row's "slots below NS/2 are never partial" is
     tight there) and its upper edge (S = 64·ns: every lane full), for all
     five models, with tables at the init range and gamma 9 (float4 spans
     132, 260, 516 have 33, 65, 129 slots: 260 and 516 are the lower edges of
     ns = 2 and 4, 132 lies inside ns = 1, and 1028 = 4·257 is the lower edge
     of ns = 8; test_case_table_covers_every_instantiation asserts the edges);
  C  spans that are multiples of 4 in tables whose base address is 4 bytes
     past a 16-byte boundary: single-float slots with every lane full;
  D  trained-regime inputs at spans 64 and 63: every positive fitted (its
     candidate-side row is the model's exact solution for the other two),
     tables scaled so that the adversarial softmax is peaked (spread of T·s
     over a row's negatives in [30, 80]) or both log_sigmoid branches
     saturate (positive scores > +20, worst negative < -40), elements of
     exactly zero distance, and n = 2, 3, 5 negatives (empty and uneven waves
     in k_row's four-wave merge).

Reference: the oracle on double copies of the same fp32 tables (ref64).
Criterion, per gradient tensor and row r:

    max|got[r] - ref64[r]| <= rtol_case · max|ref64[r]| + 1e-20 · max|ref64|

with rtol_case = max(8·rho_case, 32·2^-24), rho_case the worst per-row
relative distance of the fp32 oracle from ref64 on the same case (rows above
the floor).  The factor 8 covers another summation order, v_rsq / v_rcp at
about one ulp and the device's expf / sincosf in place of ATen's.  Every case
must have rho_case <= 5e-5 (asserted here; a case that breaks it gets another
seed or scale, the cap stays).  Scores and losses: |Δ| <= score_tol(ref64).
"""
import ctypes as C
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import pytest
import torch

from conftest import score_tol, synth_tables
from knowledgegraphembedding_amd import synth
from oracle import kge_oracle as O

NAMES = ["TransE", "DistMult", "ComplEx", "RotatE", "pRotatE"]
MODES = ("head-batch", "tail-batch")
E, R, B, N = 40, 3, 5, 7
RHO_CAP = 5e-5
RTOL_MIN = 32 * 2.0 ** -24
FLOOR = 1e-20

V4_SPANS = [4, 132, 256, 260, 512, 516, 1024, 1028, 2048]
V1_SPANS = [9, 63, 65, 127, 129, 255, 257, 511, 513, 1023, 1025, 2047]
UNALIGNED_SPANS = [64, 128, 256, 512, 1024, 2048]
ALL_SLOTS = {(4, 1), (4, 2), (4, 4), (4, 8), (1, 1), (1, 2), (1, 4), (1, 8), (1, 16), (1, 32)}


def expected_slots(span, ent_aligned=True, rel_aligned=True):
    """check_model's rule: float4 slots iff span % 4 == 0 and both bases are 16-byte aligned;
    ns the smallest power of two with 64·ns slots >= the row's."""
    vec = 4 if (span % 4 == 0 and ent_aligned and rel_aligned) else 1
    ns = 1
    while 64 * ns < span // vec:
        ns *= 2
    return vec, ns


@dataclass(frozen=True)
class Case:
    sec: str          # "B", "C", "D"
    name: str
    span: int
    kind: str = "init"    # init | peaked | saturated | zero | uneven
    ent_aligned: bool = True
    rel_aligned: bool = True
    n: int = N

    @property
    def id(self):
        al = "" if self.sec != "C" else "-e%dr%d" % (self.ent_aligned, self.rel_aligned)
        return f"{self.sec}-{self.name}-{self.span}-{self.kind}{al}" + (f"-n{self.n}" if self.n != N else "")

    @property
    def slots(self):
        return expected_slots(self.span, self.ent_aligned, self.rel_aligned)


CASES_B = [Case("B", nm, s) for nm in NAMES for s in V4_SPANS + V1_SPANS]
CASES_C = [Case("C", nm, s, ent_aligned=False, rel_aligned=False) for nm in NAMES for s in UNALIGNED_SPANS] + \
          [Case("C", nm, 256, ent_aligned=ea, rel_aligned=not ea) for nm in ("RotatE", "DistMult") for ea in (True, False)]
CASES_D = [Case("D", nm, s, kind) for nm in NAMES for s in (64, 63) for kind in ("peaked", "saturated")] + \
          [Case("D", nm, s, "zero") for nm in ("TransE", "RotatE", "pRotatE") for s in (64, 63)] + \
          [Case("D", "RotatE", 64, "uneven", n=n) for n in (2, 3, 5)]
CASES = CASES_B + CASES_C + CASES_D


# ------------------------------------------------------------------ inputs
@dataclass
class Train:
    mode: str
    adversarial: bool
    temperature: float
    uni_weight: bool
    regularization: float


@dataclass
class Inputs:
    case: Case
    gamma: float      # the Python float KGEModel is built with
    g32: float        # its fp32 value as a Python float (what the model's math reads)
    erange: float
    ent: np.ndarray
    rel: np.ndarray
    mod: np.ndarray   # [1, 1] or None
    pos: np.ndarray
    neg: dict         # mode -> [B, n]
    w: np.ndarray
    trains: list
    gout: dict        # mode -> upstream gradient of forward() ('single' included)


def _seed(case):
    return 100 + NAMES.index(case.name) * 17 + case.span % 97


def _with_duplicates(pos, neg, mode):
    """One negative per row is the row's positive entity on the candidate side, another the
    q-side entity: duplicates within an occurrence bucket and a negative equal to the positive."""
    cand, qside = (0, 2) if mode == "head-batch" else (2, 0)
    out = neg.copy()
    n = out.shape[1]
    for i in range(out.shape[0]):
        out[i, i % n] = pos[i, cand]
        if n > 1:
            out[i, (i + 3) % n if (i + 3) % n != i % n else (i + 1) % n] = pos[i, qside]
    return out


def true_column(n):
    """Trained regime: the column of each row's negatives that holds the positive's true entity.
    k_row's wave w takes negatives w, w + 4, …: in columns 4 … n - 1 the true entity comes second
    in its wave, so the wave's running maximum rises by the whole spread there and its V, Z, NL, MG
    are rescaled by exp(-spread) (first in its wave it would never be).  n < 5: one negative per
    wave, the last column."""
    i = np.arange(B)
    return n - 1 - (i % 3 if n >= 7 else 0)


def _fit_rows(name, ent, rel, pos, erange, target, noise):
    """Trained regime: entity row t_i becomes the model's solution for (h_i, r_i) — zero
    distance (TransE, RotatE, pRotatE), or the direction of h∘r scaled to score `target`
    (DistMult, ComplEx) — computed in double, plus the uniform `noise` [B, Le] (a fit without it
    leaves elements at the rounding level, whose sign no fp32 evaluation can tell: rho ~ 1)."""
    ent = ent.copy()
    e64, r64 = ent.astype(np.float64), rel.astype(np.float64)
    for i, (h, r, t) in enumerate(pos.tolist()):
        if name in ("TransE", "pRotatE"):
            row = e64[h] + r64[r]
        elif name == "DistMult":
            hr = e64[h] * r64[r]
            row = hr * (target / np.sum(hr * hr))
        else:
            d = ent.shape[1] // 2
            hre, him = e64[h, :d], e64[h, d:]
            if name == "RotatE":
                ph = r64[r] / (erange / O.PI)
                rre, rim = np.cos(ph), np.sin(ph)
            else:
                rre, rim = r64[r, :d], r64[r, d:]
            a, b = hre * rre - him * rim, hre * rim + him * rre
            row = np.concatenate([a, b])
            if name == "ComplEx":
                row = row * (target / np.sum(row * row))
        ent[t] = (row + noise[i]).astype(np.float32)
    return ent


# (gamma, entity scale, relation scale, modulus, T, target) per model: measured on the CPU with
# the oracle in double so that the conditions test_trained_regime_conditions asserts hold.
# Peaked, distance models: gamma 24 puts the other negatives' scores near 0 (a fitted positive
# scores ~23.5, they 15 … 40 lower), where sigmoid(s) is of order 1: what a wave accumulated before
# its maximum rose then weighs as much as the dominant negative's term unless it is rescaled (at
# gamma 12 their sigmoid(s) ~ 1e-6 hid a missing rescale below RotatE's rtol_case).
PEAKED = {"TransE": (24.0, 1.35, 1.35, None, 2.0, 0.0), "RotatE": (24.0, 0.86, 1.0, None, 2.0, 0.0),
          "pRotatE": (24.0, 1.0, 1.0, 0.55, 2.0, 0.0), "DistMult": (12.0, 5.0, 5.0, None, 4.0, 12.0),
          "ComplEx": (12.0, 4.0, 4.0, None, 4.0, 12.0)}
SATURATED = {"TransE": (24.0, 5.0, 5.0, None, 0.5, 0.0), "RotatE": (24.0, 2.6, 1.0, None, 0.5, 0.0),
             "pRotatE": (24.0, 1.0, 1.0, 2.0, 0.5, 0.0), "DistMult": (24.0, 4.0, 4.0, None, 0.5, 22.0),
             "ComplEx": (24.0, 4.0, 4.0, None, 0.5, 22.0)}


@lru_cache(maxsize=4)
def inputs(case: Case) -> Inputs:
    name, span, n = case.name, case.span, case.n
    seed = _seed(case)
    reg = 1e-4 if name in ("DistMult", "ComplEx") else 0.0
    pos, neg, w = synth.kge_batch(seed + 1, B, n, E, R)
    # no triple with h = t: pRotatE's 'single' score of (e, r, e) does not depend on e, so that
    # entity's gradient row is an exact cancellation of two rounded terms — no bound relative to
    # the row's own maximum can hold there (measured: a residue of 1.5e-7 of the table maximum,
    # one ulp of either term; test_edge_gpu's two-entity graph keeps such triples)
    loops = pos[:, 0] == pos[:, 2]
    pos[loops, 2] = (pos[loops, 2] + 1) % E
    if case.kind in ("init", "zero"):
        gamma = 9.0
        ent, rel, mod, erange = synth_tables(name, E, R, span, gamma, seed)
        trains = [Train(m, True, 0.75, False, reg) for m in MODES]
        if case.kind == "zero":
            # relation 0 is the identity (TransE / pRotatE r = 0, RotatE phase 0); rows 1 and 3 use
            # it, and their first negative is their own q-side entity: elements of exactly zero distance
            rel = rel.copy()
            rel[0] = 0.0
            pos[[1, 3], 1] = 0
    else:
        gamma, se, sr, modulus, T, target = (SATURATED if case.kind == "saturated" else PEAKED)[name]
        ent, rel, mod, erange = synth_tables(name, E, R, span, gamma, seed)
        ent = ent * np.float32(se)
        rel = rel * np.float32(sr) if name != "RotatE" else rel
        if mod is not None:
            mod = np.array([[modulus]], dtype=np.float32)
        # heads 0-4, tails 10-14 (fitted), their opposites 5-9 and 15-19, random negatives from 20 on:
        # fitting a row disturbs no other triple
        pos = np.stack([np.arange(B), np.arange(B) % R, 10 + np.arange(B)], 1).astype(np.int64)
        neg = 20 + neg % (E - 20)
        amp = (0.01 if name == "pRotatE" else 0.03 * se) * erange  # (pRotatE: 0.03 rad of phase)
        if name in ("DistMult", "ComplEx"):
            amp = 0.0  # the fit is a direction, not a zero: nothing sits at the rounding level
        noise = synth.uniform(seed + 50, (B, ent.shape[1]), -1.0, 1.0).astype(np.float64) * amp
        ent = _fit_rows(name, ent, rel, pos, erange, target, noise)
        if case.kind == "saturated" and name in ("DistMult", "ComplEx"):
            # negatives that score -2.2 × the positive, one for either candidate side
            ent[15:15 + B] = -2.2 * ent[pos[:, 2]]
            ent[5:5 + B] = -2.2 * ent[pos[:, 0]]
        if case.kind == "saturated":
            trains = [Train(m, adv, T, False, reg) for m in MODES for adv in (False, True)]
        elif case.kind == "uneven":
            trains = [Train("tail-batch", True, T, False, reg)]
        else:
            trains = [Train(m, adv, T, uni, reg) for m in MODES for adv, uni in ((True, False), (False, False),
                                                                                 (True, True))]
    negs = {}
    for mode in MODES:
        nm = _with_duplicates(pos, neg, mode) if case.kind in ("init", "zero") else neg.copy()
        if case.kind == "zero":
            nm[[1, 3], 0] = pos[[1, 3], 2 if mode == "head-batch" else 0]
        elif case.kind != "init":
            # head-batch fits are on the tail row too (the score of (h, r, t) is the same in both
            # modes), so the candidate-side true entity carries almost all the softmax weight
            nm[np.arange(B), true_column(n)] = pos[:, 0 if mode == "head-batch" else 2]
            if case.kind == "saturated" and name in ("DistMult", "ComplEx"):
                nm[:, 1] = (5 if mode == "head-batch" else 15) + np.arange(B)
        negs[mode] = nm
    gout = {m: synth.uniform(seed + 7 + k, (B, 1 if m == "single" else n), -1.0, 1.0)
            for k, m in enumerate(("single",) + MODES)}
    return Inputs(case, gamma, torch.Tensor([gamma]).item(), erange, ent, rel, mod, pos, negs, w, trains, gout)


# --------------------------------------------------------------- references
def _tables(inp, dtype):
    t = lambda a: None if a is None else torch.from_numpy(a).to(dtype)  # noqa: E731
    return t(inp.ent), t(inp.rel), t(inp.mod)


def ref_forward(inp, mode, dtype):
    ent, rel, mod = _tables(inp, dtype)
    P = torch.from_numpy(inp.pos)
    sample = P if mode == "single" else (P, torch.from_numpy(inp.neg[mode]))
    return O.forward(inp.case.name, ent, rel, mod, sample, mode, inp.g32, inp.erange).numpy()


def ref_backward(inp, mode, dtype):
    """(scores, grad_entity, grad_relation, grad_modulus) of forward() under the upstream gradient gout."""
    ent, rel, mod = (None if t is None else t.requires_grad_(True) for t in _tables(inp, dtype))
    P = torch.from_numpy(inp.pos)
    sample = P if mode == "single" else (P, torch.from_numpy(inp.neg[mode]))
    s = O.forward(inp.case.name, ent, rel, mod, sample, mode, inp.g32, inp.erange)
    s.backward(torch.from_numpy(inp.gout[mode]).to(dtype))
    return s.detach().numpy(), [ent.grad.numpy(), rel.grad.numpy(), None if mod is None else mod.grad.numpy()]


def ref_train(inp, tr, dtype):
    """(the three losses, [grad_entity, grad_relation, grad_modulus])."""
    ent, rel, mod = _tables(inp, dtype)
    log, ge, gr, gm = O.train_grads(inp.case.name, ent, rel, mod, torch.from_numpy(inp.pos),
                                    torch.from_numpy(inp.neg[tr.mode]), torch.from_numpy(inp.w).to(dtype), tr.mode,
                                    adversarial=tr.adversarial, temperature=tr.temperature, uni_weight=tr.uni_weight,
                                    regularization=tr.regularization, gamma=inp.g32, erange=inp.erange)
    losses = np.array([log["positive_sample_loss"], log["negative_sample_loss"], log["loss"]])
    return losses, [ge.numpy(), gr.numpy(), None if gm is None else gm.numpy()]


def _rows(a):
    a = np.asarray(a, dtype=np.float64)
    return a.reshape(a.shape[0], -1) if a.ndim > 1 else a.reshape(1, -1)


def row_distance(got, ref64):
    """Per row: (max|got - ref64|, max|ref64|), and the table's floor 1e-20 · max|ref64|."""
    g, r = _rows(got), _rows(ref64)
    rm = np.abs(r).max(axis=1)
    return np.abs(g - r).max(axis=1), rm, FLOOR * rm.max()


def rho_of(g32, g64):
    """Worst per-row relative distance of g32 from g64 over the rows above the floor."""
    err, rm, floor = row_distance(g32, g64)
    sel = rm > floor
    return float((err[sel] / rm[sel]).max()) if sel.any() else 0.0


def ratio_of(got, g64, rtol):
    """Worst err / (rtol · rowmax + floor): the criterion holds iff this is <= 1."""
    err, rm, floor = row_distance(got, g64)
    bound = rtol * rm + floor
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))


@dataclass
class Refs:
    inp: Inputs
    forward: dict     # mode -> fp64 scores
    backward: dict    # mode -> (fp64 scores, fp64 grads)
    train: list       # per inp.trains: (fp64 losses, fp64 grads)
    rho: float
    rtol: float


@lru_cache(maxsize=4)
def references(case: Case) -> Refs:
    inp = inputs(case)
    rho = 0.0
    fwd, bwd, trn = {}, {}, []
    for mode in ("single",) + MODES:
        fwd[mode] = ref_forward(inp, mode, torch.float64)
        if case.kind in ("init",):
            s64, g64 = ref_backward(inp, mode, torch.float64)
            _, g32 = ref_backward(inp, mode, torch.float32)
            bwd[mode] = (s64, g64)
            rho = max([rho] + [rho_of(a, b) for a, b in zip(g32, g64) if b is not None])
    for tr in inp.trains:
        l64, g64 = ref_train(inp, tr, torch.float64)
        _, g32 = ref_train(inp, tr, torch.float32)
        trn.append((l64, g64))
        rho = max([rho] + [rho_of(a, b) for a, b in zip(g32, g64) if b is not None])
    return Refs(inp, fwd, bwd, trn, rho, max(8.0 * rho, RTOL_MIN))


# ------------------------------------------------------------------- tests
def test_case_table_covers_every_instantiation():
    """All ten (vec, ns) instantiations, for every model (both modes run in each case), in B;
    C reaches vec = 1 with every lane full for ns = 1 … 32; each B pair at both of its edges."""
    for nm in NAMES:
        assert {c.slots for c in CASES_B if c.name == nm} == ALL_SLOTS, nm
        assert {c.slots for c in CASES_C if c.name == nm and not c.ent_aligned and not c.rel_aligned} == \
            {(1, ns) for ns in (1, 2, 4, 8, 16, 32)}, nm
        for vec, ns in ALL_SLOTS:
            S = sorted(c.span // vec for c in CASES_B if c.name == nm and c.slots == (vec, ns))
            assert S[-1] == 64 * ns or (vec == 1 and S[-1] == 64 * ns - 1), (nm, vec, ns, S)  # vec = 1: the last
            # span that is no multiple of 4; the full last slot is C's (unaligned multiples of 4)
            assert ns == 1 or S[0] == 32 * ns + 1, (nm, vec, ns, S)
    assert {c.slots for c in CASES_C if c.ent_aligned != c.rel_aligned} == {(1, 4)}
    assert len({c.id for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_criterion_is_satisfiable_in_fp32(case):
    """The fp32 oracle itself meets the criterion with room to spare: rho_case <= 5e-5, finite
    gradients, and its scores and losses within score_tol of ref64."""
    ref = references(case)
    inp = ref.inp
    assert ref.rho <= RHO_CAP, ref.rho
    for mode, s64 in ref.forward.items():
        assert np.isfinite(s64).all()
        s32 = ref_forward(inp, mode, torch.float32)
        assert np.all(np.abs(s32 - s64) <= score_tol(s64)), (mode, np.abs(s32 - s64).max())
    for tr, (l64, g64) in zip(inp.trains, ref.train):
        l32, g32 = ref_train(inp, tr, torch.float32)
        assert np.isfinite(l64).all() and np.all(np.abs(l32 - l64) <= score_tol(l64)), (tr, l32, l64)
        for a, b in zip(g32, g64):
            if b is not None:
                assert np.isfinite(a).all() and np.isfinite(b).all(), tr
                assert ratio_of(a, b, ref.rtol) <= 1.0 / 8.0 + 1e-12, tr  # (rtol_case >= 8 · rho_case)


@pytest.mark.parametrize("case", CASES_D, ids=lambda c: c.id)
def test_trained_regime_conditions(case):
    """The input conditions of D, in fp64: the spread of T·s over each row's negatives in
    [30, 80] (peaked, uneven), positives above +20 and the worst negative below -40 (saturated),
    elements of exactly zero distance whose gradient terms are zero (zero)."""
    ref = references(case)
    inp = ref.inp
    for tr, mode in ((t, t.mode) for t in inp.trains):
        s = ref.forward[mode]
        if case.kind in ("peaked", "uneven") and tr.adversarial:
            spread = tr.temperature * (s.max(axis=1) - s.min(axis=1))
            assert tr.temperature in (2.0, 4.0) and np.all((spread >= 30) & (spread <= 80)), (mode, spread)
            # the positive's true entity carries almost all the weight, and (n >= 5) is not the
            # first negative of its wave
            p = torch.softmax(torch.from_numpy(s * tr.temperature), dim=1).numpy()
            col = true_column(case.n)
            assert np.all(p[np.arange(B), col] > 0.99), p[np.arange(B), col]
            assert case.n < 5 or np.all(col >= 4)
        if case.kind == "saturated":
            assert np.all(ref.forward["single"] > 20.0), ref.forward["single"].ravel()
            assert s.min() < -40.0, s.min()
    if case.kind == "zero":
        assert not inp.rel[0].any() and np.all(inp.pos[[1, 3], 1] == 0)
        for mode in MODES:
            q = 2 if mode == "head-batch" else 0
            assert np.array_equal(inp.neg[mode][[1, 3], 0], inp.pos[[1, 3], q])
            # the score of such a negative is gamma exactly, in both precisions: every element term is zero
            for dtype in (torch.float64, torch.float32):
                assert np.all(ref_forward(inp, mode, dtype)[[1, 3], 0] == inp.g32)
        for _, g64 in ref.train:
            assert all(np.isfinite(g).all() for g in g64 if g is not None)


# ------------------------------------------------- the alignment contract
def _host_floats(n):
    """A host buffer and a 16-byte aligned address inside it (the entries below are refused on
    the host, before any launch: nothing dereferences these pointers)."""
    buf = (C.c_float * (n + 4))()
    base = C.addressof(buf)
    return buf, base + (-base) % 16


def test_fused_entries_refuse_unaligned_gradient_and_moment_buffers():
    """With float4 slots the entity and relation passes write the gradients, and stream the fused
    Adam's moments, 16 bytes at a time: kge_train_step*, kge_score_backward and the entries built
    on them return KGE_ERR_ARG for a gradient or moment buffer that is not 16-byte aligned, as
    kge_adam_step does.  The same calls with aligned buffers pass that check (they stop at the
    workspace check, KGE_ERR_WORKSPACE: nothing is launched here), and single-float slots
    (span 9) ask for no alignment."""
    from knowledgegraphembedding_amd import _lib
    ERR_ARG, ERR_WORKSPACE = 4, 5
    lib = _lib.load()
    keep = []

    def ptr(n=64):
        buf, p = _host_floats(n)
        keep.append(buf)
        return p

    def desc(span):
        d = _lib.ModelDesc()
        d.model, d.entity_dim, d.relation_dim, d.nentity, d.nrelation = 0, span, span, 4, 2  # TransE
        d.gamma, d.phase_divisor, d.phase_divisor_p = 12.0, 0.1, 0.1
        d.entity_embedding, d.relation_embedding = ptr(), ptr()
        return d

    ids, w, ge, gr, losses, ws, err = (ptr() for _ in range(7))

    def grads(d, ge_, gr_):
        return lib.kge_train_step_grads(C.byref(d), 2, ids, ids, 1, 1, w, None, 0, 0, 1, 1.0, 0.0, ge_, gr_, None,
                                        losses, ws, 0, err, None)

    def phased(d, ge_, gr_):
        return lib.kge_train_step_grads_phased(C.byref(d), 2, ids, ids, 1, 1, w, None, 0, 0, 1, 1.0, 0.0, ge_, gr_,
                                               None, losses, ws, 0, err, None, 1, 0, 4)

    def backward(d, ge_, gr_):
        return lib.kge_score_backward(C.byref(d), 2, ids, ids, 1, 1, w, ge_, gr_, None, ws, 0, err, None)

    def fused(d, shift_entity_m=0, shift_relation_v=0, ge_=None):
        a = _lib.AdamDesc()
        a.beta1, a.beta2, a.eps, a.write_grad = 0.9, 0.999, 1e-8, 1
        a.entity.param, a.relation.param = d.entity_embedding, d.relation_embedding
        a.entity.exp_avg, a.entity.exp_avg_sq = ptr() + shift_entity_m, ptr()
        a.relation.exp_avg, a.relation.exp_avg_sq = ptr(), ptr() + shift_relation_v
        return lib.kge_train_step(C.byref(d), 2, ids, ids, 1, 1, w, None, 0, 0, 1, 1.0, 0.0, C.byref(a),
                                  ge if ge_ is None else ge_, gr, None, losses, ws, 0, err, None)

    d4 = desc(8)   # float4 slots
    for call in (grads, phased, backward):
        assert call(d4, ge, gr) == ERR_WORKSPACE, call.__name__
        assert call(d4, ge + 4, gr) == ERR_ARG, call.__name__
        assert call(d4, ge, gr + 4) == ERR_ARG, call.__name__
    assert fused(d4) == ERR_WORKSPACE
    assert fused(d4, shift_entity_m=4) == ERR_ARG
    assert fused(d4, shift_relation_v=8) == ERR_ARG
    assert fused(d4, ge_=ge + 12) == ERR_ARG
    d1 = desc(9)   # single-float slots: any 4-byte aligned buffer
    for call in (grads, phased, backward):
        assert call(d1, ge + 4, gr + 4) == ERR_WORKSPACE, call.__name__
    assert fused(d1, shift_entity_m=4, shift_relation_v=4) == ERR_WORKSPACE
    # an unaligned table already selects single-float slots (check_model)
    d4.entity_embedding += 4
    assert grads(d4, ge + 4, gr + 4) == ERR_WORKSPACE
