"""Every entry point of include/kge_hip.h on exactly sized, guard-banded device
buffers (GPU box).

kge_hip.h promises that a call's scratch comes from a caller-owned workspace
"whose size the matching *_workspace_bytes() query returns", that a range call
touches only its owner's rows, that the lazy step neither reads nor writes
grad_entity, and per-query outputs of exactly [nq], [2·nq] or [nq, k].  The rest
of the suite checks values only, in torch tensors with slack behind them (the
Python mirror's workspaces are a quarter larger than asked).  Here every device
pointer a call receives is the view of its own arena (tests/arena.py): 64 KiB
of poison on either side, 0xFF in floats and workspaces, 0x7F in id arrays, the
workspace's interior exactly the queried size and left poisoned.  The calls go
through ctypes (_lib.load()), not through ops: the wrappers bring the slack.

After each call and a stream sync:
  1. the status is KGE_OK;
  2. err_flag is 0 (an id read past an index array's end is 0x7F7F…: out of range);
  3. both bands of every arena still hold their fill;
  4. every read-only buffer is byte for byte what was put in;
  5. the outputs meet the entry's existing criterion, the reference taken from
     the module that defines it (test_slot_matrix_ref's fp64 references and
     ratio_of, conftest.score_tol, oracle.filtered_ranks, rank_tie_cases,
     topk_cases.check_result, rank_candidates_cases, rank_relations_cases,
     lazy_adam_cases.lazy_adam_ref, oracle.sample_negatives, oracle.adam_steps);
  6. the outputs are bit-identical to the same call through the Python mirror
     (ops.*) on ordinary tensors at the same alignment class; losses to
     rtol = 1e-6 where the regulariser's partial sums may regroup (DistMult /
     ComplEx, as test_entity_pass_column_slices_bitwise), exact elsewhere.

Shapes: tests/arena_cases.py.  kge_ship_step has a module of its own: its five
stages need the collectives between them, which tests/test_ship_stages_gpu.py
emulates in one process on the same arenas (test_ship_gpu.py drives the real
ones through partition.py).  rank_candidates_cases and rank_relations_cases fix R = 7 / their
own R; topk's tables are built here at R = 5 and scored by
topk_cases.oracle_scores.

Recorded on an MI355X: 209 tests, 13.4 s for the module; the slowest is
test_rank_filtered[RotatE-E64-d2052-65] at 4.5 s (the CPU oracle's 2 · 65 wide
queries), every other test under 1.2 s.  All pass on the committed library: no
size query is short, no kernel reads scratch it did not write, no write leaves
its range.  Two things the tests met on the way, both in how an entry is called:
kge_train_step_grads_phased's FINALIZE sums the regulariser's entity terms over
the range it is given (kge_hip.h now says so: pass [0, nentity)), and
kge_adam_step forms 1 - beta in fp32 where torch forms it in double, so only its
parameters, not its moments, meet test_kge_adam_matches_torch_adam's bound
against torch.optim.Adam.

Sensitivity (scratch builds, not committed): per carve_* function a library
whose size query (and workspace check) reports 1 KiB less than the function lays
out — more than the 256-byte tail, far less than a band — against all 209 tests.
Every failure listed is the workspace arena's band check ("N byte(s) written
after the buffer"), before any value is compared:
    carve_rank  48 fail: all 24 test_rank_filtered, all 18 test_rank_filtered_both,
                4 test_rank_near_tie_lists, 2 test_protate_three_calls (the last
                buffer is the filter bitmap, written whole by every call)
    carve_topk  all 20 test_topk (the partial lists)
    carve_lazy  all 12 test_train_step_lazy (the compaction's scratch)
    carve_rel   the 8 RotatE cases of test_rank_relations (relation_trig NULL:
                the trig table is the last buffer, 765-768 bytes land in the
                band).  The other 18 have a layout of under 1 KiB (two int32
                counters per query): the short query wraps below zero and no
                arena can be made — they fail, but not at a band
    carve_cand  every layout here is under 1 KiB (same counters; the 2052-float
                rows are staged in LDS, not in the workspace): all 14 fail for
                that reason, none at a band.  The layout is 520 bytes of
                counters at nq = 65, rounded up to 768 by the (empty) qref
                buffer's alignment, plus the tail: a build 320 bytes short is
                still inside that slack and passes all 209; one 528 bytes short
                fails the 6 nq = 65 cases at the band (24 bytes written after
                the buffer) and the 8 smaller ones by wrapping
    carve_grad  not noticed, 0 of 209: the layout ends in q_sl (8 · B · 512
                floats for up to 8 column slices of 128 slots; RotatE at span
                280 fills 2 slices of 35) and rocPRIM's scan scratch, neither
                written to its end at these shapes.  kge_ship_step reuses this
                layout (tests/test_ship_stages_gpu.py runs it at the exact size)
One build in which the lazy entity pass ignores nrows and walks all places was
run once, guarded half only: it ended in a GPU memory fault on its first case
(TransE E = 257, (B, n) = (5, 65)) instead of a failed unchanged() — a place
past the list takes the poisoned list entry for a row id and the bucket walk
that follows reads poisoned offsets.  It was not run again, so the untouched-row
check has no recorded GPU sensitivity run.  What it would see is shown by
arithmetic instead (test_train_step_lazy): untouched rows carry non-zero
moments, so a visit of one with its empty bucket's zero gradient scales m by
beta1 and v by beta2 and moves p — bytes that the comparison with the host copy
catches; the test asserts that this update differs from the input in m, v and p.
"""
import ctypes as C
import math
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import arena_cases as A
import lazy_adam_cases as L
import rank_candidates_cases as RC
import rank_relations_cases as RR
import rank_tie_cases as T
import test_slot_matrix_ref as S
import topk_cases as K
from arena import FLOAT_FILL, arena, arena_of
from conftest import score_tol, synth_tables
from knowledgegraphembedding_amd import _lib, ops, synth
from knowledgegraphembedding_amd.filters import FilterIndex
from knowledgegraphembedding_amd.sampler import TrueLists, batch_key
from oracle import kge_oracle as O
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

MODES = A.MODES
B = A.B
LR = 3e-3
BETAS, EPS = (0.9, 0.999), 1e-8
F32, I64, I32, U8 = torch.float32, torch.int64, torch.int32, torch.uint8


def lib():
    return _lib.load()


def ok(status, what):
    assert status == 0, f"{what}: status {status} ({lib().kge_status_string(status).decode()})"


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == F32 else t


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def host(x):
    return x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x))  # (a copy: the cases' arrays are read-only)


class Bufs:
    """The buffers of one run.  guarded: every buffer an arena, the workspace exactly the asked
    size, an err_flag of its own.  Not guarded (the mirror run): ordinary tensors at the same
    16-byte phase, the mirror's own workspace and error flag."""

    def __init__(self, guarded):
        self.guarded = guarded
        self.arenas = {}
        self.ro = []
        self.keep = []
        self._err = None

    def _plain(self, shape, dtype, phase):
        n = math.prod(shape)
        es = torch.empty((), dtype=dtype).element_size()
        raw = torch.full((phase + n * es,), FLOAT_FILL, dtype=U8, device=DEV)
        assert raw.data_ptr() % 256 == 0
        v = raw[phase:phase + n * es].view(dtype).view(shape)
        self.keep.append(raw)
        return v

    def inp(self, name, src, *, ro=True, phase=0, fill=None):
        src = host(src)
        if not self.guarded:
            v = self._plain(tuple(src.shape), src.dtype, phase)
            v.copy_(src)
            return v
        assert name not in self.arenas, name
        a = self.arenas[name] = arena_of(src, DEV, phase=phase, fill=fill, name=name)
        if ro:
            self.ro.append((a, src.clone()))
        return a.view

    def out(self, name, shape, dtype, *, phase=0, fill=None):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        if not self.guarded:
            return self._plain(shape, dtype, phase)
        assert name not in self.arenas, name
        a = self.arenas[name] = arena(shape, dtype, DEV, phase=phase, fill=fill, name=name)
        return a.view

    def ws(self, nbytes, name="workspace"):
        """(pointer, workspace_bytes): guarded, an arena of exactly nbytes left at its fill."""
        nbytes = int(nbytes)
        if not self.guarded:
            t = ops.state(DEV).workspace(nbytes)
            return t.data_ptr(), t.numel()
        if name in self.arenas:
            assert self.arenas[name].nbytes == nbytes
        else:
            self.arenas[name] = arena(nbytes, U8, DEV, name=name)
        return self.arenas[name].ptr(), nbytes

    def err(self):
        if not self.guarded:
            return ops.state(DEV).err.data_ptr()
        if self._err is None:
            self._err = self.inp("err_flag", torch.zeros(1, dtype=I32), ro=False)
        return self._err.data_ptr()

    def verify(self, what=""):
        torch.cuda.synchronize(DEV)
        if not self.guarded:
            ops.raise_on_device_error(DEV)
            return
        if self._err is not None:
            assert int(self._err.item()) == 0, f"{what}: err_flag {int(self._err.item())}"
        for a in self.arenas.values():
            a.check()
        for a, h in self.ro:
            a.unchanged(h)


def stream():
    return ops._stream(DEV)


@lru_cache(maxsize=None)
def tables(shape):
    ent, rel, mod, erange = synth_tables(shape.name, shape.E, shape.R, shape.d, A.GAMMA, shape.seed)
    for x in (ent, rel):
        x.setflags(write=False)
    return ent, rel, mod, erange


def model(b, tab, name, *, ro=True, phase=0, trig=False):
    """The tables of `tab` = (ent, rel, mod, erange) in buffers of `b` and their descriptor."""
    ent, rel, mod, erange = tab
    e = b.inp("entity", ent, ro=ro, phase=phase)
    r = b.inp("relation", rel, ro=ro)
    m = None if mod is None else b.inp("modulus", mod, ro=ro)
    d = ops.make_desc(name, e, r, A.GAMMA, erange, m)
    t = None
    if trig:
        t = b.inp("relation_trig", ops.reference_rotation(torch.from_numpy(np.array(rel)), erange))
        d.relation_trig = t.data_ptr()
    return SimpleNamespace(desc=d, e=e, r=r, m=m, trig=t, name=name)


# ------------------------------------------------- scores, backward, train
@lru_cache(maxsize=None)
def batch(shape, n):
    """test_slot_matrix_ref's Inputs at this module's shapes (its own batch recipe: duplicates
    within a bucket, a negative equal to the positive, no h = t loop)."""
    ent, rel, mod, erange = tables(shape)
    seed = shape.seed
    pos, neg, w = synth.kge_batch(seed + 1, B, n, shape.E, shape.R)
    loops = pos[:, 0] == pos[:, 2]
    pos[loops, 2] = (pos[loops, 2] + 1) % shape.E
    reg = 1e-4 if shape.name in ("DistMult", "ComplEx") else 0.0
    trains = [S.Train(m, True, 0.75, False, reg) for m in MODES]
    negs = {m: S._with_duplicates(pos, neg, m) for m in MODES}
    gout = {m: synth.uniform(seed + 7 + k, (B, 1 if m == "single" else n), -1.0, 1.0)
            for k, m in enumerate(("single",) + MODES)}
    case = S.Case("B", shape.name, shape.d, n=n)
    return S.Inputs(case, A.GAMMA, torch.Tensor([A.GAMMA]).item(), erange, np.array(ent), np.array(rel), mod, pos,
                    negs, w, trains, gout)


@lru_cache(maxsize=None)
def refs(shape, n):
    """test_slot_matrix_ref.references on batch(shape, n): fp64 scores, gradients and losses,
    rho_case and rtol_case = max(8 · rho_case, 32 · 2^-24)."""
    inp = batch(shape, n)
    rho, fwd, bwd, trn = 0.0, {}, {}, []
    for mode in ("single",) + MODES:
        fwd[mode] = S.ref_forward(inp, mode, torch.float64)
        s64, g64 = S.ref_backward(inp, mode, torch.float64)
        _, g32 = S.ref_backward(inp, mode, torch.float32)
        bwd[mode] = (s64, g64)
        rho = max([rho] + [S.rho_of(a, c) for a, c in zip(g32, g64) if c is not None])
    for tr in inp.trains:
        l64, g64 = S.ref_train(inp, tr, torch.float64)
        _, g32 = S.ref_train(inp, tr, torch.float32)
        trn.append((l64, g64))
        rho = max([rho] + [S.rho_of(a, c) for a, c in zip(g32, g64) if c is not None])
    assert rho <= S.RHO_CAP, rho
    return S.Refs(inp, fwd, bwd, trn, rho, max(8.0 * rho, S.RTOL_MIN))


def n_of(shape):
    return (3,) if shape.d == A.WIDE else A.NNEG


def check_grads(got, g64, ref, what):
    for g, r, nm in zip(got, g64, ("entity", "relation", "modulus")):
        if r is None:
            continue
        g = g.detach().cpu().numpy()
        ratio = S.ratio_of(g, r, ref.rtol) if np.isfinite(g).all() else math.inf
        print(f"{what} grad_{nm}: rtol_case {ref.rtol:.3e} ratio {ratio:.3f}")
        assert ratio <= 1.0, f"{what} grad_{nm}: ratio {ratio:.3f} (rtol_case {ref.rtol:.3e})"


def same_losses(a, b, reg, what):
    """Losses of the guarded run against the mirror's: exact; with a regulariser, whose partial
    sums may regroup, to rtol = 1e-6 (test_entity_pass_column_slices_bitwise's bound)."""
    a, b = a.detach().cpu()[:4], b.detach().cpu()[:4]
    if reg:
        torch.testing.assert_close(a, b, rtol=1e-6, atol=0, msg=lambda m: f"{what}: {m}")
    else:
        assert same(a, b), (what, a, b)


SCORE_SHAPES = A.SMALL + A.WIDE_SHAPES


@pytest.mark.parametrize("shape", SCORE_SHAPES, ids=lambda s: s.id)
def test_score(shape):
    for n in n_of(shape):
        ref = refs(shape, n)
        inp = ref.inp
        for mode in ("single",) + MODES:
            nn = 1 if mode == "single" else n

            def run(guarded):
                b = Bufs(guarded)
                m = model(b, tables(shape), shape.name)
                pos = b.inp("pos", inp.pos)
                neg = None if mode == "single" else b.inp("neg", inp.neg[mode])
                if not guarded:
                    out = ops.score(m.desc, mode, pos, neg, DEV)
                else:
                    out = b.out("out", (B, nn), F32)
                    ok(lib().kge_score(m.desc, _lib.MODE_IDS[mode], pos.data_ptr(), ops._ptr(neg), B, nn,
                                       out.data_ptr(), b.err(), stream()), "kge_score")
                b.verify(f"score {mode}")
                return out.cpu()

            got, mirror = run(True), run(False)
            s64 = ref.forward[mode]
            assert np.all(np.abs(got.numpy() - s64) <= score_tol(s64)), (shape.id, mode, n)
            assert same(got, mirror), (shape.id, mode, n)


@pytest.mark.parametrize("shape", SCORE_SHAPES, ids=lambda s: s.id)
def test_score_backward(shape):
    for n in n_of(shape):
        ref = refs(shape, n)
        inp = ref.inp
        for mode in ("single",) + MODES:
            nn = 1 if mode == "single" else n
            what = f"{shape.id} backward {mode} n{nn}"

            def run(guarded):
                b = Bufs(guarded)
                m = model(b, tables(shape), shape.name)
                pos = b.inp("pos", inp.pos)
                neg = None if mode == "single" else b.inp("neg", inp.neg[mode])
                gs = b.inp("grad_scores", inp.gout[mode])
                if not guarded:
                    out = ops.score_backward(m.desc, mode, pos, neg, gs, DEV, m.m is not None)
                else:
                    ge = b.out("grad_entity", (shape.E, shape.le), F32)
                    gr = b.out("grad_relation", (shape.R, shape.lr), F32)
                    gm = b.out("grad_modulus", (1, 1), F32) if m.m is not None else None
                    mid = _lib.MODE_IDS[mode]
                    wp, wn = b.ws(lib().kge_backward_workspace_bytes(m.desc, mid, B, nn))
                    ok(lib().kge_score_backward(m.desc, mid, pos.data_ptr(), ops._ptr(neg), B, nn, gs.data_ptr(),
                                                ge.data_ptr(), gr.data_ptr(), ops._ptr(gm), wp, wn, b.err(),
                                                stream()), what)
                    out = (ge, gr, gm)
                b.verify(what)
                return [None if t is None else t.cpu() for t in out]

            got, mirror = run(True), run(False)
            check_grads(got, ref.backward[mode][1], ref, what)
            for x, y in zip(got, mirror):
                assert x is None or same(x, y), what


def train_args(inp, tr, bufs):
    """The batch of a train entry in buffers of `bufs`: pos, neg, subsampling_weight."""
    pos = bufs.inp("pos", inp.pos)
    neg = bufs.inp("neg", inp.neg[tr.mode])
    w = bufs.inp("subsampling_weight", inp.w)
    return pos, neg, w


def adam_desc(b, m, shape, *, write_grad, step=2, moments=None):
    """A kge_adam_desc over the model's tables with moments in buffers of `b` (small non-zero
    values, so a row the step must not touch has something to lose)."""
    d = _lib.AdamDesc()
    d.beta1, d.beta2, d.eps, d.write_grad = BETAS[0], BETAS[1], EPS, int(write_grad)
    mom = {}
    for field, p in (("entity", m.e), ("relation", m.r), ("modulus", m.m)):
        if p is None:
            continue
        t = getattr(d, field)
        g = np.random.default_rng(shape.seed + len(field))
        m0 = (1e-3 * g.standard_normal(tuple(p.shape))).astype(np.float32)
        v0 = (1e-6 * g.random(tuple(p.shape))).astype(np.float32)
        if moments is not None and field in moments:
            m0, v0 = moments[field]
        mom[field] = (b.inp(f"{field}.exp_avg", m0, ro=False, phase=(p.data_ptr() % 256) if field == "entity" else 0),
                      b.inp(f"{field}.exp_avg_sq", v0, ro=False,
                            phase=(p.data_ptr() % 256) if field == "entity" else 0))
        t.param, t.exp_avg, t.exp_avg_sq = p.data_ptr(), mom[field][0].data_ptr(), mom[field][1].data_ptr()
        t.step_size = LR / (1 - BETAS[0] ** step)
        t.bias_correction2_sqrt = math.sqrt(1 - BETAS[1] ** step)
    return d, mom


def grad_bufs(b, shape, m, *, entity=True, phase=0):
    ge = b.out("grad_entity", (shape.E, shape.le), F32, phase=phase) if entity else None
    gr = b.out("grad_relation", (shape.R, shape.lr), F32)
    gm = b.out("grad_modulus", (1, 1), F32) if m.m is not None else None
    losses = b.out("losses_out", 5, F32)
    return ge, gr, gm, losses


def common_args(m, tr, pos, neg, w, n, wsum=None):
    return (m.desc, _lib.MODE_IDS[tr.mode], pos.data_ptr(), neg.data_ptr(), B, n, w.data_ptr(), ops._ptr(wsum),
            int(tr.uni_weight), 0, int(tr.adversarial), float(tr.temperature), float(tr.regularization))


def mirror_kwargs(tr):
    return dict(adversarial=tr.adversarial, temperature=tr.temperature, uni_weight=tr.uni_weight,
                regularization=tr.regularization)


TRAIN_SHAPES = A.SMALL + A.SLICED + A.WIDE_SHAPES


@pytest.mark.parametrize("shape", TRAIN_SHAPES, ids=lambda s: s.id)
def test_train_step_grads(shape):
    for n in n_of(shape):
        ref = refs(shape, n)
        inp = ref.inp
        for tr, (l64, g64) in zip(inp.trains, ref.train):
            what = f"{shape.id} train_step_grads {tr.mode} n{n}"

            def run(guarded):
                b = Bufs(guarded)
                m = model(b, tables(shape), shape.name)
                pos, neg, w = train_args(inp, tr, b)
                ge, gr, gm, losses = grad_bufs(b, shape, m)
                if not guarded:
                    ops.train_step_grads(m.desc, tr.mode, pos, neg, w, DEV, grad_entity=ge, grad_relation=gr,
                                         grad_modulus=gm, losses=losses, **mirror_kwargs(tr))
                else:
                    wp, wn = b.ws(lib().kge_train_workspace_bytes(m.desc, B, n))
                    ok(lib().kge_train_step_grads(*common_args(m, tr, pos, neg, w, n), ge.data_ptr(), gr.data_ptr(),
                                                  ops._ptr(gm), losses.data_ptr(), wp, wn, b.err(), stream()), what)
                b.verify(what)
                return [None if t is None else t.cpu() for t in (ge, gr, gm, losses)]

            got, mirror = run(True), run(False)
            ls = got[3].numpy()
            assert np.isfinite(ls[:3]).all() and np.all(np.abs(ls[:3] - l64) <= score_tol(l64)), (what, ls, l64)
            assert ls[4] == 0.0, what
            check_grads(got[:3], g64, ref, what)
            for x, y in zip(got[:3], mirror[:3]):
                assert x is None or same(x, y), what
            same_losses(got[3], mirror[3], tr.regularization, what)


@pytest.mark.parametrize("write_grad", [1, 0])
@pytest.mark.parametrize("shape", A.SMALL + A.SLICED + A.WIDE_SHAPES[:1], ids=lambda s: s.id)
def test_train_step_fused(shape, write_grad):
    """kge_train_step: tables and moments updated in place inside their arenas; with write_grad = 0
    grad_entity / grad_relation keep their fill.  The gradients are kge_train_step_grads' (held to
    the fp64 reference above) and the update is kge_adam_step's on them, bit for bit — the
    criterion of test_fused_adam_bitwise_equals_unfused."""
    n = n_of(shape)[-1]
    inp = batch(shape, n)
    for tr in inp.trains:
        what = f"{shape.id} train_step {tr.mode} n{n} write_grad={write_grad}"

        def run(guarded, fused=True):
            b = Bufs(guarded)
            m = model(b, tables(shape), shape.name, ro=not fused)
            pos, neg, w = train_args(inp, tr, b)
            ge, gr, gm, losses = grad_bufs(b, shape, m)
            ad, mom = adam_desc(b, m, shape, write_grad=write_grad)
            if not fused:  # the unfused composition, through the mirror: gradients, then kge_adam_step per tensor
                ops.train_step_grads(m.desc, tr.mode, pos, neg, w, DEV, grad_entity=ge, grad_relation=gr,
                                     grad_modulus=gm, losses=losses, **mirror_kwargs(tr))
                for field, p, g in (("entity", m.e, ge), ("relation", m.r, gr), ("modulus", m.m, gm)):
                    if p is not None:
                        ops.adam_step(p, g, mom[field][0], mom[field][1], step=2, lr=LR, beta1=BETAS[0],
                                      beta2=BETAS[1], eps=EPS)
            elif not guarded:
                ops.train_step_grads(m.desc, tr.mode, pos, neg, w, DEV, grad_entity=ge, grad_relation=gr,
                                     grad_modulus=gm, losses=losses, adam=ad, **mirror_kwargs(tr))
            else:
                wp, wn = b.ws(lib().kge_train_workspace_bytes(m.desc, B, n))
                ok(lib().kge_train_step(*common_args(m, tr, pos, neg, w, n), C.byref(ad), ge.data_ptr(),
                                        gr.data_ptr(), ops._ptr(gm), losses.data_ptr(), wp, wn, b.err(), stream()),
                   what)
            b.verify(what)
            if guarded and not write_grad:
                b.arenas["grad_entity"].poisoned()
                b.arenas["grad_relation"].poisoned()
            out = {"losses": losses.cpu()}
            for field, p in (("entity", m.e), ("relation", m.r), ("modulus", m.m)):
                if p is not None:
                    out[field] = p.cpu()
                    out[field + ".m"], out[field + ".v"] = mom[field][0].cpu(), mom[field][1].cpu()
            if write_grad:
                out["ge"], out["gr"] = ge.cpu(), gr.cpu()
            return out

        got, mirror, unfused = run(True), run(False), run(False, fused=False)
        for k in got:
            if k == "losses":
                same_losses(got[k], mirror[k], tr.regularization, what)
                same_losses(got[k], unfused[k], tr.regularization, what)
            else:
                assert same(got[k], mirror[k]), f"{what}: {k} differs from the mirror's"
                assert same(got[k], unfused[k]), f"{what}: {k} differs from gradients + kge_adam_step"


PHASED = tuple((s, 0) for s in A.SMALL if s.E == 257) + ((A.SLICED[0], 0), (A.SLICED[0], 16))


@pytest.mark.parametrize("shape,phase", PHASED, ids=lambda x: x.id if isinstance(x, A.Shape) else f"phase{x}")
def test_train_step_grads_phased(shape, phase):
    """ROWS, then ENTITY over [0, 100), [100, 257) and an empty range, then FINALIZE: the single
    call's gradients and losses bit for bit (test_phased_step_bitwise_equals_single_call).  RotatE
    at span 280 with the entity table, grad_entity (and, fused, the moments) 16 bytes past a
    256-byte boundary: the line-aligned column slicing with a non-zero row phase, which torch's
    512-byte aligned tensors never reach."""
    n = n_of(shape)[-1]
    ref = refs(shape, n)
    inp = ref.inp
    chunks = ((0, 100), (100, shape.E), (57, 57))
    for tr, (l64, g64) in zip(inp.trains, ref.train):
        what = f"{shape.id} phased {tr.mode} n{n} phase {phase}"

        def run(guarded, phased=True):
            b = Bufs(guarded)
            m = model(b, tables(shape), shape.name, phase=phase)
            assert m.e.data_ptr() % 256 == phase
            pos, neg, w = train_args(inp, tr, b)
            ge, gr, gm, losses = grad_bufs(b, shape, m, phase=phase)
            whole = (0, shape.E)  # (FINALIZE sums the regulariser's entity partials over its range: the whole table)
            steps = [(_lib.PHASE_ALL, *whole)] if not phased else \
                [(_lib.PHASE_ROWS, *whole)] + [(_lib.PHASE_ENTITY, a, z) for a, z in chunks] + [(_lib.PHASE_FINALIZE, *whole)]
            for ph, e0, e1 in steps:
                if not guarded:
                    ops.train_step_grads(m.desc, tr.mode, pos, neg, w, DEV, grad_entity=ge, grad_relation=gr,
                                         grad_modulus=gm, losses=losses, phases=ph,
                                         entity_range=(e0, e1) if phased else None, **mirror_kwargs(tr))
                else:
                    wp, wn = b.ws(lib().kge_train_workspace_bytes(m.desc, B, n))
                    ok(lib().kge_train_step_grads_phased(*common_args(m, tr, pos, neg, w, n), ge.data_ptr(),
                                                         gr.data_ptr(), ops._ptr(gm), losses.data_ptr(), wp, wn,
                                                         b.err(), stream(), ph, e0, e1), what)
            b.verify(what)
            return [None if t is None else t.cpu() for t in (ge, gr, gm, losses)]

        got, mirror, single = run(True), run(False), run(False, phased=False)
        ls = got[3].numpy()
        assert np.all(np.abs(ls[:3] - l64) <= score_tol(l64)), (what, ls, l64)
        check_grads(got[:3], g64, ref, what)
        for x, y, z in zip(got[:3], mirror[:3], single[:3]):
            assert x is None or (same(x, y) and same(x, z)), what
        same_losses(got[3], mirror[3], tr.regularization, what)
        same_losses(got[3], single[3], tr.regularization, what)


@pytest.mark.parametrize("bn", [(5, 65), (2, 3)], ids=lambda x: f"B{x[0]}n{x[1]}")
@pytest.mark.parametrize("shape", tuple(s for s in A.SMALL if s.E == 257) + (A.Shape("TransE", 256, 37),),
                         ids=lambda s: s.id)
def test_train_step_lazy(shape, bn):
    """kge_train_step_lazy with grad_entity NULL: (B, n) = (5, 65) has 335 occurrences, above E,
    so the touched list has E places; (2, 3) has 10.  Touched rows start from zero moments and are
    held to lazy_adam_cases.lazy_adam_ref on the dense gradient (test_lazy_adam_gpu's bound for the
    restated rule).  Untouched rows start from small non-zero moments, and their rows of the table
    and of both moments are compared byte for byte with what was put in: a pass that wrongly visits
    an in-range untouched row finds an empty bucket (gradient 0), so it scales that row's m by
    beta1 and its v by beta2 and moves p by -step_size · m / (sqrt(v) / bc2s + eps) — every one a
    change of bytes (from zero moments it would change nothing, which is why these are not zero).
    The relation table's dense update, its gradient and the losses equal the mirror's."""
    nb, n = bn
    tabs = tables(shape)
    ent0 = torch.from_numpy(np.array(tabs[0]))
    pos0, neg0, w0 = synth.kge_batch(shape.seed + 5, nb, n, shape.E, shape.R)
    touched = L.touched_ids(torch.from_numpy(pos0), torch.from_numpy(neg0), shape.E)
    assert len(touched) == len(set(pos0[:, [0, 2]].ravel()) | set(neg0.ravel()))
    un = torch.ones(shape.E, dtype=torch.bool)
    un[touched] = False
    assert un.sum() >= 16, "the case should leave rows untouched"
    g_ = np.random.default_rng(shape.seed + 23)
    m0 = (1e-3 * g_.standard_normal(tabs[0].shape)).astype(np.float32)
    v0 = (1e-6 * (0.1 + g_.random(tabs[0].shape))).astype(np.float32)
    m0[touched.numpy()] = 0.0  # lazy_adam_ref starts from zero moments: the touched rows only
    v0[touched.numpy()] = 0.0
    assert m0[un.numpy()].all() and v0[un.numpy()].all()
    start = {"entity": ent0, "m": torch.from_numpy(m0), "v": torch.from_numpy(v0)}
    for mode in MODES:
        tr = S.Train(mode, True, 0.75, False, 0.0)
        what = f"{shape.id} lazy {mode} B{nb} n{n}"

        def run(guarded, lazy=True):
            b = Bufs(guarded)
            m = model(b, tabs, shape.name, ro=False)
            pos, neg, w = b.inp("pos", pos0), b.inp("neg", neg0), b.inp("subsampling_weight", w0)
            ge, gr, gm, losses = grad_bufs(b, shape, m, entity=not lazy)
            ad, mom = adam_desc(b, m, shape, write_grad=1, step=1, moments={"entity": (m0, v0)})
            args = (m.desc, _lib.MODE_IDS[mode], pos.data_ptr(), neg.data_ptr(), nb, n, w.data_ptr(), None, 0, 0, 1,
                    0.75, 0.0)
            if not lazy:  # dense gradients alone, through the mirror
                ops.train_step_grads(m.desc, mode, pos, neg, w, DEV, grad_entity=ge, grad_relation=gr,
                                     grad_modulus=gm, losses=losses, **mirror_kwargs(tr))
            elif not guarded:
                ops.train_step_grads(m.desc, mode, pos, neg, w, DEV, grad_entity=None, grad_relation=gr,
                                     grad_modulus=gm, losses=losses, adam=ad, lazy=True, **mirror_kwargs(tr))
            else:
                wp, wn = b.ws(lib().kge_train_lazy_workspace_bytes(m.desc, nb, n))
                ok(lib().kge_train_step_lazy(*args, C.byref(ad), None, gr.data_ptr(), ops._ptr(gm),
                                             losses.data_ptr(), wp, wn, b.err(), stream()), what)
            b.verify(what)
            out = {"entity": m.e.cpu(), "m": mom["entity"][0].cpu(), "v": mom["entity"][1].cpu(),
                   "relation": m.r.cpu(), "gr": gr.cpu(), "losses": losses.cpu()}
            if not lazy:
                out["ge"] = ge.cpu()
            return out

        got, mirror, dense = run(True), run(False), run(False, lazy=False)
        for k in got:
            assert same(got[k], mirror[k]), f"{what}: {k} differs from the mirror's"
        p, mm, vv = L.lazy_adam_ref(ent0, [dense["ge"]], [touched], lr=LR, betas=BETAS, eps=EPS)
        for k, want in (("entity", p), ("m", mm), ("v", vv)):  # (test_lazy_adam_gpu's bound for the restated rule)
            torch.testing.assert_close(got[k][touched], want[touched], rtol=2e-6, atol=1e-7,
                                       msg=lambda s_: f"{what} {k}: {s_}")
        for k in ("entity", "m", "v"):  # unchanged(), with the touched rows masked out
            a, z = bits(got[k][un]), bits(start[k][un])
            bad = (a != z).any(dim=1).nonzero().reshape(-1)
            assert not len(bad), (f"{what}: {len(bad)} untouched row(s) of {k} changed, first row "
                                  f"{int(un.nonzero().reshape(-1)[bad[0]])}")
        # the same comparison does see a wrong visit: the update of an empty bucket changes all three
        e = int(un.nonzero()[0])
        mw = m0[e] + np.float32(1.0 - BETAS[0]) * (np.float32(0.0) - m0[e])
        vw = v0[e] * np.float32(BETAS[1])
        pw = tabs[0][e] + np.float32(-LR / (1 - BETAS[0])) * (mw / (np.sqrt(vw) / np.float32(math.sqrt(1 - BETAS[1]))
                                                                       + np.float32(EPS)))
        assert (mw != m0[e]).all() and (vw != v0[e]).all() and (pw != tabs[0][e]).any(), what


# ------------------------------------------------------------ factor exchange
@pytest.mark.parametrize("shape", tuple(s for s in A.SMALL if s.E == 257) + A.SLICED, ids=lambda s: s.id)
def test_rows_slices_then_from_rows(shape):
    """kge_weight_sum, two half-batch kge_train_rows_slice calls written into the gathered g / dq /
    stats arenas, then kge_train_step_from_rows on the whole batch: the single call's gradients
    and losses (the fp64 criterion; bit-identical to the mirror's exchange and to its single call)."""
    n = n_of(shape)[-1]
    ref = refs(shape, n)
    inp = ref.inp
    cuts = ((0, B // 2), (B // 2, B))
    for tr, (l64, g64) in zip(inp.trains, ref.train):
        what = f"{shape.id} from_rows {tr.mode} n{n}"

        def run(guarded, exchange=True):
            b = Bufs(guarded)
            m = model(b, tables(shape), shape.name)
            pos, neg, w = train_args(inp, tr, b)
            ge, gr, gm, losses = grad_bufs(b, shape, m)
            if not exchange:
                ops.train_step_grads(m.desc, tr.mode, pos, neg, w, DEV, grad_entity=ge, grad_relation=gr,
                                     grad_modulus=gm, losses=losses, **mirror_kwargs(tr))
                b.verify(what)
                return [None if t is None else t.cpu() for t in (ge, gr, gm, losses)]
            wsum = b.out("weight_sum", 1, F32)
            g = b.out("g", (B, n), F32)
            dq = b.out("dq", (B, shape.le), F32)
            stats = b.out("stats", (B, 4), F32)
            mid = _lib.MODE_IDS[tr.mode]
            if not guarded:
                ops.weight_sum(w, wsum)
                for a, z in cuts:
                    ops.train_rows_slice(m.desc, tr.mode, pos[a:z], neg[a:z], w[a:z], wsum, DEV,
                                         adversarial=tr.adversarial, temperature=tr.temperature,
                                         uni_weight=tr.uni_weight, uni_batch=B, g_out=g[a:z], dq_out=dq[a:z],
                                         stats_out=stats[a:z])
                ops.train_step_from_rows(m.desc, tr.mode, pos, neg, w, wsum, DEV, uni_weight=tr.uni_weight,
                                         uni_batch=B, regularization=tr.regularization, g_in=g, dq_in=dq,
                                         stats=stats, grad_entity=ge, grad_relation=gr, grad_modulus=gm,
                                         losses=losses)
            else:
                ok(lib().kge_weight_sum(w.data_ptr(), B, wsum.data_ptr(), stream()), "kge_weight_sum")
                for i, (a, z) in enumerate(cuts):
                    wp, wn = b.ws(lib().kge_train_workspace_bytes(m.desc, z - a, n), name=f"workspace.slice{i}")
                    ok(lib().kge_train_rows_slice(m.desc, mid, pos[a:z].data_ptr(), neg[a:z].data_ptr(), z - a, n,
                                                  w[a:z].data_ptr(), wsum.data_ptr(), int(tr.uni_weight), B,
                                                  int(tr.adversarial), float(tr.temperature), g[a:z].data_ptr(),
                                                  dq[a:z].data_ptr(), stats[a:z].data_ptr(), wp, wn, b.err(),
                                                  stream()), what + f" slice {i}")
                wp, wn = b.ws(lib().kge_train_workspace_bytes(m.desc, B, n))
                ok(lib().kge_train_step_from_rows(m.desc, mid, pos.data_ptr(), neg.data_ptr(), B, n, w.data_ptr(),
                                                  wsum.data_ptr(), int(tr.uni_weight), B,
                                                  float(tr.regularization), g.data_ptr(), dq.data_ptr(),
                                                  stats.data_ptr(), None, ge.data_ptr(), gr.data_ptr(), ops._ptr(gm),
                                                  losses.data_ptr(), wp, wn, b.err(), stream()), what)
            b.verify(what)
            return [None if t is None else t.cpu() for t in (ge, gr, gm, losses, g, dq)]

        got, mirror, single = run(True), run(False), run(False, exchange=False)
        ls = got[3].numpy()
        assert np.all(np.abs(ls[:3] - l64) <= score_tol(l64)), (what, ls, l64)
        check_grads(got[:3], g64, ref, what)
        for i, (x, y) in enumerate(zip(got, mirror)):
            if x is not None and i != 3:
                assert same(x, y), (what, i)
        for x, z in zip(got[:3], single[:3]):
            assert x is None or same(x, z), what
        same_losses(got[3], mirror[3], tr.regularization, what)
        same_losses(got[3], single[3], tr.regularization, what)


@pytest.mark.parametrize("form", ["csr", "range", "phased"])
@pytest.mark.parametrize("shape", (A.Shape("RotatE", 257, 36), A.Shape("DistMult", 257, 36), A.Shape("TransE", 257, 37),
                                   A.SLICED[0]), ids=lambda s: s.id)
def test_from_rows_csr_and_range(shape, form):
    """kge_train_csr → kge_train_step_from_rows_csr (the whole table), and the owner-computes
    forms over [100, 257): kge_train_csr_range → kge_train_step_from_rows_range / _phased with a
    fused Adam whose moment arenas hold exactly 157 rows, the pointers passed 100 rows before
    them (as the header allows): the bands sit exactly where rows 99 and 257 would be.  Rows
    0..99 of the table keep their bits and rows 0..99 of grad_entity their fill; the owned rows, their moments, the relation table and
    the losses equal the mirror's bit for bit, and the owned rows equal the whole-table fused
    step's (kge_train_step)."""
    n = n_of(shape)[-1]
    inp = batch(shape, n)
    e0, e1 = (0, shape.E) if form == "csr" else (100, shape.E)
    tr = inp.trains[1]
    what = f"{shape.id} {form} {tr.mode} n{n}"
    g_ = np.random.default_rng(shape.seed + 3)
    m0 = (1e-3 * g_.standard_normal((shape.E, shape.le))).astype(np.float32)
    v0 = (1e-6 * g_.random((shape.E, shape.le))).astype(np.float32)

    def run(guarded, whole=False):
        b = Bufs(guarded)
        m = model(b, tables(shape), shape.name, ro=False)
        pos, neg, w = train_args(inp, tr, b)
        ge, gr, gm, losses = grad_bufs(b, shape, m)
        ad, mom = adam_desc(b, m, shape, write_grad=1, moments={"entity": (m0, v0)})
        if whole:  # the single fused step on the whole table, through the mirror
            ops.train_step_grads(m.desc, tr.mode, pos, neg, w, DEV, grad_entity=ge, grad_relation=gr,
                                 grad_modulus=gm, losses=losses, adam=ad, **mirror_kwargs(tr))
            b.verify(what)
            return {"entity": m.e.cpu(), "m": mom["entity"][0].cpu(), "v": mom["entity"][1].cpu(),
                    "relation": m.r.cpu(), "losses": losses.cpu(), "ge": ge.cpu()}
        # shard-sized entity moments, addressed by global row
        sm = b.inp("shard.exp_avg", m0[e0:e1], ro=False)
        sv = b.inp("shard.exp_avg_sq", v0[e0:e1], ro=False)
        ad.entity.exp_avg = sm.data_ptr() - e0 * shape.le * 4
        ad.entity.exp_avg_sq = sv.data_ptr() - e0 * shape.le * 4
        wsum = b.out("weight_sum", 1, F32)
        g, dq, stats = b.out("g", (B, n), F32), b.out("dq", (B, shape.le), F32), b.out("stats", (B, 4), F32)
        mid = _lib.MODE_IDS[tr.mode]
        if not guarded:
            wst = ops.state(DEV).workspace(lib().kge_train_workspace_bytes(m.desc, B, n))
            ops.weight_sum(w, wsum)
            ops.train_rows_slice(m.desc, tr.mode, pos, neg, w, wsum, DEV, adversarial=tr.adversarial,
                                 temperature=tr.temperature, uni_weight=tr.uni_weight, uni_batch=B, g_out=g,
                                 dq_out=dq, stats_out=stats)
            ops.train_csr(m.desc, tr.mode, pos, neg, DEV, workspace=wst,
                          entity_range=None if form == "csr" else (e0, e1))
            kw = dict(uni_weight=tr.uni_weight, uni_batch=B, regularization=tr.regularization, g_in=g, dq_in=dq,
                      stats=stats, grad_entity=ge, grad_relation=gr, grad_modulus=gm, losses=losses, adam=ad,
                      csr_ready=True, workspace=wst)
            if form == "csr":
                ops.train_step_from_rows(m.desc, tr.mode, pos, neg, w, wsum, DEV, **kw)
            elif form == "range":
                ops.train_step_from_rows(m.desc, tr.mode, pos, neg, w, wsum, DEV, entity_range=(e0, e1), **kw)
            else:
                for ph, a, z in ((_lib.PHASE_ROWS, e0, e1), (_lib.PHASE_ENTITY, e0, 180), (_lib.PHASE_ENTITY, 180, e1),
                                 (_lib.PHASE_FINALIZE, e0, e1)):
                    ops.train_step_from_rows(m.desc, tr.mode, pos, neg, w, wsum, DEV, entity_range=(a, z), phases=ph,
                                             **kw)
        else:
            ok(lib().kge_weight_sum(w.data_ptr(), B, wsum.data_ptr(), stream()), "kge_weight_sum")
            wp, wn = b.ws(lib().kge_train_workspace_bytes(m.desc, B, n))
            ok(lib().kge_train_rows_slice(m.desc, mid, pos.data_ptr(), neg.data_ptr(), B, n, w.data_ptr(),
                                          wsum.data_ptr(), int(tr.uni_weight), B, int(tr.adversarial),
                                          float(tr.temperature), g.data_ptr(), dq.data_ptr(), stats.data_ptr(), wp, wn,
                                          b.err(), stream()), what + " rows")
            if form == "csr":
                ok(lib().kge_train_csr(m.desc, mid, pos.data_ptr(), neg.data_ptr(), B, n, wp, wn, b.err(), stream()),
                   what + " csr")
            else:
                ok(lib().kge_train_csr_range(m.desc, mid, pos.data_ptr(), neg.data_ptr(), B, n, e0, e1, wp, wn,
                                             b.err(), stream()), what + " csr_range")
            args = (m.desc, mid, pos.data_ptr(), neg.data_ptr(), B, n, w.data_ptr(), wsum.data_ptr(),
                    int(tr.uni_weight), B, float(tr.regularization), g.data_ptr(), dq.data_ptr(), stats.data_ptr(),
                    C.byref(ad), ge.data_ptr(), gr.data_ptr(), ops._ptr(gm), losses.data_ptr(), wp, wn, b.err(),
                    stream())
            if form == "csr":
                ok(lib().kge_train_step_from_rows_csr(*args), what)
            elif form == "range":
                ok(lib().kge_train_step_from_rows_range(*args, e0, e1, 1, 1), what)
            else:
                for ph, a, z in ((_lib.PHASE_ROWS, e0, e1), (_lib.PHASE_ENTITY, e0, 180), (_lib.PHASE_ENTITY, 180, e1),
                                 (_lib.PHASE_FINALIZE, e0, e1)):
                    ok(lib().kge_train_step_from_rows_phased(*args, ph, a, z, 1, 1), what + f" phase {ph}")
        b.verify(what)
        if guarded and e0:  # no gradient row below the owned range was written: those rows keep the arena's fill
            below = b.arenas["grad_entity"].bytes[:e0 * shape.le * 4]
            bad = (below != FLOAT_FILL).nonzero()
            assert not bad.numel(), (f"{what}: {bad.shape[0]} byte(s) of grad_entity rows below {e0} written, first "
                                     f"in row {int(bad[0, 0]) // (shape.le * 4)}")
        return {"entity": m.e.cpu(), "m": sm.cpu(), "v": sv.cpu(), "relation": m.r.cpu(), "losses": losses.cpu(),
                "ge": ge.cpu()[e0:e1]}

    got, mirror, whole = run(True), run(False), run(False, whole=True)
    for k in got:
        if k == "losses":
            same_losses(got[k], mirror[k], tr.regularization, what)
        else:
            assert same(got[k], mirror[k]), f"{what}: {k} differs from the mirror's"
    ent0 = torch.from_numpy(np.array(tables(shape)[0]))
    assert same(got["entity"][:e0], ent0[:e0]), f"{what}: a row below the owned range was written"
    assert same(got["entity"][e0:e1], whole["entity"][e0:e1]), f"{what}: owned rows differ from kge_train_step's"
    assert same(got["m"], whole["m"][e0:e1]) and same(got["v"], whole["v"][e0:e1]), what
    assert same(got["ge"], whole["ge"][e0:e1]) and same(got["relation"], whole["relation"]), what


# ------------------------------------------------- weight sum and dense Adam
def test_weight_sum_and_adam_step():
    """numel = 257 · 37, odd.  kge_adam_step against oracle.adam_steps (torch.optim.Adam) to
    test_kge_adam_matches_torch_adam's bound, and bit-identical to the mirror's; kge_weight_sum
    against its documented summation order restated in fp32, bit for bit."""
    E, d = 257, 37
    g_ = np.random.default_rng(11)
    p0 = g_.standard_normal((E, d)).astype(np.float32)
    grads = [g_.standard_normal((E, d)).astype(np.float32) for _ in range(2)]
    w0 = g_.uniform(0.2, 1.0, E * d).astype(np.float32)

    def run(guarded):
        b = Bufs(guarded)
        p = b.inp("param", p0, ro=False)
        m = b.inp("exp_avg", np.zeros_like(p0), ro=False)
        v = b.inp("exp_avg_sq", np.zeros_like(p0), ro=False)
        w = b.inp("w", w0)
        out = b.out("weight_sum", 1, F32)
        if guarded:
            ok(lib().kge_weight_sum(w.data_ptr(), E * d, out.data_ptr(), stream()), "kge_weight_sum")
        else:
            ops.weight_sum(w, out)
        for step, g0 in enumerate(grads, 1):
            g = b.inp(f"grad{step}", g0)
            if guarded:
                ok(lib().kge_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), E * d, BETAS[0],
                                       BETAS[1], EPS, LR / (1 - BETAS[0] ** step), math.sqrt(1 - BETAS[1] ** step),
                                       stream()), "kge_adam_step")
            else:
                ops.adam_step(p, g, m, v, step=step, lr=LR, beta1=BETAS[0], beta2=BETAS[1], eps=EPS)
        b.verify("adam")
        return [t.cpu() for t in (p, m, v, out)]

    got, mirror = run(True), run(False)
    for x, y in zip(got, mirror):
        assert same(x, y)
    (rp,), ((rm, rv),) = O.adam_steps([torch.from_numpy(p0)], [[torch.from_numpy(g)] for g in grads], LR)
    # (the parameters, as test_kge_adam_matches_torch_adam; the library forms 1 - beta in fp32, torch in
    # double, so the moments have no bound against torch's: the mirror's bits above)
    torch.testing.assert_close(got[0], rp, rtol=2e-6, atol=1e-7)
    # kge_weight_sum's order is fixed and part of its contract (kge_hip.h: "the same fixed order as a
    # single process's in-kernel sum"; block_weight_sum): thread t of 256 adds w[t], w[t + 256], ... in
    # turn, then a tree folds the 256 partial sums, upper half onto lower.  Restated in fp32: exact.
    part = np.zeros(256, dtype=np.float32)
    for k in range(0, len(w0), 256):
        chunk = w0[k:k + 256]
        part[:len(chunk)] = part[:len(chunk)] + chunk
    o = 128
    while o:
        part[:o] = part[:o] + part[o:2 * o]
        o //= 2
    assert got[3].numpy().view(np.int32)[0] == part[:1].view(np.int32)[0], (float(got[3]), float(part[0]))


# ------------------------------------------------------------ filtered ranks
def rank_paths(shape):
    """(path id, name) of every fast pass rank_path accepts for the model at this span."""
    bil = shape.name in ("DistMult", "ComplEx")
    out = [(0, "auto"), (3, "scan")]
    if shape.d % 4 == 0:
        out.append((2, "tile"))
    if bil:
        out.append((1, "mfma"))
    if bil and shape.le % 4 == 0:
        out.append((4, "mfma32"))
    return out


@lru_cache(maxsize=None)
def rank_inputs(shape, nq):
    """(queries [nq, 3], all_true_triples): the last query's filter lists are not empty (the last
    list ends exactly at filt_ids' end) and, nq > 1, query 0's are empty in both directions."""
    E, R = shape.E, shape.R
    g = np.random.default_rng(shape.seed + 31 + nq)
    tr = np.unique(np.stack([g.integers(0, E, 6 * E), g.integers(0, R, 6 * E), g.integers(0, E, 6 * E)], 1), axis=0)
    q = tr[g.permutation(len(tr))[:nq]].copy()
    h, r, t = q[-1]
    extra = [(h, r, (t + k) % E) for k in (1, 2, 64, 255)] + [((h + k) % E, r, t) for k in (1, 3, 200)]
    tr = np.unique(np.concatenate([tr, np.asarray(extra, dtype=np.int64)]), axis=0)
    if nq > 1:
        h, r, t = q[0]
        drop = ((tr[:, 0] == h) & (tr[:, 1] == r)) | ((tr[:, 1] == r) & (tr[:, 2] == t))
        tr = np.concatenate([tr[~drop], q[:1]])
    q.setflags(write=False)
    tr.setflags(write=False)
    return q, tr


@lru_cache(maxsize=None)
def oracle_ranks(shape, nq, mode):
    ent, rel, mod, erange = tables(shape)
    q, tr = rank_inputs(shape, nq)
    t = lambda a: None if a is None else torch.from_numpy(np.array(a))  # noqa: E731
    r = O.filtered_ranks(shape.name, t(ent), t(rel), t(mod), q, tr, mode, torch.Tensor([A.GAMMA]).item(), erange)
    return np.asarray(r["rank_count"], dtype=np.int64), np.asarray(r["ties"], dtype=np.int32)


def filters_of(shape, nq, mode, table):
    q, tr = rank_inputs(shape, nq)
    idx = FilterIndex(tr, shape.E, shape.R)
    if table:
        off, ids = idx._host_table_on(mode, "cpu")
        off, ids = off.numpy(), ids.numpy()
        assert off.shape == (shape.E * shape.R + 1,) and off[-1] == len(ids)
    else:
        off, ids = idx.filter_csr(q, mode)
        assert off.shape == (nq + 1,) and off[-1] == len(ids) and off[-1] > off[-2]
        assert nq == 1 or off[1] == off[0]
    return off, ids


RANK_SHAPES = A.SMALL + A.WIDE_SHAPES


@pytest.mark.parametrize("nq", A.NQS)
@pytest.mark.parametrize("shape", RANK_SHAPES, ids=lambda s: s.id)
def test_rank_filtered(shape, nq):
    """kge_rank_filtered and kge_rank_filtered_ex on every path rank_path accepts, per-query lists
    and the whole filter index (exactly E·R + 1 offsets), KGE_RANK_REUSE_TABLE on the first call of
    a poisoned workspace (the tag cannot match: the unflagged call's ranks).  Ranks and ties: the
    oracle's (not pRotatE, whose one-call form uses the device's correctly rounded sin: the mirror's
    bits there, the oracle's in test_protate_three_calls); RotatE also with relation_trig."""
    q0, _ = rank_inputs(shape, nq)
    wide = shape.d == A.WIDE
    paths = [(3, "scan")] if wide else rank_paths(shape)  # (wide rows: the wave scan)
    ap, an = paths[0]
    for mode in MODES:
        want = oracle_ranks(shape, nq, mode) if shape.name != "pRotatE" else None
        variants = [(p, nm, False, False, False) for p, nm in paths]
        variants += [(ap, an, True, False, False), (ap, an, False, True, False)]
        if shape.name == "RotatE":
            variants.append((ap, an, False, False, True))
        results = {}
        for path, pname, table, reuse, trig in variants:
            what = f"{shape.id} rank nq{nq} {mode} {pname} table={table} reuse={reuse} trig={trig}"
            off0, ids0 = filters_of(shape, nq, mode, table)

            def run(guarded):
                b = Bufs(guarded)
                m = model(b, tables(shape), shape.name, trig=trig)
                q = b.inp("queries", q0)
                off, ids = b.inp("filt_off", off0), b.inp("filt_ids", ids0)
                if not guarded:
                    st = ops.state(DEV)
                    st.rank_ws_ptr = 0
                    r, t, ls = ops.rank_filtered(m.desc, mode, q, off, ids, DEV, path=pname, listed=True,
                                                 relation_trig=m.trig, filter_table=table)
                else:
                    r, t, ls = b.out("ranks", nq, I64), b.out("ties", nq, I32), b.out("listed", nq, I32)
                    wp, wn = b.ws(lib().kge_rank_workspace_bytes(m.desc, nq))
                    flags = path | (ops.RANK_REUSE_TABLE if reuse else 0) | (_lib.RANK_FILTER_TABLE if table else 0)
                    ok(lib().kge_rank_filtered_ex(m.desc, _lib.MODE_IDS[mode], q.data_ptr(), nq, off.data_ptr(),
                                                  ids.data_ptr(), r.data_ptr(), t.data_ptr(), ls.data_ptr(), flags,
                                                  wp, wn, b.err(), stream()), what)
                b.verify(what)
                return r.cpu(), t.cpu(), ls.cpu()

            got = run(True)
            if not reuse:
                mirror = run(False)
                assert all(same(x, y) for x, y in zip(got, mirror)), what
            if want is not None:
                assert np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[1].numpy(), want[1]), what
            results[(pname, table, reuse, trig)] = got
        base = results[(an, False, False, False)]
        for key, got in results.items():
            if not key[3]:
                assert same(got[0], base[0]) and same(got[1], base[1]), (shape.id, mode, key)
    # the plain entry (no path, no listed_out)
    mode = "tail-batch"
    off0, ids0 = filters_of(shape, nq, mode, False)
    b = Bufs(True)
    m = model(b, tables(shape), shape.name)
    q, off, ids = b.inp("queries", q0), b.inp("filt_off", off0), b.inp("filt_ids", ids0)
    r, t = b.out("ranks", nq, I64), b.out("ties", nq, I32)
    wp, wn = b.ws(lib().kge_rank_workspace_bytes(m.desc, nq))
    ok(lib().kge_rank_filtered(m.desc, _lib.MODE_IDS[mode], q.data_ptr(), nq, off.data_ptr(), ids.data_ptr(),
                               r.data_ptr(), t.data_ptr(), wp, wn, b.err(), stream()), "kge_rank_filtered")
    b.verify("kge_rank_filtered")
    assert same(r, results[(an, False, False, False)][0]) and same(t, results[(an, False, False, False)][1])


@pytest.mark.parametrize("table", [False, True], ids=["lists", "table"])
@pytest.mark.parametrize("shape", tuple(s for s in A.SMALL if s.name != "pRotatE") + (A.Shape("pRotatE", 257, 36),),
                         ids=lambda s: s.id)
def test_rank_filtered_both(shape, table):
    """kge_rank_filtered_both: outputs of exactly [2 · nq], the workspace of 2 · nq queries."""
    nq = 65
    q0, _ = rank_inputs(shape, nq)
    fh, ft = filters_of(shape, nq, "head-batch", table), filters_of(shape, nq, "tail-batch", table)
    what = f"{shape.id} both table={table}"

    def run(guarded):
        b = Bufs(guarded)
        m = model(b, tables(shape), shape.name)
        q = b.inp("queries", q0)
        oh, ih = b.inp("filt_off_head", fh[0]), b.inp("filt_ids_head", fh[1])
        ot, it = b.inp("filt_off_tail", ft[0]), b.inp("filt_ids_tail", ft[1])
        if not guarded:
            ops.state(DEV).rank_ws_ptr = 0
            r, t, ls = ops.rank_filtered_both(m.desc, q, (oh, ih), (ot, it), DEV, listed=True, filter_table=table)
        else:
            r, t, ls = b.out("ranks", 2 * nq, I64), b.out("ties", 2 * nq, I32), b.out("listed", 2 * nq, I32)
            wp, wn = b.ws(lib().kge_rank_workspace_bytes(m.desc, 2 * nq))
            ok(lib().kge_rank_filtered_both(m.desc, q.data_ptr(), nq, oh.data_ptr(), ih.data_ptr(), ot.data_ptr(),
                                            it.data_ptr(), r.data_ptr(), t.data_ptr(), ls.data_ptr(),
                                            _lib.RANK_FILTER_TABLE if table else 0, wp, wn, b.err(), stream()), what)
        b.verify(what)
        return r.cpu(), t.cpu(), ls.cpu()

    got, mirror = run(True), run(False)
    assert all(same(x, y) for x, y in zip(got, mirror)), what
    if shape.name != "pRotatE":
        for k, mode in enumerate(MODES):
            wr, wt = oracle_ranks(shape, nq, mode)
            assert np.array_equal(got[0][k * nq:(k + 1) * nq].numpy(), wr), (what, mode)
            assert np.array_equal(got[1][k * nq:(k + 1) * nq].numpy(), wt), (what, mode)


TIE_CASE = next(c for c in T.CASES if c.name == "DistMult" and c.d == 32 and c.aligned)


@pytest.mark.parametrize("path", TIE_CASE.paths)
def test_rank_near_tie_lists(path):
    """rank_tie_cases' DistMult table on each fast path: one query lists exactly 1024 near-ties,
    one 1025 and some more.  A list row written past its 1024 places lands in the next sub-buffer
    of the workspace (or, for the last query, in the filter bitmap) and surfaces as wrong ranks."""
    case = TIE_CASE
    ent, rel, mod, erange = T.tables(case)
    q0 = T.queries(case)
    nq = len(q0)
    idx = FilterIndex(T.true_triples(case), case.E, nq)
    for mode in MODES:
        off0, ids0 = idx.filter_csr(q0, mode)
        what = f"{case.id} {mode} {path}"

        def run(guarded):
            b = Bufs(guarded)
            m = model(b, (ent, rel, mod, erange), case.name)
            q, off, ids = b.inp("queries", q0), b.inp("filt_off", off0), b.inp("filt_ids", ids0)
            if not guarded:
                ops.state(DEV).rank_ws_ptr = 0
                r, t, ls = ops.rank_filtered(m.desc, mode, q, off, ids, DEV, path=path, listed=True)
            else:
                r, t, ls = b.out("ranks", nq, I64), b.out("ties", nq, I32), b.out("listed", nq, I32)
                wp, wn = b.ws(lib().kge_rank_workspace_bytes(m.desc, nq))
                ok(lib().kge_rank_filtered_ex(m.desc, _lib.MODE_IDS[mode], q.data_ptr(), nq, off.data_ptr(),
                                              ids.data_ptr(), r.data_ptr(), t.data_ptr(), ls.data_ptr(),
                                              ops.RANK_PATHS[path], wp, wn, b.err(), stream()), what)
            b.verify(what)
            return r.cpu(), t.cpu(), ls.cpu()

        got, mirror = run(True), run(False)
        assert all(same(x, y) for x, y in zip(got, mirror)), what
        listed = got[2].numpy()
        assert (listed == T.CAP).any() and (listed == T.CAP + 1).any() and (listed > T.CAP + 1).any(), what
        wr, wt = T.reference(case, mode)
        assert np.array_equal(got[0].numpy(), wr) and np.array_equal(got[1].numpy(), wt), what


@pytest.mark.parametrize("mode", MODES)
def test_protate_three_calls(mode):
    """KGE_RANK_STAGE_LIST, kge_rank_sin_args, the host's torch.sin, kge_rank_finish_sin on one
    workspace arena that is not refilled in between; args_out and sin_values hold exactly
    item_off[nq] rows.  Ranks and ties: the oracle's (the three-call form is bit-exact)."""
    shape = A.Shape("pRotatE", 257, 36)
    nq = 65
    ent, rel, mod, erange = tables(shape)
    ent = np.array(ent)
    ent[100:110] = ent[5]  # ten exact copies of entity 5: near-ties only the host sin can order
    q0, tr = rank_inputs(shape, nq)
    q0 = np.array(q0)
    q0[::2, 0 if mode == "head-batch" else 2] = 5
    idx = FilterIndex(tr, shape.E, shape.R)
    off0, ids0 = idx.filter_csr(q0, mode)
    ids0 = ids0 if len(ids0) else np.zeros(1, dtype=np.int64)
    mid = _lib.MODE_IDS[mode]
    b = Bufs(True)
    m = model(b, (ent, rel, mod, erange), shape.name)
    q, off, ids = b.inp("queries", q0), b.inp("filt_off", off0), b.inp("filt_ids", ids0)
    r, t, cnt = b.out("ranks", nq, I64), b.out("ties", nq, I32), b.out("listed", nq, I32)
    wp, wn = b.ws(lib().kge_rank_workspace_bytes(m.desc, nq))
    ok(lib().kge_rank_filtered_ex(m.desc, mid, q.data_ptr(), nq, off.data_ptr(), ids.data_ptr(), r.data_ptr(),
                                  t.data_ptr(), cnt.data_ptr(), _lib.RANK_STAGE_LIST, wp, wn, b.err(), stream()), "list")
    b.verify("list stage")
    c = cnt.cpu().numpy().astype(np.int64)
    items = np.where((c >= 1) & (c <= _lib.RANK_LIST_CAP), 1 + c, 0)
    io = np.zeros(nq + 1, dtype=np.int64)
    np.cumsum(items, out=io[1:])
    total = int(io[-1])
    assert total > 0, "the fixture should leave some near-ties for the host"
    item_off = b.inp("item_off", io)
    args = b.out("args_out", (total, shape.le), F32)
    ok(lib().kge_rank_sin_args(m.desc, mid, nq, item_off.data_ptr(), args.data_ptr(), wp, wn, b.err(), stream()), "args")
    b.verify("sin args")
    sins0 = torch.sin(args.cpu())
    assert torch.isfinite(sins0).all()
    sins = b.inp("sin_values", sins0)
    ok(lib().kge_rank_finish_sin(m.desc, mid, nq, item_off.data_ptr(), sins.data_ptr(), r.data_ptr(), t.data_ptr(),
                                 None, wp, wn, b.err(), stream()), "finish")
    b.verify("finish")
    tt = lambda a: torch.from_numpy(np.array(a))  # noqa: E731
    ref = O.filtered_ranks(shape.name, tt(ent), tt(rel), tt(mod), q0, tr, mode, torch.Tensor([A.GAMMA]).item(), erange)
    assert np.array_equal(r.cpu().numpy(), np.asarray(ref["rank_count"])), mode
    assert np.array_equal(t.cpu().numpy(), np.asarray(ref["ties"], dtype=np.int32)), mode
    # the mirror's library-sin form on ordinary tensors
    p = Bufs(False)
    pm = model(p, (ent, rel, mod, erange), shape.name)
    ops.state(DEV).rank_ws_ptr = 0
    mr, mt = ops.rank_filtered(pm.desc, mode, p.inp("q", q0), p.inp("o", off0), p.inp("i", ids0), DEV, library_sin=True)
    p.verify()
    assert same(r, mr) and same(t, mt)


# -------------------------------------------------------------------- top-k
@lru_cache(maxsize=None)
def topk_inputs(shape, nq, mode):
    q, tr = rank_inputs(shape, nq)
    return q, K.excluded_mask(q, mode, tr, nentity=shape.E), topk_scores(shape, nq, mode)


@lru_cache(maxsize=None)
def topk_scores(shape, nq, mode):
    ent, rel, mod, erange = tables(shape)
    assert erange == K.erange_of(shape.d), (erange, K.erange_of(shape.d))
    q, _ = rank_inputs(shape, nq)
    return K.oracle_scores(shape.name, np.array(ent), np.array(rel), mod, q, mode, d=shape.d)


@pytest.mark.parametrize("nq", A.NQS)
@pytest.mark.parametrize("shape", A.SMALL, ids=lambda s: s.id)
def test_topk(shape, nq):
    """kge_topk: outputs of exactly [nq, k], k in {1, 128}, parts in {0, 2, 5} (5 tiles of 64 at
    E = 257: 5 is the one-part-per-tile limit; E = 256 has 4 tiles, so 5 is replaced by 4), both
    paths the rows allow, per-query lists, the whole index and no filter; topk_cases.check_result."""
    max_parts = (shape.E + 63) // 64
    for mode in MODES:
        q0, mask, s64 = topk_inputs(shape, nq, mode)
        variants = [(k, min(parts, max_parts), "auto", "lists") for k in A.KS for parts in A.PARTS]
        variants += [(128, 2, "scan", "table"), (1, 0, "scan", None)]
        if shape.d % 4 == 0:
            variants.append((128, 0, "tile", "lists"))
        for k, parts, path, filt in variants:
            what = f"{shape.id} topk nq{nq} {mode} k{k} parts{parts} {path} {filt}"
            f0 = None if filt is None else filters_all(shape, nq, mode, filt == "table")

            def run(guarded):
                b = Bufs(guarded)
                m = model(b, tables(shape), shape.name)
                q = b.inp("queries", q0)
                off = ids = None
                if f0 is not None:
                    off, ids = b.inp("filt_off", f0[0]), b.inp("filt_ids", f0[1])
                if not guarded:
                    oi, os_ = ops.topk(m.desc, mode, q, k, DEV, filt=None if off is None else (off, ids),
                                       filter_table=filt == "table", path=path, parts=parts)
                else:
                    oi, os_ = b.out("ids_out", (nq, k), I64), b.out("scores_out", (nq, k), F32)
                    wp, wn = b.ws(lib().kge_topk_workspace_bytes(m.desc, nq, k, parts))
                    flags = ops.TOPK_PATHS[path] | (_lib.RANK_FILTER_TABLE if filt == "table" else 0)
                    ok(lib().kge_topk(m.desc, _lib.MODE_IDS[mode], q.data_ptr(), nq, ops._ptr(off), ops._ptr(ids), k,
                                      oi.data_ptr(), os_.data_ptr(), flags, parts, wp, wn, b.err(), stream()), what)
                b.verify(what)
                return oi.cpu(), os_.cpu()

            got, mirror = run(True), run(False)
            assert same(got[0], mirror[0]) and same(got[1], mirror[1]), what
            msk = mask if filt is not None else np.zeros_like(mask)
            K.check_result(got[0].numpy(), got[1].numpy(), s64, msk, k, True, what)


def filters_all(shape, nq, mode, table):
    """top-k excludes everything on the list (there is no true id): the whole-index form, or
    per-query lists cut from it."""
    q, tr = rank_inputs(shape, nq)
    if table:
        return filters_of(shape, nq, mode, True)
    mask = K.excluded_mask(q, mode, tr, nentity=shape.E)
    off, ids = K.csr_of(mask)
    return off, (ids if len(ids) else np.zeros(1, dtype=np.int64))


# ------------------------------------------------- candidate lists, relations
def cand_cases():
    out = []
    for nm in A.NAMES:
        out += [RC.Case(nm, 36, E=257, nq=65, C=65, pad=True), RC.Case(nm, 37, E=256, nq=1, C=1)]
    out += [RC.Case("TransE", 36, E=257, nq=65, C=1), RC.Case("DistMult", 37, E=256, nq=1, C=65),
            RC.Case("TransE", A.WIDE, E=A.WIDE_E, nq=6, C=65, pad=True),
            RC.Case("RotatE", A.WIDE, E=A.WIDE_E, nq=6, C=65, pad=True)]
    return out


@pytest.mark.parametrize("case", cand_cases(), ids=lambda c: c.id)
def test_rank_candidates(case):
    """kge_rank_candidates with -1 padding at the start, in the middle and at the end of a list:
    rank_candidates_cases.reference, exact (pRotatE: except where excusable, as its own GPU test)."""
    tab = RC.tables(case)
    q0 = RC.queries(case)
    for mode in MODES:
        c0 = RC.cand(case, mode)
        what = f"{case.id} {mode}"

        def run(guarded):
            b = Bufs(guarded)
            m = model(b, tab, case.name)
            q, cd = b.inp("queries", q0), b.inp("cand", c0)
            if not guarded:
                r, t = ops.rank_candidates(m.desc, mode, q, cd, DEV)
            else:
                r, t = b.out("ranks", case.nq, I64), b.out("ties", case.nq, I32)
                wp, wn = b.ws(lib().kge_rank_candidates_workspace_bytes(m.desc, case.nq, case.C))
                ok(lib().kge_rank_candidates(m.desc, _lib.MODE_IDS[mode], q.data_ptr(), case.nq, cd.data_ptr(),
                                             case.C, r.data_ptr(), t.data_ptr(), wp, wn, b.err(), stream()), what)
            b.verify(what)
            return r.cpu(), t.cpu()

        got, mirror = run(True), run(False)
        assert same(got[0], mirror[0]) and same(got[1], mirror[1]), what
        wr, wt = RC.reference(case, mode)
        bad = (got[0].numpy() != wr) | (got[1].numpy() != wt)
        if case.name == "pRotatE":
            bad &= ~RC.excusable(case, mode)
        assert not bad.any(), (what, np.nonzero(bad)[0])


def rel_cases():
    out = []
    for nm in A.NAMES:
        out += [RR.Case(nm, 36, R=65, E=257, nq=65), RR.Case(nm, 37, R=5, E=256, nq=1)]
    out += [RR.Case("RotatE", 37, R=65, E=256, nq=65), RR.Case("DistMult", A.WIDE, R=5, E=A.WIDE_E, nq=6),
            RR.Case("RotatE", A.WIDE, R=5, E=A.WIDE_E, nq=6)]
    return out


@pytest.mark.parametrize("with_scores", [True, False], ids=["scores", "noscores"])
@pytest.mark.parametrize("case", rel_cases(), ids=lambda c: c.id)
def test_rank_relations(case, with_scores):
    """kge_rank_relations, R in {5, 65}, with and without scores_out, filtered and raw; RotatE
    with relation_trig NULL, whose trig table is then the last buffer carve_rel lays out."""
    tab = RR.tables(case)
    q0 = RR.queries(case)
    off0, ids0 = RR.filt(case)
    ids0 = ids0 if len(ids0) else np.zeros(1, dtype=np.int64)
    for filtered in (True, False):
        what = f"{case.id} filtered={filtered} scores={with_scores}"

        def run(guarded):
            b = Bufs(guarded)
            m = model(b, tab, case.name)
            q = b.inp("queries", q0)
            off = ids = None
            if filtered:
                off, ids = b.inp("filt_off", off0), b.inp("filt_ids", ids0)
            if not guarded:
                out = ops.rank_relations(m.desc, q, DEV, filt=(off, ids) if filtered else None, scores=with_scores)
                r, t, sc = out if with_scores else (*out, None)
            else:
                r, t = b.out("ranks", case.nq, I64), b.out("ties", case.nq, I32)
                sc = b.out("scores_out", (case.nq, case.R), F32) if with_scores else None
                wp, wn = b.ws(lib().kge_rank_relations_workspace_bytes(m.desc, case.nq))
                ok(lib().kge_rank_relations(m.desc, q.data_ptr(), case.nq, ops._ptr(off), ops._ptr(ids), r.data_ptr(),
                                            t.data_ptr(), ops._ptr(sc), wp, wn, b.err(), stream()), what)
            b.verify(what)
            return r.cpu(), t.cpu(), None if sc is None else sc.cpu()

        got, mirror = run(True), run(False)
        assert same(got[0], mirror[0]) and same(got[1], mirror[1]), what
        assert got[2] is None or same(got[2], mirror[2]), what
        wr, wt = RR.reference(case, filtered)
        bad = (got[0].numpy() != wr) | (got[1].numpy() != wt)
        if case.name == "pRotatE":
            bad &= ~RR.excusable(case)
        elif case.name != "RotatE" and got[2] is not None:  # (RotatE without relation_trig: correctly rounded cos / sin)
            assert np.array_equal(got[2].numpy().view(np.int32), RR.scores(case).view(np.int32)), what
        assert not bad.any(), (what, np.nonzero(bad)[0])


# ------------------------------------------------------------------ sampler
@lru_cache(maxsize=None)
def sampler_graph():
    """E = 257, R = 5.  Relations 0-2: a random graph.  Relation 3: one triple (7, 3, tA) — its
    row is given an EMPTY true list on the device.  Relation 4: (9, 4, t) for every t but 123 —
    its row's list leaves a single allowed entity."""
    E = 257
    g = np.random.default_rng(17)
    base = np.unique(np.stack([g.integers(0, E, 300), g.integers(0, 3, 300), g.integers(0, E, 300)], 1), axis=0)
    full = np.array([[9, 4, t] for t in range(E) if t != 123], dtype=np.int64)
    return E, base, full


@pytest.mark.parametrize("n", A.NNEG)
def test_sample_negatives(n):
    E, base, full = sampler_graph()
    key = batch_key(5, n)
    max_draws = 1 << 20
    mode = "tail-batch"

    def graph(t_a):
        tr = np.concatenate([base, np.array([[7, 3, t_a]], dtype=np.int64), full])
        return tr, np.array([3, len(base), 11, len(base) + 1 + 40, len(tr) - 1], dtype=np.int64)

    # row 1 (the relation-3 triple) has an empty list on the device: its negatives are its stream's
    # first n draws.  The oracle always lists the row's own tail; two runs with different tails
    # that agree on the row's negatives show that neither tail was drawn, so both are the raw draws.
    want = None
    for t_a, t_b in ((1, 2), (3, 4), (5, 6), (8, 10), (12, 13), (14, 15)):
        (tr, bt), (tr2, _) = graph(t_a), graph(t_b)
        pa, na, oka = O.sample_negatives(tr, bt, E, n, mode, key, max_draws)
        _, nb_, _ = O.sample_negatives(tr2, bt, E, n, mode, key, max_draws)
        if np.array_equal(na[1], nb_[1]):
            want = (pa, na, oka)
            break
    assert want is not None and want[2].all()
    assert (want[1][4] == 123).all()  # the single allowed entity
    tl = TrueLists(tr, E, 5)
    off0, len0, ids0 = (np.array(x) for x in tl.lists(mode))
    len0[bt[1]] = 0
    what = f"sample_negatives n{n}"

    def run(guarded):
        b = Bufs(guarded)
        triples, batch_ = b.inp("triples", tr), b.inp("batch", bt)
        off = b.inp("true_off", off0)
        ln = b.inp("true_len", len0.astype(np.int32))
        ids = b.inp("true_ids", ids0)
        w = b.inp("weights", tl.weights)
        po, no, wo = b.out("pos_out", (B, 3), I64), b.out("neg_out", (B, n), I64), b.out("w_out", B, F32)
        if not guarded:
            ops.sample_negatives(triples, batch_, E, n, off, ln, ids, w, key, max_draws, po, no, wo)
        else:
            ok(lib().kge_sample_negatives(triples.data_ptr(), len(tr), batch_.data_ptr(), B, E, n, off.data_ptr(),
                                          ln.data_ptr(), ids.data_ptr(), w.data_ptr(), key, max_draws, po.data_ptr(),
                                          no.data_ptr(), wo.data_ptr(), b.err(), stream()), what)
        b.verify(what)
        return po.cpu(), no.cpu(), wo.cpu()

    got, mirror = run(True), run(False)
    assert all(same(x, y) for x, y in zip(got, mirror)), what
    assert np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[1].numpy(), want[1]), what
    assert np.array_equal(got[2].numpy(), tl.weights[bt]), what
