"""The kernels on entity tables past 2 GiB, 4 GiB and 2^31 floats (GPU box).

Tables, id lists and references are tests/big_table_cases.py's (pooled rows:
the table is pool[idx], built on the device by one index_select; the CPU
reference works on the 8192 pool rows and expands through idx; its own checks
are tests/test_big_table_ref.py).  Sizes (rows x floats per row): S2 540,000 x
1000 (past 2^31 bytes, and the fp32 MFMA tile's former 0x7FFFFFF0 sentinel),
S4 1,080,000 x 1000, S4odd 1,080,000 x 1001, S4wide 530,000 x 2051 (past 2^32
bytes), S8 2,100,000 x 1024 (past 2^31 floats).  Every id list takes at least
half of its entries from rows past the 2^31-byte line and holds row 0, row
E - 1 and the three rows around every line the table crosses.

  ranking   rank_filtered (both modes, every path the table admits) and
            rank_filtered_both: ranks and ties equal to the pooled reference
            (the reference's fp32 score order) and equal between paths; a path
            the table does not admit is KGE_ERR_ARG before any launch, the
            error flag 0 and the outputs untouched.  `listed` is equal between
            paths too: these queries list their true row's copies and little
            else.  (It is a property of the path in general: every fast pass
            has a window of its own, k_rank_window, and mid-ranked queries on
            these tables list 278 candidates on the register tile and 15,899
            on the wave scan; see the end of this docstring.)
  sentinel  S2 DistMult with +-3e38 in the 16 bytes at table offset
            0x7FFFFFF0, on mfma32 and the other paths.
  top-k     topk (tile and scan), the acceptance checks of
            tests/topk_cases.py on the expanded fp64 scores, and each
            returned pool row's copies being its lowest unexcluded ids.
  gathers   score in its three modes (score_tol of fp64), rank_candidates and
            rank_relations (exact; relation scores by score_tol).
  training  kge_train_step_grads and kge_score_backward, kge_train_step,
            kge_train_step_lazy, kge_train_step_adagrad (row-wise and
            element-wise state).  Reference: the compacted problem (the sorted
            unique touched ids mapped to 0..U-1) in the fp64 oracle, gradient
            rows by test_slot_matrix_ref's criterion (ratio <= 1 with
            rtol_case from the fp32 oracle's own distance to fp64).  The same
            entry on the compacted table on the device must give the same
            bits (regularization 0) in losses and touched rows of gradient,
            parameters and state; the optimizer entries' compacted run is in
            turn the composed reference (gradients, then kge_adam_step / the
            numpy Adagrad rule of tests/adagrad_cases.py) bit for bit.
            Untouched rows, in chunks regenerated from pool and idx:
            parameters bit-unchanged, gradient, moments and state exactly 0
            (S4 DistMult with regularization 1e-4: the regulariser's own
            gradient 3 r e |e|, and its loss terms by score_tol).
  dense     kge_adam_step / kge_adagrad_step on 2^30 + 1027 elements: the
            head, the elements around the 2^32-byte line and the tail
            against the same entry on small copies, bit for bit (the line
            lies 1027 elements before the end, so one window of 4096 holds
            both); everything between against the torch formula, in chunks.

Out of scope: pRotatE ranking (its phase tables double the table in the
workspace, and its exact ranks need the host sin of the three-call form); the
2^32-element line at 16 GiB and above; kge_ship_step and the
kge_train_step_from_rows* family; graph capture; any sensitivity build that
miscomputes an address on the GPU (a wrapped or negative offset can leave the
allocation: test_big_table_ref.py's wrapped-offset check stands in for it).

A test skips, naming its need and the free amount, only when
torch.cuda.mem_get_info() reports less free memory than it needs.

Recorded on an MI355X, one run of this module (37 s in all, nothing skipped;
288 GB card, the largest need 17 GiB).  Wall time per test (--durations):

    ranking    S2 DistMult 1.1 s, S2 ComplEx 0.7, S4 DistMult 0.7, S4 TransE 0.7,
               S4 RotatE 1.0, S4odd TransE 1.0, S4wide TransE 2.5, S8 TransE 2.2,
               S8 RotatE 1.8; sentinel 7.9 (below)
    top-k      S4 TransE 1.4 s, S4 DistMult 1.4, S8 RotatE 7.8 (nearly all of it the
               CPU side: fp64 pool scores and check_result's sort of [4, 2.1e6]
               scores; TOPK_NQ = 4 of the 16 queries for that reason)
    gathers    S8 TransE 0.1 s, S8 RotatE 0.7, S4wide TransE 0.2
    training   every case under 1.2 s
    dense      kge_adam_step 0.2 s, kge_adagrad_step 0.1

Peak device memory while each table was alive: S2 2.06 GiB, S4 16.74 (the
dense fused Adam step: table, gradient, two moments), S4odd 8.70, S4wide 9.32,
S8 8.67; kge_adam_step 16.38, kge_adagrad_step 12.38.  Every test asserts
its peak <= 20 GiB.

Training, worst kernel ratio per case (err / (rtol_case * rowmax + floor), the
criterion is ratio <= 1) and rho_case:

    grads S4 RotatE tail-batch, hot bucket      8.26e-06   0.084  (backward, entity)
    grads S4 DistMult head-batch, reg 1e-4      2.52e-07   0.143  (train, entity)
    grads S4odd TransE head-batch, n = 3        8.66e-06   0.016  (train, entity)
    grads S4wide TransE tail-batch              2.47e-05   0.008  (train, entity)
    kge_train_step S4 RotatE                    5.38e-06   0.131  (entity)
    kge_train_step_lazy S4 RotatE               6.19e-06   0.150  (entity)
    adagrad row-wise S8 TransE, hot bucket      1.57e-05   0.007  (entity; G' at 0.005 of rowsum_bound)
    adagrad row-wise S8 RotatE                  4.78e-06   0.126  (entity; G' at 0.002 of rowsum_bound)
    adagrad element-wise S4 RotatE              5.38e-06   0.131  (entity)

Every bit comparison held: no quantity needed the fp64 criterion in place of
bit equality with the compacted run.  The dense entries between their windows
were bit-equal to the torch formula (ratio 0.000 of the bound).

Near-tie lists (`listed`, max over the queries): 71 ... 297 on every path, the
true row's copies and a few others.  A first version of the cases took the
true rows from the drawn pool: at the init range a mid-ranked query then lists
2,800 ... 33,700 candidates (0.5 % ... 4.6 % of the table, the wave scan's
window the widest), overflows the 1024 cap and takes k_rank_exact's rescan of
all E candidates.  All ranks and ties were the reference's there too, on every
path and size, but a ranking call with 15 such queries took 3.5 s on S2, 25 s
on S4 and 45 s on S8: the rescan is the designed fallback for degenerate
tables and is slow at these sizes.  The sentinel case is the one test that
still takes it: the +-3e38 row's norm overflows the table statistics, every
window is infinite and every query lists all 540,032 padded candidates (7.9 s
for two calls); it ran on mfma32 only for that reason, with the ranks of the
reference, before and after OOB2 moved from 0x7FFFFFF0 to 0xFFFFFF10.
"""
import math

import numpy as np
import pytest
import torch

import adagrad_cases as A
import big_table_cases as C
import topk_cases as T
from conftest import score_tol
from knowledgegraphembedding_amd import _lib, ops
from test_slot_matrix_ref import ratio_of

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GIB = 1 << 30
PEAK_CAP = 20 * GIB
CHUNK = 1 << 16      # rows per chunk of the untouched-row checks
PEAK = {}            # table key -> peak bytes allocated while it was alive
RATIOS = {}          # training case id -> [worst kernel ratio, where, rho_case]
LISTED = []          # (case, mode, path, min, max of listed)
TOPK_NQ = 4          # queries of the top-k checks (their CPU side sorts [nq, E] float64 scores per call)
LR_ADAM, BETAS, EPS_ADAM = 3e-3, (0.9, 0.999), 1e-8


class Big:
    """One table on the device: pool, idx, the table, the relation table, the descriptor."""

    def __init__(self, sp):
        pool, rel = C.pool_of(sp)
        self.sp = sp
        self.pool = torch.from_numpy(np.array(pool)).to(DEV)
        self.idx = torch.from_numpy(np.array(C.idx_of(sp))).to(DEV)
        self.ent = torch.index_select(self.pool, 0, self.idx)
        self.rel = torch.from_numpy(np.array(rel)).to(DEV)
        assert self.ent.shape == (sp.table.E, sp.table.Le) and self.ent.data_ptr() % 16 == 0
        self.desc = ops.make_desc(sp.name, self.ent, self.rel, C.GAMMA, sp.erange, None)
        self.trig = ops.reference_rotation(self.rel, sp.erange).to(DEV) if sp.name == "RotatE" else None
        self.q = torch.from_numpy(np.array(C.queries(sp))).to(DEV)
        self._filt = {}

    def filt(self, mode):
        if mode not in self._filt:
            self._filt[mode] = tuple(torch.from_numpy(np.array(a)).to(DEV) for a in C.filters(self.sp, mode))
        return self._filt[mode]

    def rows(self, a, b):
        """Rows [a, b) regenerated from pool and idx."""
        return torch.index_select(self.pool, 0, self.idx[a:b])


_CUR = {}


def _note_peak():
    if _CUR:
        key = _CUR["big"].sp.table.key
        PEAK[key] = max(PEAK.get(key, 0), torch.cuda.max_memory_allocated(DEV))


def _free():
    _note_peak()
    _CUR.clear()
    st = ops.state(DEV)
    st.ws.clear()  # the shared workspace grew with the table
    st.rank_ws_ptr = 0
    torch.cuda.empty_cache()


def table(sp, extra=0.0):
    """The table of `sp`, the only big one alive.  `extra`: what the test allocates beside
    it, in units of the table's size."""
    if _CUR.get("sp") != sp:
        _free()
        need = int((1.0 + extra) * sp.table.nbytes) + GIB
        free = torch.cuda.mem_get_info(DEV)[0]
        if free < need:
            pytest.skip(f"{sp.id}: needs {need / GIB:.1f} GiB of device memory, {free / GIB:.1f} GiB are free")
        torch.cuda.reset_peak_memory_stats(DEV)
        _CUR.update(sp=sp, big=Big(sp))
    elif extra:
        need = int(extra * sp.table.nbytes) + GIB
        free = torch.cuda.mem_get_info(DEV)[0] + torch.cuda.memory_reserved(DEV) - torch.cuda.memory_allocated(DEV)
        if free < need:
            pytest.skip(f"{sp.id}: needs {need / GIB:.1f} GiB more device memory, {free / GIB:.1f} GiB are free")
    return _CUR["big"]


@pytest.fixture(scope="module", autouse=True)
def _tables():
    yield
    _free()
    print("\nbig tables: peak device memory while each table was alive")
    for key, b in PEAK.items():
        print("big tables: %-7s %.2f GiB" % (key, b / GIB))
    print("big tables: training case, rho_case, worst kernel ratio (where)")
    for cid, (ratio, where, rho) in RATIOS.items():
        print("big tables: %-44s %.3e  %.3f  (%s)" % (cid, rho, ratio, where))
    print("big tables: ranking case, mode, path, min / max listed")
    for row in LISTED:
        print("big tables: %-18s %-10s %-7s %5d %5d" % row)


@pytest.fixture(autouse=True)
def _after():
    yield
    try:
        torch.cuda.synchronize(DEV)
    except RuntimeError as exc:  # a GPU fault: nothing more is started on the device
        pytest.exit(f"GPU error after a big-table test: {exc}", returncode=3)
    ops.raise_on_device_error(DEV)
    _note_peak()
    assert torch.cuda.max_memory_allocated(DEV) <= PEAK_CAP


def _d(a, dtype=None):
    t = torch.from_numpy(np.array(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------- ranking
def _rank(b, mode, path):
    off, ids = b.filt(mode)
    r, t, l = ops.rank_filtered(b.desc, mode, b.q, off, ids, DEV, path=path, listed=True, relation_trig=b.trig)
    return _np(r), _np(t), _np(l)


def _check_ranks(sp, mode, got, what):
    want = C.rank_reference(sp, mode)
    bad = np.nonzero((got[0] != want[0]) | (got[1] != want[1]))[0]
    assert not len(bad), (f"{what}: queries {bad[:8]}: ranks {got[0][bad[:8]]} vs {want[0][bad[:8]]}, "
                          f"ties {got[1][bad[:8]]} vs {want[1][bad[:8]]}")


def _refused(b, mode, path):
    """The C entry itself on outputs of its own: KGE_ERR_ARG, the error flag 0, nothing written."""
    lib, st = _lib.load(), ops.state(DEV)
    nq = b.q.shape[0]
    off, ids = b.filt(mode)
    ranks = torch.full((nq,), -7, dtype=torch.int64, device=DEV)
    ties = torch.full((nq,), -7, dtype=torch.int32, device=DEV)
    listed = torch.full((nq,), -7, dtype=torch.int32, device=DEV)
    ws = st.workspace(lib.kge_rank_workspace_bytes(b.desc, nq))
    status = lib.kge_rank_filtered_ex(b.desc, _lib.MODE_IDS[mode], b.q.data_ptr(), nq, off.data_ptr(), ids.data_ptr(),
                                      ranks.data_ptr(), ties.data_ptr(), listed.data_ptr(), ops.RANK_PATHS[path],
                                      ws.data_ptr(), ws.numel(), st.err.data_ptr(),
                                      torch.cuda.current_stream(DEV).cuda_stream)
    assert status == 4, (path, status)  # KGE_ERR_ARG
    assert int(st.err.item()) == 0
    assert bool((ranks == -7).all()) and bool((ties == -7).all()) and bool((listed == -7).all())
    with pytest.raises(_lib.KGEHipError, match="status 4"):
        ops.rank_filtered(b.desc, mode, b.q, off, ids, DEV, path=path, relation_trig=b.trig)


def _rank_case(sp, paths, refused, both=True):
    b = table(sp, extra=0.1)
    for mode in C.MODES:
        first = None
        for path in paths:
            got = _rank(b, mode, path)
            LISTED.append((sp.id, mode, path, int(got[2].min()), int(got[2].max())))
            _check_ranks(sp, mode, got, f"{sp.id} {mode} {path}")
            first = first or got
            assert all(np.array_equal(x, y) for x, y in zip(got, first)), (sp.id, mode, path, got[2], first[2])
        for path in refused:
            _refused(b, mode, path)
    for path in (paths[0], "auto") if both else ():
        r, t, _ = ops.rank_filtered_both(b.desc, b.q, b.filt("head-batch"), b.filt("tail-batch"), DEV, path=path,
                                         listed=True, relation_trig=b.trig)
        r, t, nq = _np(r), _np(t), b.q.shape[0]
        for k, mode in enumerate(C.MODES):
            _check_ranks(sp, mode, (r[k * nq:(k + 1) * nq], t[k * nq:(k + 1) * nq]), f"{sp.id} both/{mode} {path}")


@pytest.mark.parametrize("sp", list(C.RANK_CASES), ids=lambda sp: sp.id)
def test_ranking(sp):
    paths, refused = C.RANK_CASES[sp]
    _rank_case(sp, paths, refused)


def test_ranking_sentinel():
    """+-3e38 in the 16 bytes at table offset 0x7FFFFFF0 (the fp32 MFMA tile's "no row" /
    "past K" offset until it moved past every admitted buffer): the ranks are the
    reference's on mfma32 and on every other path."""
    sp = C.SENTINEL_CASE
    b = table(sp, extra=0.1)
    row, col = divmod(C.SENTINEL // 4, sp.table.Le)
    assert bool((b.ent.view(-1)[C.SENTINEL // 4:C.SENTINEL // 4 + 4].abs() == C.HUGE).all())
    assert bool((b.ent[row, col:col + 4].abs() == C.HUGE).all())
    _rank_case(sp, ("mfma32",), ("mfma",), both=False)


# --------------------------------------------------------------------- top-k
def _lowest_ids_first(sp, ids, mask):
    """Every returned pool row's copies are its lowest unexcluded ids."""
    idx = C.idx_of(sp)
    for i in range(len(ids)):
        got = ids[i][ids[i] >= 0]
        for p in np.unique(idx[got])[:24]:
            members = np.nonzero((idx == p) & ~mask[i])[0]
            mine = np.sort(got[idx[got] == p])
            assert np.array_equal(mine, members[:len(mine)]), f"q{i} pool row {p}: {mine} vs {members[:len(mine)]}"


@pytest.mark.parametrize("sp", C.TOPK_CASES, ids=lambda sp: sp.id)
def test_topk(sp):
    b = table(sp, extra=0.1)
    q = b.q[:TOPK_NQ]
    idx = C.idx_of(sp)
    for mode, k in zip(C.MODES, C.KS):
        off, ids = b.filt(mode)
        s64 = C.pool_s64(sp, mode, None, TOPK_NQ)[:, idx]
        mask = C.filter_mask(sp, mode, TOPK_NQ)
        for path in ("tile", "scan"):
            oi, os_ = ops.topk(b.desc, mode, q, k, DEV, filt=(off[:TOPK_NQ + 1], ids), path=path)
            oi, os_ = _np(oi), _np(os_)
            T.check_result(oi, os_, s64, mask, k, True, f"{sp.id} {mode} k={k} {path}")
            _lowest_ids_first(sp, oi, mask)


# ------------------------------------------------------------------- gathers
@pytest.mark.parametrize("sp", C.GATHER_CASES, ids=lambda sp: sp.id)
def test_gathers(sp):
    b = table(sp, extra=0.1)
    neg = _d(C.negatives(sp))
    for mode in ("single",) + C.MODES:
        s = _np(ops.score(b.desc, mode, b.q, None if mode == "single" else neg, DEV))
        ref = C.score_reference(sp, mode)
        assert s.shape == ref.shape and np.isfinite(s).all()
        assert (np.abs(s - ref) <= score_tol(ref)).all(), f"{sp.id} score {mode}: {np.abs(s - ref).max():.3e}"
    for mode in C.MODES:
        r, t = ops.rank_candidates(b.desc, mode, b.q, _d(C.candidates(sp, mode)), DEV, relation_trig=b.trig)
        want = C.candidates_reference(sp, mode)
        assert np.array_equal(_np(r), want[0]) and np.array_equal(_np(t), want[1]), (sp.id, mode, _np(r), want[0])
    r, t, s = ops.rank_relations(b.desc, b.q, DEV, relation_trig=b.trig, scores=True)
    wr, wt, _, s64 = C.relations_reference(sp)
    assert np.array_equal(_np(r), wr) and np.array_equal(_np(t), wt), (sp.id, _np(r), wr)
    assert (np.abs(_np(s) - s64) <= score_tol(s64)).all()


# ------------------------------------------------------------------ training
def _bits_equal(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def _note_ratio(tc, got, g64, ref, where, fails):
    g = _np(got)
    ratio = ratio_of(g, g64, ref.rtol) if np.isfinite(g).all() else math.inf
    print(f"{tc.id} {where}: rho_case {ref.rho:.3e} rtol_case {ref.rtol:.3e} ratio {ratio:.3f}")
    w = RATIOS.setdefault(tc.id, [0.0, "", ref.rho])
    if ratio > w[0]:
        w[0], w[1] = ratio, where
    if not ratio <= 1.0:
        fails.append(f"{where}: ratio {ratio:.3f} (rtol_case {ref.rtol:.3e})")


def _untouched(b, uniq_d, fails, params=True, zero=(), reg=0.0, grad=None):
    """Every row outside uniq, in chunks: the table bit-equal to pool[idx]; the `zero`
    tensors ([E, Le] or [E]) exactly 0; with a regulariser, `grad` its own gradient."""
    E = b.sp.table.E
    touched = torch.zeros(E, dtype=torch.bool, device=DEV)
    touched[uniq_d] = True
    bad = {"param": 0, "zero": 0, "reg": 0}
    for a in range(0, E, CHUNK):
        e = min(a + CHUNK, E)
        keep = ~touched[a:e]
        want = b.rows(a, e)
        if params:
            bad["param"] += int(((b.ent[a:e].view(torch.int32) != want.view(torch.int32)).any(1) & keep).sum())
        for z in zero:
            nz = (z[a:e] != 0) | torch.isnan(z[a:e])
            bad["zero"] += int(((nz.any(1) if nz.dim() > 1 else nz) & keep).sum())
        if reg:
            wg = 3.0 * reg * want * want.abs()
            tol = 1e-5 * wg.abs().amax(1, keepdim=True)
            bad["reg"] += int((~((grad[a:e] - wg).abs() <= tol).all(1) & keep).sum())
    for k, n in bad.items():
        if n:
            fails.append(f"untouched rows: {n} rows fail the {k} check")


def _train_args(tc):
    return dict(adversarial=True, temperature=C.ADV_T, uni_weight=False, regularization=tc.regularization)


def _check_losses(tc, losses, ref, fails, where):
    want = ref.losses.copy()
    got = _np(losses)[:4].astype(np.float64)
    if tc.regularization:
        reg = C.reg_reference(tc.spec, tc.regularization)
        want[2] += reg
        if not abs(got[3] - reg) <= score_tol(reg):
            fails.append(f"{where}: regularization {got[3]} vs {reg}")
    if not (np.isfinite(got[:3]).all() and (np.abs(got[:3] - want) <= score_tol(want)).all()):
        fails.append(f"{where}: losses {got[:3]} vs {want}")


@pytest.mark.parametrize("tc", C.GRAD_CASES, ids=lambda tc: tc.id)
def test_train_grads_and_backward(tc):
    sp = tc.spec
    b = table(sp, extra=1.1)
    ref = C.train_reference(tc)
    fails = []
    uniq = _d(ref.uniq)
    pos, neg, w = (_d(a) for a in C.train_batch(sp, tc.n, tc.hot))
    posc, negc = _d(ref.pos), _d(ref.neg)
    ent_c = b.ent[uniq].contiguous()
    assert _bits_equal(ent_c, _d(ref.ent))
    desc_c = ops.make_desc(sp.name, ent_c, b.rel, C.GAMMA, sp.erange, None)

    def grads(desc, p, n_, rows):
        ge = torch.full((rows, sp.table.Le), math.nan, device=DEV)
        gr = torch.full_like(b.rel, math.nan)
        losses = torch.full((5,), math.nan, device=DEV)
        ops.train_step_grads(desc, tc.mode, p, n_, w, DEV, grad_entity=ge, grad_relation=gr, grad_modulus=None,
                             losses=losses, **_train_args(tc))
        return ge, gr, losses

    ge, gr, losses = grads(b.desc, pos, neg, sp.table.E)
    gec, grc, lossc = grads(desc_c, posc, negc, len(ref.uniq))
    _check_losses(tc, losses, ref, fails, "train")
    _note_ratio(tc, ge[uniq], ref.grads[0], ref, "train entity", fails)
    _note_ratio(tc, gr, ref.grads[1], ref, "train relation", fails)
    if not tc.regularization:
        for nm, x, y in (("losses", losses[:4], lossc[:4]), ("entity", ge[uniq], gec), ("relation", gr, grc)):
            if not _bits_equal(x, y):
                fails.append(f"train {nm}: the big table's bits differ from the compacted table's")
        _untouched(b, uniq, fails, zero=(ge,))
    else:
        _untouched(b, uniq, fails, reg=tc.regularization, grad=ge)
    del ge, gec

    gout = _d(ref.gout[tc.mode])
    ge, gr, _ = ops.score_backward(b.desc, tc.mode, pos, neg, gout, DEV, False)
    gec, grc, _ = ops.score_backward(desc_c, tc.mode, posc, negc, gout, DEV, False)
    _note_ratio(tc, ge[uniq], ref.backward[tc.mode][0], ref, "backward entity", fails)
    _note_ratio(tc, gr, ref.backward[tc.mode][1], ref, "backward relation", fails)
    for nm, x, y in (("entity", ge[uniq], gec), ("relation", gr, grc)):
        if not _bits_equal(x, y):
            fails.append(f"backward {nm}: the big table's bits differ from the compacted table's")
    _untouched(b, uniq, fails, zero=(ge,))
    assert not fails, "\n".join([tc.id] + fails)


def _adam_desc(ent, rel, st):
    d = _lib.AdamDesc()
    d.beta1, d.beta2, d.eps, d.write_grad = BETAS[0], BETAS[1], EPS_ADAM, 1
    for field, p in (("entity", ent), ("relation", rel)):
        t = getattr(d, field)
        t.param, t.exp_avg, t.exp_avg_sq = p.data_ptr(), st[field][0].data_ptr(), st[field][1].data_ptr()
        t.step_size, t.bias_correction2_sqrt = LR_ADAM / (1 - BETAS[0]), math.sqrt(1 - BETAS[1])
    return d


def _adagrad_desc(ent, rel, st, rowwise):
    d = _lib.AdagradDesc()
    d.lr, d.eps, d.entity_rowwise, d.write_grad = A.LR, A.EPS, int(rowwise), 1
    for field, p in (("entity", ent), ("relation", rel)):
        t = getattr(d, field)
        t.param, t.state_sum = p.data_ptr(), st[field][0].data_ptr()
    return d


def _step(tc, sp, ent, rel, pos, neg, w):
    """One fused optimizer step of the case's entry on (ent, rel) in place from zero state.
    Returns (losses, entity gradient or None, relation gradient, state: field -> tensors)."""
    rows, Le = ent.shape
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    desc = ops.make_desc(sp.name, ent, rel, C.GAMMA, sp.erange, None)
    gr = torch.full_like(rel, math.nan)
    losses = torch.full((5,), math.nan, device=DEV)
    ge = torch.full((rows, Le), math.nan, device=DEV) if tc.entry == "adam" else None
    kw = dict(grad_entity=ge, grad_relation=gr, grad_modulus=None, losses=losses, **_train_args(tc))
    if tc.entry in ("adam", "lazy"):
        st = {"entity": (z(rows, Le), z(rows, Le)), "relation": (z(*rel.shape), z(*rel.shape))}
        ops.train_step_grads(desc, tc.mode, pos, neg, w, DEV, adam=_adam_desc(ent, rel, st), lazy=tc.entry == "lazy", **kw)
    else:
        rowwise = tc.entry == "adagrad-row"
        st = {"entity": (z(rows) if rowwise else z(rows, Le),), "relation": (z(*rel.shape),)}
        ops.train_step_grads(desc, tc.mode, pos, neg, w, DEV, adagrad=_adagrad_desc(ent, rel, st, rowwise), **kw)
    return losses, ge, gr, st


def _composed(tc, sp, ref, ent_c, rel, posc, negc, w, got, fails):
    """The compacted run `got` against gradients + the optimizer's own rule, bit for bit;
    the gradients against fp64 (every compacted row is touched, so lazy = dense here)."""
    pe, pr, st = got
    ge = torch.full_like(ent_c, math.nan)
    gr = torch.full_like(rel, math.nan)
    losses = torch.full((5,), math.nan, device=DEV)
    desc = ops.make_desc(sp.name, ent_c, rel, C.GAMMA, sp.erange, None)
    ops.train_step_grads(desc, tc.mode, posc, negc, w, DEV, grad_entity=ge, grad_relation=gr, grad_modulus=None,
                         losses=losses, **_train_args(tc))
    _check_losses(tc, losses, ref, fails, "composed")
    _note_ratio(tc, ge, ref.grads[0], ref, f"{tc.entry} entity", fails)
    _note_ratio(tc, gr, ref.grads[1], ref, f"{tc.entry} relation", fails)
    for field, p0, g, p1 in (("entity", ent_c, ge, pe), ("relation", rel, gr, pr)):
        if tc.entry in ("adam", "lazy"):
            p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
            ops.adam_step(p, g.contiguous(), m, v, step=1, lr=LR_ADAM, beta1=BETAS[0], beta2=BETAS[1], eps=EPS_ADAM)
            same = _bits_equal(p, p1) and _bits_equal(m, st[field][0]) and _bits_equal(v, st[field][1])
        elif tc.entry == "adagrad-row" and field == "entity":
            G1 = _np(st[field][0])
            same = np.array_equal(A.adagrad_move_ref(_np(p0), _np(g), G1).view(np.int32), _np(p1).view(np.int32))
            g64 = _np(g).astype(np.float64)
            G64 = (g64 * g64).sum(1) / g64.shape[1]
            err, bound = np.abs(G1 - G64), A.rowsum_bound(G64, g64.shape[1])
            print(f"{tc.id}: max |G' - G'_f64| / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
            same = same and bool((err <= bound).all())
        else:
            p, s = A.adagrad_elem_ref(_np(p0), _np(g), np.zeros(p0.shape, dtype=np.float32))
            same = (np.array_equal(p.view(np.int32), _np(p1).view(np.int32))
                    and np.array_equal(s.view(np.int32), _np(st[field][0]).view(np.int32)))
        if not same:
            fails.append(f"{tc.entry} {field}: the compacted run differs from gradients + the optimizer's rule")


@pytest.mark.parametrize("tc", C.STEP_CASES, ids=lambda tc: tc.id)
def test_train_steps(tc):
    sp = tc.spec
    extra = {"adam": 3.1, "lazy": 2.1, "adagrad-elem": 1.1, "adagrad-row": 0.1}[tc.entry]
    b = table(sp, extra=extra)
    ref = C.train_reference(tc, backward=False)
    fails = []
    uniq = _d(ref.uniq)
    pos, neg, w = (_d(a) for a in C.train_batch(sp, tc.n, tc.hot))
    posc, negc = _d(ref.pos), _d(ref.neg)
    ent_c0 = b.ent[uniq].contiguous()
    assert _bits_equal(ent_c0, _d(ref.ent))
    ent_c, rel_c, rel_b = ent_c0.clone(), b.rel.clone(), b.rel.clone()
    try:
        losses, ge, gr, st = _step(tc, sp, b.ent, rel_b, pos, neg, w)       # moves the shared table's touched rows
        lossc, gec, grc, stc = _step(tc, sp, ent_c, rel_c, posc, negc, w)
        _check_losses(tc, losses, ref, fails, tc.entry)
        pairs = [("losses", losses[:4], lossc[:4]), ("entity", b.ent[uniq], ent_c), ("relation", rel_b, rel_c),
                 ("relation gradient", gr, grc)]
        pairs += [(f"entity state {k}", x[uniq], y) for k, (x, y) in enumerate(zip(st["entity"], stc["entity"]))]
        pairs += [(f"relation state {k}", x, y) for k, (x, y) in enumerate(zip(st["relation"], stc["relation"]))]
        if ge is not None:
            pairs.append(("entity gradient", ge[uniq], gec))
        for nm, x, y in pairs:
            if not _bits_equal(x, y):
                fails.append(f"{tc.entry} {nm}: the big table's bits differ from the compacted table's")
        if _bits_equal(b.ent[uniq], ent_c0):
            fails.append(f"{tc.entry}: the step moved no touched row")
        _untouched(b, uniq, fails, zero=tuple(st["entity"]) + ((ge,) if ge is not None else ()))
        del ge, st
        _composed(tc, sp, ref, ent_c0, b.rel, posc, negc, w, (ent_c, rel_c, stc), fails)
    finally:
        b.ent[uniq] = torch.index_select(b.pool, 0, b.idx[uniq])  # the shared table as it was
    assert not fails, "\n".join([tc.id] + fails)


# --------------------------------------------------- dense optimizer entries
NUMEL = 2 ** 30 + 1027          # the byte offsets cross 2^32
FILL = 1 << 24                  # elements per chunk
WINDOWS = ((0, 4096), (NUMEL - 4096, NUMEL))  # the head; the last 4096 elements: the line (element 2^30) and the tail


def _hash01(a, e, mult):
    """Pseudo-random floats in [0, 1) as a function of the element index: any chunk can be regenerated."""
    i = torch.arange(a, e, dtype=torch.int64, device=DEV)
    return (((i * mult + 12345) >> 7) & 0xFFFFFF).to(torch.float32) / float(1 << 24)


GEN = {"p": lambda a, e: (_hash01(a, e, 2654435761) - 0.5) * 0.03,
       "g": lambda a, e: (_hash01(a, e, 40503 * 65537 + 2) - 0.5) * 0.02,
       "m": lambda a, e: (_hash01(a, e, 2246822519) - 0.5) * 0.01,
       "v": lambda a, e: _hash01(a, e, 3266489917) * 1e-4 + 1e-8}


def _filled(kind):
    t = torch.empty(NUMEL, device=DEV)
    for a in range(0, NUMEL, FILL):
        e = min(a + FILL, NUMEL)
        t[a:e] = GEN[kind](a, e)
    return t


def _need(nbytes, what):
    _free()
    free = torch.cuda.mem_get_info(DEV)[0]
    if free < nbytes:
        pytest.skip(f"{what}: needs {nbytes / GIB:.1f} GiB of device memory, {free / GIB:.1f} GiB are free")
    torch.cuda.reset_peak_memory_stats(DEV)


def _between(check):
    """check(a, e) on every chunk of the elements outside the windows."""
    edges = [0] + [x for w in WINDOWS for x in w] + [NUMEL]
    for lo, hi in zip(edges[1::2], edges[2::2]):
        for a in range(lo, hi, FILL):
            check(a, min(a + FILL, hi))


def test_adam_step_past_4gib():
    _need(4 * NUMEL * 4 + 2 * GIB, "kge_adam_step")
    step = 3
    kw = dict(step=step, lr=LR_ADAM, beta1=BETAS[0], beta2=BETAS[1], eps=EPS_ADAM)
    big = {k: _filled(k) for k in "pgmv"}
    small = [{k: big[k][a:e].clone() for k in "pgmv"} for a, e in WINDOWS]
    ops.adam_step(big["p"], big["g"], big["m"], big["v"], **kw)
    for (a, e), s in zip(WINDOWS, small):
        ops.adam_step(s["p"], s["g"], s["m"], s["v"], **kw)
        for k in "pmv":
            assert _bits_equal(big[k][a:e], s[k]), f"window [{a}, {e}) {k}"
        assert _bits_equal(big["g"][a:e], s["g"])
    f32 = lambda x: torch.tensor(x, dtype=torch.float32, device=DEV)  # noqa: E731
    step_size, bc2s = f32(LR_ADAM / (1 - BETAS[0] ** step)), f32(math.sqrt(1 - BETAS[1] ** step))
    worst = [0.0, 0.0]

    def check(a, e):
        p, g, m, v = (GEN[k](a, e) for k in "pgmv")
        # adam_elem's formula (kge_device.h; 1 - beta in fp32); 16 roundings of slack as in
        # adagrad_cases' bounds, the first moment's relative to |m| + |g| (m' may cancel)
        m1 = m + (f32(1.0) - f32(BETAS[0])) * (g - m)
        v1 = v * f32(BETAS[1]) + (f32(1.0) - f32(BETAS[1])) * (g * g)
        denom = v1.sqrt() / bc2s + f32(EPS_ADAM)
        p1 = p + (-step_size) * (m1 / denom)
        mb = 2.0 ** -22 * (m.abs() + g.abs())
        bound = 2.0 ** -22 * p1.abs() + 2.0 ** -20 * step_size * (m.abs() + g.abs()) / denom
        worst[0] = max(worst[0], float(((big["p"][a:e] - p1).abs() / bound).max()))
        worst[1] = max(worst[1], float(((big["m"][a:e] - m1).abs() / mb).max()),
                       float(((big["v"][a:e] - v1).abs() / (2.0 ** -22 * v1)).max()))
        assert bool(torch.equal(big["g"][a:e], g))

    _between(check)
    print(f"kge_adam_step between the windows: max |dp| / bound {worst[0]:.3f}, moments {worst[1]:.3f}")
    PEAK["adam_step"] = torch.cuda.max_memory_allocated(DEV)
    assert worst[0] <= 1.0 and worst[1] <= 1.0


def test_adagrad_step_past_4gib():
    _need(3 * NUMEL * 4 + 2 * GIB, "kge_adagrad_step")
    big = {"p": _filled("p"), "g": _filled("g"), "s": _filled("v")}
    small = [{k: big[k][a:e].clone() for k in "pgs"} for a, e in WINDOWS]
    ops.adagrad_step(big["p"], big["g"], big["s"], lr=A.LR, eps=A.EPS)
    for (a, e), s in zip(WINDOWS, small):
        ops.adagrad_step(s["p"], s["g"], s["s"], lr=A.LR, eps=A.EPS)
        for k in "pgs":
            assert _bits_equal(big[k][a:e], s[k]), f"window [{a}, {e}) {k}"
    worst = [0.0, 0.0]
    lr, eps = np.float32(A.LR), np.float32(A.EPS)

    def check(a, e):
        p, g, s = GEN["p"](a, e), GEN["g"](a, e), GEN["v"](a, e)
        s1 = s + g * g
        std = s1.sqrt() + float(eps)
        p1 = p + (-float(lr)) * (g / std)
        bound = 2.0 ** -22 * p1.abs() + 2.0 ** -20 * float(lr) * g.abs() / std  # adagrad_cases.p_bound
        worst[0] = max(worst[0], float(((big["p"][a:e] - p1).abs() / bound).max()))
        worst[1] = max(worst[1], float(((big["s"][a:e] - s1).abs() / (2.0 ** -22 * s1)).max()))  # sum_bound
        assert bool(torch.equal(big["g"][a:e], g))

    _between(check)
    print(f"kge_adagrad_step between the windows: max |dp| / bound {worst[0]:.3f}, |dsum| / bound {worst[1]:.3f}")
    PEAK["adagrad_step"] = torch.cuda.max_memory_allocated(DEV)
    assert worst[0] <= 1.0 and worst[1] <= 1.0
