"""kge_rank_shard_fast on the device, one process playing every rank through ops
(the Shards pattern of test_rank_shard_gpu.py): the fast entry's counts equal the
exact stage's (ops.rank_shard_count) on every shard, bit for bit, on every path
the shard's rows admit — and the path is asserted (ops.rank_shard_fast_path), so
a silent fallback to the exact kernel cannot pass for the fast pass.

Against the fp32 reference-order oracle (rank_shard_cases.shard_counts) the four
exact models match exactly: the planted exact ties and one-float nudges on both
sides of every shard boundary decide the window (TransE on the register tile
runs with a zero window).  The near-tie ladders of rank_tie_cases put 1023, 1024
and 1025 listed candidates into one shard: the list's cap.
"""
import numpy as np
import pytest
import torch

import rank_shard_cases as S
import rank_tie_cases as T
from knowledgegraphembedding_amd import ops
from test_slot_matrix_gpu import unaligned

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
WORLDS = ("w1", "w2", "w3", "w4")
MFMA, TILE, EXACT = 1, 2, 3
PATH_NAME = {MFMA: "mfma", TILE: "tile", EXACT: "exact"}


class Parts:
    """Tables on the device, one tensor and descriptor per row range (each shard a tensor of its
    own rows alone, the descriptor's entity pointer own_begin rows before it)."""

    def __init__(self, name, tables, gamma, ranges, aligned=True):
        ent, rel, mod, erange = tables
        self.name, self.ranges, self.E = name, ranges, ent.shape[0]
        self.rel = torch.from_numpy(rel.copy()).to(DEV)
        self.mod = None if mod is None else torch.from_numpy(mod.copy()).to(DEV)
        self.trig = ops.reference_rotation(self.rel, erange).to(DEV) if name == "RotatE" else None
        self.le = ent.shape[1]
        self.rows, self.descs = [], []
        for b, e in ranges:
            t = torch.from_numpy(ent[b:max(e, b + 1)].copy()).to(DEV)  # (an empty shard: one row that is never read)
            if not aligned:
                t = unaligned(t)
            assert (t.data_ptr() % 16 == 0) == aligned
            d = ops.make_desc(name, t, self.rel, gamma, erange, self.mod)
            d.entity_embedding = t.data_ptr() - b * self.le * 4
            d.nentity = self.E
            self.rows.append(t)
            self.descs.append(d)

    def reduce(self, mode, q):
        """ROWS and TRUE over every shard, summed as the all-reduces would: (fixed_rows, s_true)."""
        nq = q.shape[0]
        fixed = torch.zeros(nq, self.le, dtype=torch.int32, device=DEV)
        for d, own in zip(self.descs, self.ranges):
            part = torch.empty(nq, self.le, device=DEV)
            ops.rank_shard_rows(d, mode, q, own, DEV, part)
            fixed += part.view(torch.int32)
        fixed = fixed.view(torch.float32)
        st = torch.zeros(nq, dtype=torch.int32, device=DEV)
        for d, own in zip(self.descs, self.ranges):
            part = torch.empty(nq, device=DEV)
            ops.rank_shard_true(d, mode, q, own, DEV, fixed, part, relation_trig=self.trig)
            st += part.view(torch.int32)
        return fixed, st.view(torch.float32)

    def exact(self, mode, q, fixed, st, filt, table):
        out = []
        for d, own in zip(self.descs, self.ranges):
            c = torch.empty(2, q.shape[0], dtype=torch.int64, device=DEV)
            ops.rank_shard_count(d, mode, q, own, DEV, fixed, st, filt, c, filter_table=table, relation_trig=self.trig)
            out.append(c)
        return torch.stack(out).cpu().numpy()

    def path(self, i, path="auto", fixed=None):
        return ops.rank_shard_fast_path(self.descs[i], self.ranges[i], path, fixed_rows=fixed, relation_trig=self.trig)

    def fast(self, mode, q, fixed, st, filt, table, path="auto"):
        """The fast entry on every shard: (counts [world, 2, nq], listed [world, nq]) on the host.
        Outputs start poisoned: the entry writes every place."""
        nq = q.shape[0]
        cs, ls = [], []
        for d, own in zip(self.descs, self.ranges):
            c = torch.full((2, nq), -7, dtype=torch.int64, device=DEV)
            l = torch.full((nq,), -7, dtype=torch.int32, device=DEV)
            ops.rank_shard_count_fast(d, mode, q, own, DEV, fixed, st, filt, c, filter_table=table, path=path,
                                      relation_trig=self.trig, listed=l)
            cs.append(c)
            ls.append(l)
        return torch.stack(cs).cpu().numpy(), torch.stack(ls).cpu().numpy()


def shards(case, world):
    return Parts(case.name, S.tables(case), S.GAMMA, S.splits(case.E)[world], case.aligned)


def expected_auto(case):
    """The path "auto" must take on every shard of the case (each shard a 16-byte aligned tensor unless
    the case says otherwise): rank_path's rules on the shard's view, pRotatE and wide rows on the exact kernel."""
    if not case.aligned or case.name == "pRotatE" or case.d > 2048:
        return EXACT
    if case.name in ("DistMult", "ComplEx"):
        return MFMA
    return TILE if case.d % 4 == 0 else EXACT


def explicit_paths(case):
    """The explicit paths the case's shards admit (exact: everywhere)."""
    auto = expected_auto(case)
    if auto == MFMA:
        return (MFMA, TILE, EXACT) if case.d % 4 == 0 else (MFMA, EXACT)
    return (TILE, EXACT) if auto == TILE else (EXACT,)


def dev_filt(case, mode, form):
    return tuple(torch.from_numpy(x.copy()).to(DEV) for x in S.filt(case, mode, form))


def check_case(case, worlds=WORLDS, forms=S.FORMS, oracle=True):
    auto = expected_auto(case)
    q = torch.from_numpy(S.queries(case).copy()).to(DEV)
    for world in worlds:
        sh = shards(case, world)
        for i in range(len(sh.ranges)):
            assert sh.path(i) == auto, (case.id, world, i)
            for p in (MFMA, TILE):
                if p in explicit_paths(case):
                    assert sh.path(i, PATH_NAME[p]) == p
                else:
                    with pytest.raises(ValueError):
                        sh.path(i, PATH_NAME[p])
            assert sh.path(i, "exact") == EXACT
        for mode in S.MODES:
            fixed, st = sh.reduce(mode, q)
            for form in forms:
                filt = dev_filt(case, mode, form)
                want = sh.exact(mode, q, fixed, st, filt, form == "table")
                if oracle and case.name != "pRotatE":
                    for i, (b, e) in enumerate(sh.ranges):
                        assert np.array_equal(want[i], S.shard_counts(case, mode, b, e)), (case.id, mode, world, form, i)
                for path in ("auto",) + tuple(PATH_NAME[p] for p in explicit_paths(case)):
                    got, listed = sh.fast(mode, q, fixed, st, filt, form == "table", path)
                    what = (case.id, mode, world, form, path)
                    assert np.array_equal(got, want), what
                    assert (listed >= 0).all(), what
                    if path == "exact" or (path == "auto" and auto == EXACT):
                        assert not listed.any(), what
                    for i, (b, e) in enumerate(sh.ranges):
                        assert (listed[i] <= max(e - b, 0)).all(), what  # cap 1024 > the 301 rows: never rescanned
                        # every exact tie of the shard was re-scored in reference order
                        if path != "exact" and auto != EXACT:
                            assert (listed[i] >= want[i, 1]).all(), what
                if case.plant:
                    # the planted exact copy ties in the shard that owns it (and nowhere else, see the oracle)
                    for (j, side), i in S.planned_tie_shard(case, world).items():
                        if side == mode:
                            assert want[i, 1, j] >= 1, (case.id, mode, world, j, i)
    ops.raise_on_device_error(DEV)


ONE_CALL = tuple(c for c in S.ALL_CASES if c.nq <= 65535)


@pytest.mark.parametrize("case", ONE_CALL, ids=[c.id for c in ONE_CALL])
def test_equals_exact_stage(case):
    """Every shard of worlds w1 to w4, both modes, both filter forms, every admitted path."""
    check_case(case)


# tile-eligible TransE (d = 37 is not); every BASE model with one full block of 64 queries and one short one
NEW_CASES = (S.Case("TransE", 36, plant=True), S.Case("TransE", 36, nq=70, plant=True)) + tuple(
    S.Case(c.name, c.d, nq=70, plant=c.plant) for c in S.BASE)


@pytest.mark.parametrize("case", NEW_CASES, ids=[c.id for c in NEW_CASES])
def test_new_cases_vs_oracle(case):
    check_case(case, forms=("lists",))
    check_case(case, worlds=("w4",), forms=("table",))


def test_many_queries():
    """70,001 queries in one call: refused on the tile-eligible shape (the tiles put queries on grid.y),
    served by path 3 with the exact stage's counts."""
    case = S.MANY[0]
    assert expected_auto(case) == TILE
    sh = shards(case, "w2")
    q = torch.from_numpy(S.queries(case).copy()).to(DEV)
    mode = "tail-batch"
    fixed, st = sh.reduce(mode, q)
    filt = dev_filt(case, mode, "lists")
    assert sh.path(0) == TILE
    for path in ("auto", "tile"):
        with pytest.raises(ValueError):
            sh.fast(mode, q, fixed, st, filt, False, path)
    want = sh.exact(mode, q, fixed, st, filt, False)
    got, listed = sh.fast(mode, q, fixed, st, filt, False, "exact")
    assert np.array_equal(got, want) and not listed.any()
    for i, (b, e) in enumerate(sh.ranges):
        assert np.array_equal(want[i], S.shard_counts(case, mode, b, e))
    # ... and the first 65,535 of them on the tile
    n = 65535
    f2 = (filt[0][:n + 1].contiguous(), filt[1])
    got, _ = sh.fast(mode, q[:n].contiguous(), fixed[:n].contiguous(), st[:n].contiguous(), f2, False, "tile")
    assert np.array_equal(got, want[:, :, :n])
    ops.raise_on_device_error(DEV)


# ---- the list's cap

TIE_CASES = tuple(c for c in T.CASES if c.aligned and (c.name, c.d) in (
    ("TransE", 32), ("DistMult", 32), ("ComplEx", 16), ("RotatE", 16), ("RotatE", 1000), ("DistMult", 1100)))


def tie_ranges(case, parts):
    rest = case.E - T.C
    if parts == 2:
        return [(0, T.C), (T.C, case.E)]
    return [(0, T.C), (T.C, T.C + rest // 2), (T.C + rest // 2, case.E)]


def tie_lists(case, mode):
    m = T.filtered_mask(case, mode)
    off = np.zeros(len(m) + 1, dtype=np.int64)
    np.cumsum(m.sum(1), out=off[1:])
    return off, np.nonzero(m)[1].astype(np.int64)


def tie_counts(case, mode, b, e):
    """[2, nq]: the oracle's counts of the shard [b, e)."""
    s, st = T.score_row(case, mode)
    q = T.queries(case)
    keep = ~T.filtered_mask(case, mode)
    keep[np.arange(len(q)), q[:, 0 if mode == "head-batch" else 2]] = False
    keep = keep[:, b:e]
    x = s[None, b:e]
    return np.stack([(keep & (x > st)).sum(1), (keep & (x == st)).sum(1)]).astype(np.int64)


@pytest.mark.parametrize("case", TIE_CASES, ids=[c.id for c in TIE_CASES])
@pytest.mark.parametrize("parts", (2, 3))
def test_list_cap(case, parts):
    """One shard holds the 1100 exact copies: query j lists exactly ladder[j] of them there — 1023, 1024 (the
    full list) and 1025 (rescanned over the own rows) among them.  Counts == exact stage == oracle."""
    ranges = tie_ranges(case, parts)
    sh = Parts(case.name, T.tables(case), T.GAMMA, ranges)
    q = torch.from_numpy(T.queries(case).copy()).to(DEV)
    p = T.ladder(case)
    assert {T.CAP - 1, T.CAP, T.CAP + 1} <= set(p.tolist())
    bil = case.name in ("DistMult", "ComplEx")
    paths = ("auto", "tile") if bil and case.d % 4 == 0 else ("auto",)
    for mode in T.MODES:
        fixed, st = sh.reduce(mode, q)
        filt = tuple(torch.from_numpy(x).to(DEV) for x in tie_lists(case, mode))
        want = sh.exact(mode, q, fixed, st, filt, False)
        for i, (b, e) in enumerate(ranges):
            assert np.array_equal(want[i], tie_counts(case, mode, b, e)), (case.id, mode, i)
        for path in paths:
            assert sh.path(0, path) == (TILE if path == "tile" or not bil else MFMA)
            got, listed = sh.fast(mode, q, fixed, st, filt, False, path)
            assert np.array_equal(got, want), (case.id, mode, path)
            # shard 0 holds plants only: the unfiltered ones all tie exactly, and nothing else is there to list
            assert np.array_equal(listed[0], p), (case.id, mode, path, listed[0], p)
            assert (listed[0] > T.CAP).any() and (listed[0] == T.CAP).any() and (listed[0] < T.CAP).any()
            assert np.array_equal(got[0, 1], p) and not got[0, 0].any()
    ops.raise_on_device_error(DEV)


# ---- bad queries, small shards, determinism

@pytest.mark.parametrize("col,bad", [(0, 10 ** 6), (0, -1), (1, S.R), (1, -1), (2, 301), (2, -7)])
@pytest.mark.parametrize("case", (S.Case("DistMult", 40, nq=70, plant=True), S.Case("RotatE", 20, nq=70, plant=True),
                                  S.Case("TransE", 36, nq=70, plant=True)), ids=lambda c: c.id)
def test_query_out_of_range(case, col, bad):
    """A bad query inside a 64-query block: 0 / 0 for it, its neighbours' counts unchanged, IndexError from
    raise_on_device_error — on every shard of w3 (the one-row shard and the empty one included)."""
    sh = shards(case, "w3")
    qh = S.queries(case).copy()
    qh[37, col] = bad
    q = torch.from_numpy(qh).to(DEV)
    good = torch.from_numpy(S.queries(case).copy()).to(DEV)
    for mode in S.MODES:
        filt = dev_filt(case, mode, "lists")
        # (the reduced buffers of the good queries: a bad fixed side leaves zeros in its row, which no one reads)
        fixed, st = sh.reduce(mode, good)
        ops.raise_on_device_error(DEV)
        for path in ("auto",) + tuple(PATH_NAME[p] for p in explicit_paths(case)):
            got, listed = sh.fast(mode, q, fixed, st, filt, False, path)
            with pytest.raises(IndexError):
                ops.raise_on_device_error(DEV)
            ops.raise_on_device_error(DEV)  # (cleared)
            for i, (b, e) in enumerate(sh.ranges):
                want = S.shard_counts(case, mode, b, e).copy()
                want[:, 37] = 0
                assert np.array_equal(got[i], want), (case.id, mode, path, i, col, bad)
                assert listed[i, 37] == 0
        # the empty shard alone flags the query too
        c = torch.empty(2, case.nq, dtype=torch.int64, device=DEV)
        ops.rank_shard_count_fast(sh.descs[1], mode, q, sh.ranges[1], DEV, fixed, st, filt, c)
        with pytest.raises(IndexError):
            ops.raise_on_device_error(DEV)
        assert not c.any()


@pytest.mark.parametrize("case", (S.BASE[1], S.BASE[3], S.Case("TransE", 36, plant=True)), ids=lambda c: c.id)
def test_filter_ids_outside_the_table_are_no_error(case):
    """As in the exact stage: a listed id outside the shard or the table is simply not this shard's."""
    sh = shards(case, "w2")
    q = torch.from_numpy(S.queries(case).copy()).to(DEV)
    mode = "head-batch"
    off, ids = S.filter_lists(case, mode)
    ids = ids.copy()
    ids[::7] = case.E + 5
    ids[3::11] = -2
    filt = (torch.from_numpy(off.copy()).to(DEV), torch.from_numpy(ids).to(DEV))
    fixed, st = sh.reduce(mode, q)
    want = sh.exact(mode, q, fixed, st, filt, False)
    ops.raise_on_device_error(DEV)
    for path in ("auto",) + tuple(PATH_NAME[p] for p in explicit_paths(case)):
        got, _ = sh.fast(mode, q, fixed, st, filt, False, path)
        assert np.array_equal(got, want), path
        ops.raise_on_device_error(DEV)


@pytest.mark.parametrize("case", (S.BASE[1], S.BASE[3], S.Case("TransE", 36, plant=True)), ids=lambda c: c.id)
def test_any_given_true_score(case):
    """s_true is the caller's: whatever it holds — another query's score, ±0, huge, infinite, NaN — the counts
    are the exact stage's for the same buffer (an infinite one is rescanned; a NaN compares with nothing)."""
    sh = shards(case, "w2")
    q = torch.from_numpy(S.queries(case).copy()).to(DEV)
    for mode in S.MODES:
        fixed, st = sh.reduce(mode, q)
        st = st.roll(1).contiguous()
        st[2], st[3], st[4], st[5], st[6], st[7] = float("inf"), float("-inf"), float("nan"), 0.0, -0.0, 3e38
        filt = dev_filt(case, mode, "lists")
        want = sh.exact(mode, q, fixed, st, filt, False)
        for path in ("auto",) + tuple(PATH_NAME[p] for p in explicit_paths(case)):
            got, listed = sh.fast(mode, q, fixed, st, filt, False, path)
            assert np.array_equal(got, want), (case.id, mode, path)
            assert not got[:, :, 4].any()
            if path != "exact":
                assert (listed[:, 2:4] > T.CAP).all()  # rescanned
    ops.raise_on_device_error(DEV)


@pytest.mark.parametrize("case", (S.BASE[1], S.BASE[3], S.Case("TransE", 36, nq=70, plant=True), T.CASES[1]),
                         ids=lambda c: c.id)
def test_deterministic(case):
    if isinstance(case, T.Case):
        sh = Parts(case.name, T.tables(case), T.GAMMA, tie_ranges(case, 2))
        q = torch.from_numpy(T.queries(case).copy()).to(DEV)
        filt = tuple(torch.from_numpy(x).to(DEV) for x in tie_lists(case, "tail-batch"))
    else:
        sh = shards(case, "w2")
        q = torch.from_numpy(S.queries(case).copy()).to(DEV)
        filt = dev_filt(case, "tail-batch", "lists")
    fixed, st = sh.reduce("tail-batch", q)
    a = sh.fast("tail-batch", q, fixed, st, filt, False)
    b = sh.fast("tail-batch", q, fixed, st, filt, False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    ops.raise_on_device_error(DEV)


def test_bad_buffers():
    case = S.BASE[1]
    sh = shards(case, "w2")
    d, own = sh.descs[0], sh.ranges[0]
    q = torch.from_numpy(S.queries(case).copy()).to(DEV)
    fixed = torch.empty(case.nq, sh.le, device=DEV)
    st = torch.empty(case.nq, device=DEV)
    c = torch.empty(2, case.nq, dtype=torch.int64, device=DEV)
    filt = tuple(torch.from_numpy(x.copy()) for x in S.filter_lists(case, "tail-batch"))
    fast = ops.rank_shard_count_fast
    with pytest.raises(ValueError):
        fast(d, "single", q, own, DEV, fixed, st, filt, c)
    with pytest.raises(ValueError):
        fast(d, "tail-batch", q, own, DEV, fixed[:, :-1].contiguous(), st, filt, c)
    with pytest.raises(ValueError):
        fast(d, "tail-batch", q, (5, 4), DEV, fixed, st, filt, c)
    with pytest.raises(ValueError):
        fast(d, "tail-batch", q, own, DEV, fixed, st[:-1], filt, c)
    with pytest.raises(ValueError):
        fast(d, "tail-batch", q, own, DEV, fixed, st, filt, c.int())
    with pytest.raises(ValueError):  # per-query offsets given as the whole index
        fast(d, "tail-batch", q, own, DEV, fixed, st, filt, c, filter_table=True)
    with pytest.raises(ValueError):
        fast(d, "tail-batch", q, own, DEV, fixed, st, filt, c, path="mfma32")
    with pytest.raises(ValueError):
        fast(d, "tail-batch", q, own, DEV, fixed, st, filt, c, listed=torch.empty(case.nq, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):  # TransE has no MFMA tile
        t = shards(S.Case("TransE", 36, plant=True), "w1")
        ops.rank_shard_fast_path(t.descs[0], t.ranges[0], "mfma")
