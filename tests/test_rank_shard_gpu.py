"""kge_rank_shard on the device, one process playing every rank through ops:
each shard is a tensor of its own rows alone, addressed by global id through a
descriptor whose entity pointer lies own_begin rows before it; the stage
buffers of the ranks are summed here as the all-reduces would (fixed_rows and
s_true viewed as int32, counts as int64).

Per-shard counts equal the fp32 reference-order oracle's exactly for TransE,
DistMult, ComplEx and RotatE (RotatE with relation_trig =
ops.reference_rotation, the torch CPU cos / sin the oracle uses) over the cases
of tests/rank_shard_cases.py, in every world and both filter forms, and their
sums equal ops.rank_filtered's ranks and ties on the whole table.

pRotatE: the sums equal the device's one-call ops.rank_filtered exactly.
Against the oracle (sin = the float64 sin rounded once, the device's sin_rn) a
query may differ only if rank_candidates_cases.excusable's rule excuses it, at
most 5 % of the queries may, and the inputs excuse none
(test_rank_shard_ref.py), so agreement is exact there too.
"""
import numpy as np
import pytest
import torch

import rank_shard_cases as S
from knowledgegraphembedding_amd import ops
from test_slot_matrix_gpu import unaligned

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


class Shards:
    """The case's tables on the device, one tensor and descriptor per shard of `world`."""

    def __init__(self, case, world):
        ent, rel, mod, erange = S.tables(case)
        self.case, self.ranges = case, S.splits(case.E)[world]
        self.rel = torch.from_numpy(rel.copy()).to(DEV)
        self.mod = None if mod is None else torch.from_numpy(mod.copy()).to(DEV)
        self.trig = ops.reference_rotation(self.rel, erange).to(DEV) if case.name == "RotatE" else None
        self.le = ent.shape[1]
        self.rows, self.descs = [], []
        for b, e in self.ranges:
            t = torch.from_numpy(ent[b:max(e, b + 1)].copy()).to(DEV)  # (an empty shard: one row that is never read)
            if not case.aligned:
                t = unaligned(t)
            assert (t.data_ptr() % 16 == 0) == case.aligned
            d = ops.make_desc(case.name, t, self.rel, S.GAMMA, erange, self.mod)
            d.entity_embedding = t.data_ptr() - b * self.le * 4
            d.nentity = case.E
            self.rows.append(t)
            self.descs.append(d)
        whole = torch.from_numpy(ent.copy()).to(DEV)
        self.whole = whole if case.aligned else unaligned(whole)
        self.whole_desc = ops.make_desc(case.name, self.whole, self.rel, S.GAMMA, erange, self.mod)

    def run(self, mode, form, queries=None):
        """The three stages over every shard; returns (per-shard counts [world, 2, nq] int64 on the
        host, fixed_rows, s_true) — the reduced buffers as device tensors."""
        case = self.case
        q = torch.from_numpy((S.queries(case) if queries is None else queries).copy()).to(DEV)
        nq = q.shape[0]
        filt = tuple(torch.from_numpy(x.copy()).to(DEV) for x in S.filt(case, mode, form))
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
        st = st.view(torch.float32)
        counts = []
        for d, own in zip(self.descs, self.ranges):
            c = torch.empty(2, nq, dtype=torch.int64, device=DEV)
            ops.rank_shard_count(d, mode, q, own, DEV, fixed, st, filt, c, filter_table=form == "table",
                                 relation_trig=self.trig)
            counts.append(c)
        return torch.stack(counts).cpu().numpy(), fixed, st


def whole_table_ranks(sh, mode):
    off, ids = S.filter_lists(sh.case, mode)
    r, t = ops.rank_filtered(sh.whole_desc, mode, torch.from_numpy(S.queries(sh.case).copy()), torch.from_numpy(off.copy()),
                             torch.from_numpy(ids.copy()), DEV, relation_trig=sh.trig)
    return r.cpu().numpy(), t.cpu().numpy()


def check_vs_oracle(case, mode, world, form, counts):
    for i, (b, e) in enumerate(S.splits(case.E)[world]):
        want = S.shard_counts(case, mode, b, e)
        bad = np.nonzero((counts[i] != want).any(0))[0]
        what = f"{case.id} {mode} {world} {form} shard [{b}, {e})"
        print(f"{what}: {len(bad)} of {case.nq} queries differ from the oracle")
        if case.name == "pRotatE":
            ok = S.excusable(case, mode)
            assert ok.sum() <= 0.05 * case.nq, what
            bad = bad[~ok[bad]]
        assert not len(bad), f"{what}: queries {bad[:8]}: {counts[i][:, bad[:8]]} vs {want[:, bad[:8]]}"


WORLDS = ("w1", "w2", "w3", "w4")


@pytest.mark.parametrize("case", S.ALL_CASES, ids=[c.id for c in S.ALL_CASES])
def test_vs_oracle_and_whole_table(case):
    whole = {}
    for world in WORLDS:
        sh = Shards(case, world)
        for mode in S.MODES:
            # the whole-index form once per case and mode (its lookup does not depend on the split)
            for form in (S.FORMS if world == "w4" else ("lists",)):
                counts, fixed, st = sh.run(mode, form)
                ops.raise_on_device_error(DEV)
                check_vs_oracle(case, mode, world, form, counts)
                # the reduced stage buffers: the fixed side's rows and the oracle's true score, bit for bit
                x = S.queries(case)[:, 2 if mode == "head-batch" else 0]
                assert np.array_equal(fixed.cpu().numpy().view(np.int32), S.tables(case)[0][x].view(np.int32))
                if case.name != "pRotatE":
                    assert np.array_equal(st.cpu().numpy().view(np.int32), S.scores(case, mode)[:, 0].view(np.int32))
                if case.nq > 65535:
                    continue  # (past ops.rank_filtered's queries per call)
                if mode not in whole:
                    whole[mode] = whole_table_ranks(sh, mode)
                tot = counts.sum(0)
                assert np.array_equal(1 + tot[0], whole[mode][0]), (case.id, mode, world, form)
                assert np.array_equal(tot[1], whole[mode][1].astype(np.int64)), (case.id, mode, world, form)
    ops.raise_on_device_error(DEV)


@pytest.mark.parametrize("case", (S.BASE[0], S.BASE[3], S.WIDTHS[0]), ids=lambda c: c.id)
def test_deterministic_and_geometry_independent(case, monkeypatch):
    mode = "tail-batch"
    sh = Shards(case, "w2")
    a = sh.run(mode, "lists")
    b = sh.run(mode, "lists")
    assert np.array_equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
    for chunk in ("7", "64", "1000"):  # rows per chunk (a diagnostic switch): other grids, the same counts
        monkeypatch.setenv("KGE_RANK_SHARD_CHUNK", chunk)
        assert np.array_equal(sh.run(mode, "lists")[0], a[0]), chunk
    ops.raise_on_device_error(DEV)


@pytest.mark.parametrize("case", (S.BASE[1], S.BASE[2], S.BASE[3], S.BASE[4], S.WIDTHS[0], S.WIDTHS[1]), ids=lambda c: c.id)
@pytest.mark.parametrize("qpw", ("2", "4"))
def test_queries_per_workgroup(case, qpw, monkeypatch):
    """KGE_RANK_SHARD_QPW (a diagnostic switch): every staged row scored against 2 or 4 queries of one
    workgroup — the oracle's counts again; nq = 24, 8 and 6 leave a short last group at 4, and a bad
    query inside a group leaves its neighbours' counts alone."""
    monkeypatch.setenv("KGE_RANK_SHARD_QPW", qpw)
    for world in ("w3", "w4"):
        sh = Shards(case, world)
        for mode in S.MODES:
            counts, _, _ = sh.run(mode, "lists")
            check_vs_oracle(case, mode, world, "lists", counts)
    ops.raise_on_device_error(DEV)
    q = S.queries(case).copy()
    q[1, 1] = S.R
    counts, _, _ = sh.run("tail-batch", "table", queries=q)
    with pytest.raises(IndexError):
        ops.raise_on_device_error(DEV)
    for i, (b, e) in enumerate(sh.ranges):
        want = S.shard_counts(case, "tail-batch", b, e).copy()
        want[:, 1] = 0
        assert np.array_equal(counts[i], want), i


@pytest.mark.parametrize("col,bad", [(0, 10 ** 6), (0, -1), (1, S.R), (2, 301), (2, -7)])
@pytest.mark.parametrize("mode", S.MODES)
def test_query_out_of_range(col, bad, mode):
    case = S.BASE[1]
    sh = Shards(case, "w3")  # (an empty shard flags the query too)
    q = S.queries(case).copy()
    q[5, col] = bad
    ops.raise_on_device_error(DEV)
    counts, fixed, st = sh.run(mode, "lists", queries=q)
    with pytest.raises(IndexError):
        ops.raise_on_device_error(DEV)
    ops.raise_on_device_error(DEV)  # (cleared)
    for i, (b, e) in enumerate(sh.ranges):
        want = S.shard_counts(case, mode, b, e).copy()
        want[:, 5] = 0
        assert np.array_equal(counts[i], want), (i, col, bad)
    assert int(st.view(torch.int32)[5]) == 0
    # every stage alone raises the flag for the ids it reads
    qd = torch.from_numpy(q).to(DEV)
    fixed_col = 2 if mode == "head-batch" else 0
    ops.rank_shard_rows(sh.descs[2], mode, qd, sh.ranges[2], DEV, torch.empty_like(fixed))
    if col == fixed_col:
        with pytest.raises(IndexError):
            ops.raise_on_device_error(DEV)
    ops.raise_on_device_error(DEV)
    c = torch.empty(2, case.nq, dtype=torch.int64, device=DEV)
    filt = tuple(torch.from_numpy(x.copy()) for x in S.filter_lists(case, mode))
    ops.rank_shard_count(sh.descs[1], mode, qd, sh.ranges[1], DEV, fixed, st, filt, c)  # the empty shard
    with pytest.raises(IndexError):
        ops.raise_on_device_error(DEV)
    assert not c.any()


def test_bad_buffers():
    case = S.BASE[1]
    sh = Shards(case, "w2")
    d, own = sh.descs[0], sh.ranges[0]
    q = torch.from_numpy(S.queries(case).copy()).to(DEV)
    fixed = torch.empty(case.nq, sh.le, device=DEV)
    st = torch.empty(case.nq, device=DEV)
    c = torch.empty(2, case.nq, dtype=torch.int64, device=DEV)
    filt = tuple(torch.from_numpy(x.copy()) for x in S.filter_lists(case, "tail-batch"))
    with pytest.raises(ValueError):
        ops.rank_shard_rows(d, "single", q, own, DEV, fixed)
    with pytest.raises(ValueError):
        ops.rank_shard_rows(d, "tail-batch", q, own, DEV, fixed[:, :-1].contiguous())
    with pytest.raises(ValueError):
        ops.rank_shard_rows(d, "tail-batch", q, (5, 4), DEV, fixed)
    with pytest.raises(ValueError):
        ops.rank_shard_rows(d, "tail-batch", q, (0, case.E + 1), DEV, fixed)
    with pytest.raises(ValueError):
        ops.rank_shard_true(d, "tail-batch", q, own, DEV, fixed, st[:-1])
    with pytest.raises(ValueError):
        ops.rank_shard_count(d, "tail-batch", q, own, DEV, fixed, st, filt, c.int())
    with pytest.raises(ValueError):  # per-query offsets given as the whole index
        ops.rank_shard_count(d, "tail-batch", q, own, DEV, fixed, st, filt, c, filter_table=True)
    with pytest.raises(ValueError):
        ops.rank_shard_count(d, "tail-batch", q, own, DEV, fixed, st, (filt[0][:-1], filt[1]), c)
