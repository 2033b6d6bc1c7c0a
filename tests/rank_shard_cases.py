"""Shared inputs of the sharded filtered ranking tests (test_rank_shard_ref.py on
the CPU; test_rank_shard_gpu.py and test_rank_shard_arena_gpu.py on the
device): per case the tables, the queries, the filter in both forms, the row
splits ("worlds") and the counts the fp32 reference-order oracle gives every
shard.

Tables: rank_candidates_cases.tables() of the same shapes (R = 7, GAMMA = 12,
dims 37 / 40 / 20 / 20 / 40, E = 301), with the planted rows below written over
a copy.

Expected counts: oracle.ref_order_scores on the sample (queries, [true id |
every entity]) in the call's mode — column 0 is the true score s_true — and per
shard [b, e)
    counts[0] = #{x in [b, e), x != true id, x not excluded : s_x > s_true}
    counts[1] = the same with ==
where a query's excluded ids are the other known answers of its key in
ALL_TRUE (TestDataset's filter, dataloader.py:134-154).

Worlds (splits(E)): one shard; two ([0, E // 2), [E // 2, E)); three uneven
([0, 1), [1, 1), [1, E)): a one-row shard, an empty one and a chunk tail; and
EntityRowPartition's own split at world 4 (rows = ceil(E / 4)).

Queries: h, r, t uniform, so with four shards h, t and a scanned row usually
belong to three different ranks.  all_true = the first 300 queries plus, per
query j < 300 and direction, 0 / 2 / 9 / 30 (j mod 4) further answers drawn
over the whole table, so lists span the shards and every fourth one is empty
but for coincidences.

Filter forms.  "table": the whole index, filt_off [E·R + 1] by key h·R + r
(tail-batch) / r·E + t (head-batch) — its lists hold the true id.  "lists":
per-query lists of the same ids without the true id, except that queries
j mod 5 = 1 list the true id too and queries j mod 5 = 2 list every id twice, in
shuffled order.

`plant` cases (not pRotatE): planted query j < len(PLANT_ROWS) is
(h = 20 + 2j, r, t = 21 + 2j); row PLANT_ROWS[j] — the rows either side of
every shard boundary of the worlds above — is an exact copy of its h row
(j even) or t row (j odd), so ranking that side it has one exact tie, in the
shard that owns the planted row (planned_tie_shard); rows 100 + j and 120 + j are
its h and t row with one coordinate moved to the next float: near-ties.  No
planted query's extra answers fall on a planted row.

pRotatE: the oracle takes sin as the float64 sin rounded once to fp32 (the
device's sin_rn); rank_candidates_cases.excusable's rule decides which queries
could differ, and these inputs have none (test_rank_shard_ref.py).
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

import rank_candidates_cases as K
from oracle import kge_oracle as O

MODES = K.MODES
GAMMA, R = K.GAMMA, K.R
N_TRUE_Q = 300  # queries whose triple (and extra answers) are in all_true


@dataclass(frozen=True)
class Case:
    name: str
    d: int
    E: int = 301
    nq: int = 24
    seed: int = 5
    plant: bool = False
    aligned: bool = True  # False: every shard one float past a 16-byte boundary

    @property
    def id(self):
        return (f"{self.name}-d{self.d}-E{self.E}-nq{self.nq}" + ("-plant" if self.plant else "")
                + ("" if self.aligned else "-unaligned"))

    @property
    def base(self):
        """The rank_candidates_cases case whose tables this one starts from."""
        return K.Case(self.name, self.d, E=self.E, seed=self.seed)


# all five models at the slot shapes of rank_candidates_cases.BASE
BASE = (Case("TransE", 37, plant=True), Case("DistMult", 40, plant=True), Case("ComplEx", 20, plant=True),
        Case("RotatE", 20, plant=True), Case("pRotatE", 40))
# the staging variants of k_rshard_count: 16-byte slots prefetched in 4 (BASE) /
# 8 / 16 registers per lane (DistMult 600, RotatE 1000), staged without prefetch
# (DistMult 2400), rows read in place (RotatE 9000, a 72 KB row: q in the workspace)
WIDTHS = (Case("RotatE", 1000, nq=8), Case("DistMult", 600, nq=6), Case("DistMult", 2400, E=64, nq=4),
          Case("RotatE", 9000, E=64, nq=4))
UNALIGNED = (Case("DistMult", 40, aligned=False), Case("RotatE", 20, aligned=False))
# rows of exactly 512 | 513 slots, the last step of the prefetch ladder
# (rank_candidates_cases.BOUNDARY): 16-byte slots of 2048 | 2052 floats,
# single-float slots of 512 | 516 floats on an unaligned table
BOUNDARY = (Case("DistMult", 2048, E=200, nq=5), Case("DistMult", 2052, E=200, nq=5),
            Case("DistMult", 512, E=200, nq=5, aligned=False), Case("DistMult", 516, E=200, nq=5, aligned=False))
# one call past the 65,535-query ceiling of kge_rank_filtered*
MANY = (Case("TransE", 8, E=50, nq=70001),)
EXACT_CASES = tuple(c for c in BASE if c.name != "pRotatE") + WIDTHS + UNALIGNED + BOUNDARY + MANY
PROTATE_CASES = tuple(c for c in BASE if c.name == "pRotatE")
ALL_CASES = EXACT_CASES + PROTATE_CASES
FORMS = ("lists", "table")

# the rows either side of every shard boundary of splits(301)
PLANT_ROWS = (0, 1, 75, 76, 149, 150, 151, 152, 227, 228, 300)
NUDGE_H, NUDGE_T = 100, 120


def splits(E):
    """{world name: [(begin, end) per rank]}"""
    rows = -(-E // 4)  # EntityRowPartition: rank r owns [min(r·rows, E), min(E, (r + 1)·rows))
    return {"w1": [(0, E)], "w2": [(0, E // 2), (E // 2, E)], "w3": [(0, 1), (1, 1), (1, E)],
            "w4": [(min(r * rows, E), min(E, (r + 1) * rows)) for r in range(4)]}


def planted(case):
    """[(query j, h, t, planted row, which side it copies)]"""
    if not case.plant:
        return []
    return [(j, 20 + 2 * j, 21 + 2 * j, p, "head-batch" if j % 2 == 0 else "tail-batch")
            for j, p in enumerate(PLANT_ROWS)]


@lru_cache(maxsize=None)
def queries(case):
    g = np.random.default_rng(case.seed + 400)
    q = np.stack([g.integers(0, case.E, case.nq), g.integers(0, R, case.nq), g.integers(0, case.E, case.nq)],
                 1).astype(np.int64)
    for j, h, t, _, _ in planted(case):
        q[j, 0], q[j, 2] = h, t
    q.setflags(write=False)
    return q


def true_ids(case, mode):
    return queries(case)[:, 0 if mode == "head-batch" else 2]


@lru_cache(maxsize=None)
def tables(case):
    """(ent [E, Le], rel [R, Lr], modulus or None, erange), float32, read-only."""
    ent, rel, mod, erange = K.tables(case.base)
    if case.plant:
        assert case.name != "pRotatE" and case.E == 301 and case.nq >= len(PLANT_ROWS)
        ent = ent.copy()
        le = ent.shape[1]
        for j, h, t, p, side in planted(case):
            ent[p] = ent[h if side == "head-batch" else t]
            for base, src in ((NUDGE_H, h), (NUDGE_T, t)):
                row = ent[src].copy()
                k = (7 * j + 3) % le
                row[k] = np.nextafter(row[k], np.float32(np.inf if j % 2 else -np.inf), dtype=np.float32)
                ent[base + j] = row
        ent.setflags(write=False)
    return ent, rel, mod, erange


@lru_cache(maxsize=None)
def all_true(case):
    """[n, 3] int64, unique rows: the known true triples the filter is built from."""
    g = np.random.default_rng(case.seed + 500)
    q = queries(case)[:N_TRUE_Q]
    keep_off = set(PLANT_ROWS) if case.plant else set()
    rows = [q]
    for j, (h, r, t) in enumerate(q.tolist()):
        k = (0, 2, 9, 30)[j % 4]
        for col in (0, 2):
            x = g.integers(0, case.E, k)
            if j < len(planted(case)):
                x = np.asarray([e for e in x.tolist() if e not in keep_off], dtype=np.int64)
            extra = np.tile(np.asarray([[h, r, t]], dtype=np.int64), (len(x), 1))
            extra[:, col] = x
            rows.append(extra)
    a = np.unique(np.concatenate(rows), axis=0)
    a.setflags(write=False)
    return a


def _keys(case, trip, mode):
    return trip[:, 1] * case.E + trip[:, 2] if mode == "head-batch" else trip[:, 0] * R + trip[:, 1]


@lru_cache(maxsize=None)
def filter_table(case, mode):
    """(filt_off [E·R + 1], filt_ids): the whole index (KGE_RANK_FILTER_TABLE), ids sorted by key."""
    a = all_true(case)
    key = _keys(case, a, mode)
    val = a[:, 0] if mode == "head-batch" else a[:, 2]
    order = np.lexsort((val, key))
    off = np.zeros(case.E * R + 1, dtype=np.int64)
    np.cumsum(np.bincount(key, minlength=case.E * R), out=off[1:])
    ids = np.ascontiguousarray(val[order])
    off.setflags(write=False)
    ids.setflags(write=False)
    return off, ids


@lru_cache(maxsize=None)
def excluded(case, mode):
    """[nq, E] bool: the ids a query's filter excludes (the true id apart)."""
    off, ids = filter_table(case, mode)
    key = _keys(case, queries(case), mode)
    ex = np.zeros((case.nq, case.E), dtype=bool)
    for j, k in enumerate(key.tolist()):
        ex[j, ids[off[k]:off[k + 1]]] = True
    ex[np.arange(case.nq), true_ids(case, mode)] = False
    ex.setflags(write=False)
    return ex


@lru_cache(maxsize=None)
def filter_lists(case, mode):
    """(filt_off [nq + 1], filt_ids): per-query lists — see the module docstring."""
    g = np.random.default_rng(case.seed + 600)
    ex, tid = excluded(case, mode), true_ids(case, mode)
    lists = []
    for j in range(case.nq):
        l = np.nonzero(ex[j])[0].astype(np.int64)
        if j % 5 == 1:
            l = np.append(l, tid[j])
        if j % 5 == 2:
            l = g.permutation(np.concatenate([l, l]))
        lists.append(l)
    off = np.zeros(case.nq + 1, dtype=np.int64)
    np.cumsum([len(l) for l in lists], out=off[1:])
    ids = np.concatenate(lists) if off[-1] else np.zeros(0, dtype=np.int64)
    off.setflags(write=False)
    ids.setflags(write=False)
    return off, ids


def filt(case, mode, form):
    return filter_lists(case, mode) if form == "lists" else filter_table(case, mode)


@lru_cache(maxsize=None)
def scores(case, mode):
    """[nq, 1 + E] float32: the oracle's reference-order scores of [true id | every entity]."""
    ent, rel, mod, erange = tables(case)
    trig = (None, K.sin_rn) if case.name == "pRotatE" else None
    out = []
    for b0 in range(0, case.nq, 8192):  # (blocks bound the [nq, 1 + E, d] temporaries)
        q = queries(case)[b0:b0 + 8192]
        tid = true_ids(case, mode)[b0:b0 + 8192]
        ids = np.concatenate([tid[:, None], np.broadcast_to(np.arange(case.E, dtype=np.int64), (len(q), case.E))], 1)
        sample = (torch.from_numpy(q.copy()), torch.from_numpy(np.ascontiguousarray(ids)))
        out.append(np.asarray(O.ref_order_scores(case.name, ent.copy(), rel.copy(), mod, sample, mode, GAMMA, erange,
                                                 trig=trig), dtype=np.float32))
    s = np.ascontiguousarray(np.concatenate(out))
    assert s.shape == (case.nq, 1 + case.E)
    s.setflags(write=False)
    return s


def shard_counts(case, mode, b, e):
    """[2, nq] int64: the oracle's counts of the shard [b, e)."""
    s, ex = scores(case, mode), excluded(case, mode)
    keep = ~ex[:, b:e]
    tid = true_ids(case, mode)
    own = (tid >= b) & (tid < e)
    keep[np.nonzero(own)[0], tid[own] - b] = False
    st = s[:, :1]
    x = s[:, 1 + b:1 + e]
    return np.stack([(keep & (x > st)).sum(1), (keep & (x == st)).sum(1)]).astype(np.int64)


def planned_tie_shard(case, world):
    """{(query j, mode): index of the shard of `world` that owns j's planted exact copy}"""
    out = {}
    for j, _, _, p, side in planted(case):
        out[(j, side)] = next(i for i, (b, e) in enumerate(splits(case.E)[world]) if b <= p < e)
    return out


def excusable(case, mode, ulps=4):
    """[nq] bool, rank_candidates_cases.excusable's rule over the whole table: the oracle has
    an unexcluded entity other than the true one within `ulps` of the true score."""
    s = scores(case, mode)
    near = np.abs(K.float_ord(s[:, 1:]) - K.float_ord(s[:, :1])) <= ulps
    other = ~excluded(case, mode)
    other[np.arange(case.nq), true_ids(case, mode)] = False
    return (near & other).any(1)
