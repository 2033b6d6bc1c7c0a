"""Shared inputs of the relation-prediction tests (test_rank_relations_ref.py on
the CPU, test_rank_relations_gpu.py on the device): per case the tables, the
queries, each query's filter list, and the scores, ranks and tie counts the
fp32 reference-order oracle gives.

Expected values: oracle.ref_order_scores in 'single' mode on the nq·R triples
(h, r', t), r' = 0..R-1, reshaped to [nq, R]; then
  rank = 1 + #{r' != r, r' not excluded : s(r') > s(r)},  ties likewise with ==,
and rank 0, ties 0 for a query with r = -1 ("no true relation").

`plant` cases (TransE, DistMult, ComplEx, RotatE; R >= 61) lay out the relation
table as
  rows 0..3       the true rows: query j < 8 has r = j mod 4
  rows 4..19      exact copies: 4 + 4·e + c, c < 4, is a copy of true row e
  rows 20..31     nudged copies: 20 + 3·e + k, k < 3, is true row e with three
                  coordinates scaled by 1 ± 2^-x, x = NUDGE_EXP[3e + k]: twelve
                  exponents of 8..21, 2^-20 and 2^-21 among them
  rows 32..       untouched background
Every relation is scored, so raw each planted query ties with its 4 exact copies
(planned_ties); its filter list excludes the first 1 + j mod 3 of them, so the
filtered tie count drops by exactly those.  A nudged copy is a near-tie that may
round onto the true score as well.

Filter lists (every case): query j's list holds background relations (one of
them twice when j mod 4 = 0), its true r, the id R + j (outside [0, R)), and for
a planted query the copies above — shuffled.  Query nq // 2's list is empty.

`pred` cases: rows 2 and 5 carry r = -1 among ranked rows.

pRotatE: the oracle takes sin as the float64 sin rounded once to fp32 (`rn`,
the device's sin_rn).  A query could be excused from exact agreement only if
the oracle has another relation within 4 ulp of the true score; these inputs
have no such query (test_rank_relations_ref.py).
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

from conftest import dims, synth_tables
from oracle import kge_oracle as O

GAMMA = 12.0
N_TRUE, N_COPY, N_NUDGE, BG0 = 4, 4, 3, 32
N_PLANTED_Q = 8


@dataclass(frozen=True)
class Case:
    name: str
    d: int
    R: int = 61
    E: int = 301
    nq: int = 24
    seed: int = 5
    plant: bool = False
    pred: bool = False
    aligned: bool = True  # False: both tables one float past a 16-byte boundary

    @property
    def id(self):
        return (f"{self.name}-d{self.d}-E{self.E}-R{self.R}-nq{self.nq}" + ("-plant" if self.plant else "")
                + ("-pred" if self.pred else "") + ("" if self.aligned else "-unaligned"))


# all five models: single-float slots (TransE 37, pRotatE 37), one full cascade
# row plus a tail vector (DistMult 40), tail vectors plus a scalar tail (ComplEx /
# RotatE 20)
BASE = (Case("TransE", 37), Case("DistMult", 40), Case("ComplEx", 20), Case("RotatE", 20), Case("pRotatE", 40),
        Case("pRotatE", 37, R=130))
# relation counts of one chunk, of several, with a partial last chunk; R = 1: rank 1, ties 0
COUNTS = tuple(Case("DistMult", 40, R=r, nq=5) for r in (1, 2, 7, 61, 64, 65, 130, 1500)) + \
    (Case("TransE", 37, R=65, nq=5), Case("TransE", 37, R=1500, nq=5))
# every staging variant of the kernel: 16-byte slots prefetched in 4 / 8 / 16
# registers per lane (rows of <= 128 / 256 / 512 slots: BASE, DistMult 600,
# RotatE 1000) or staged without prefetch (DistMult 2400); single-float slots
# likewise (TransE 37 / 203 / 301 / 2051); rows read in place (RotatE 9000: a
# 72 KB row)
WIDTHS = (Case("RotatE", 1000, R=9, nq=8), Case("DistMult", 600, R=20, nq=6), Case("DistMult", 2400, R=12, E=64, nq=4),
          Case("TransE", 203, R=20, nq=6), Case("TransE", 301, R=20, nq=6), Case("TransE", 2051, R=12, E=64, nq=4),
          Case("RotatE", 9000, R=5, E=64, nq=4))
UNALIGNED = (Case("DistMult", 40, aligned=False), Case("RotatE", 20, aligned=False), Case("TransE", 37, aligned=False))
# relation rows of exactly 256 | 257 slots, the second step of the prefetch
# ladder, of both slot kinds (rank_candidates_cases.BOUNDARY): two chunks of 35
BOUNDARY = (Case("DistMult", 1024, R=70, E=200, nq=5), Case("DistMult", 1028, R=70, E=200, nq=5),
            Case("DistMult", 256, R=70, E=200, nq=5, aligned=False), Case("DistMult", 257, R=70, E=200, nq=5))
PLANTED = tuple(Case(n, d, plant=True) for n, d in (("TransE", 37), ("DistMult", 40), ("ComplEx", 20), ("RotatE", 20)))
PRED =(Case("DistMult", 40, pred=True), Case("RotatE", 20, pred=True))
# one call past the 65,535-query ceiling of the other ranking entry points
MANY = (Case("TransE", 8, R=3, E=50, nq=70001),)
EXACT_CASES = tuple(c for c in BASE if c.name != "pRotatE") + COUNTS + WIDTHS + UNALIGNED + BOUNDARY + \
    PLANTED + PRED + MANY
PROTATE_CASES = tuple(c for c in BASE if c.name == "pRotatE")
ALL_CASES = EXACT_CASES + PROTATE_CASES


def sin_rn(a):
    """The float64 sin rounded once to fp32: the device's sin_rn."""
    return np.sin(np.asarray(a, dtype=np.float64)).astype(np.float32)


# nudged copy i of the N_NUDGE · N_TRUE is scaled by 1 ± 2^-x: twelve of 8..21, the finest all there
NUDGE_EXP = (8, 10, 11, 12, 13, 15, 16, 17, 18, 19, 20, 21)


def nudge_exponent(i):
    return NUDGE_EXP[i]


@lru_cache(maxsize=None)
def tables(case):
    """(ent [E, Le], rel [R, Lr], modulus or None, erange), float32, read-only."""
    ent, rel, mod, erange = synth_tables(case.name, case.E, case.R, case.d, GAMMA, case.seed)
    if case.plant:
        assert case.name != "pRotatE" and case.R >= BG0 + 16
        lr = dims(case.name, case.d)[1]
        for e in range(N_TRUE):
            rel[N_TRUE + N_COPY * e:N_TRUE + N_COPY * (e + 1)] = rel[e]
            for k in range(N_NUDGE):
                i = N_NUDGE * e + k
                row = rel[e].copy()
                f = np.float32(2.0 ** -nudge_exponent(i))
                f = np.float32(1.0) + f if i % 2 == 0 else np.float32(1.0) - f
                for c in range(3):
                    row[(7 * i + 11 * c) % lr] *= f
                rel[N_TRUE + N_COPY * N_TRUE + i] = row
    for x in (ent, rel):
        x.setflags(write=False)
    return ent, rel, mod, erange


@lru_cache(maxsize=None)
def queries(case):
    g = np.random.default_rng(case.seed + 100)
    q = np.stack([g.integers(0, case.E, case.nq), g.integers(0, case.R, case.nq), g.integers(0, case.E, case.nq)],
                 1).astype(np.int64)
    if case.plant:
        j = np.arange(N_PLANTED_Q)
        q[j, 1] = j % N_TRUE
    if case.pred:
        assert case.nq >= 6
        q[2, 1] = q[5, 1] = -1
    q.setflags(write=False)
    return q


def planted_excluded(j):
    """The exact copies query j < N_PLANTED_Q excludes: the first 1 + j mod 3 of its true row's."""
    e = j % N_TRUE
    return [N_TRUE + N_COPY * e + c for c in range(1 + j % 3)]


@lru_cache(maxsize=None)
def filt(case):
    """(off [nq + 1], ids) int64: every query's list of relation ids to exclude."""
    g = np.random.default_rng(case.seed + 400)
    q = queries(case)
    lo = BG0 if case.plant else 0
    rows = []
    for j in range(case.nq):
        if j == case.nq // 2:
            rows.append([])
            continue
        bg = g.integers(lo, case.R, min(5, case.R)).tolist() if case.R > lo else []
        row = bg + ([bg[0]] if bg and j % 4 == 0 else [])
        if q[j, 1] >= 0:
            row.append(int(q[j, 1]))
        row.append(case.R + j)
        if case.plant and j < N_PLANTED_Q:
            row += planted_excluded(j)
        rows.append(g.permutation(np.asarray(row, dtype=np.int64)).tolist())
    off = np.zeros(case.nq + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    ids = np.asarray([x for r in rows for x in r], dtype=np.int64)
    off.setflags(write=False)
    ids.setflags(write=False)
    return off, ids


@lru_cache(maxsize=None)
def excluded(case):
    """[nq, R] bool: relation r' is on query q's filter list."""
    off, ids = filt(case)
    m = np.zeros((case.nq, case.R), dtype=bool)
    owner = np.repeat(np.arange(case.nq), np.diff(off))
    ok = (ids >= 0) & (ids < case.R)
    m[owner[ok], ids[ok]] = True
    m.setflags(write=False)
    return m


def all_relation_triples(q, R):
    """[nq·R, 3]: (h, r', t) for every query and every r' in ascending order."""
    nq = len(q)
    tr = np.empty((nq, R, 3), dtype=np.int64)
    tr[:, :, 0] = q[:, :1]
    tr[:, :, 1] = np.arange(R)[None, :]
    tr[:, :, 2] = q[:, 2:]
    return tr.reshape(nq * R, 3)


@lru_cache(maxsize=None)
def scores(case):
    """[nq, R] float32: the oracle's reference-order 'single' score of (h, r', t)."""
    ent, rel, mod, erange = tables(case)
    tr = torch.from_numpy(all_relation_triples(queries(case), case.R))
    trig = (None, sin_rn) if case.name == "pRotatE" else None
    s = O.ref_order_scores(case.name, ent.copy(), rel.copy(), mod, tr, "single", GAMMA, erange, trig=trig)
    s = np.ascontiguousarray(np.asarray(s, dtype=np.float32).reshape(case.nq, case.R))
    s.setflags(write=False)
    return s


def count(s, r, excl=None):
    """(ranks int64, ties int32) of score rows [n, R] for the true relations r [n]
    (-1: rank 0, ties 0), over the relations other than r that `excl` [n, R] does
    not exclude."""
    n, R = s.shape
    has = r >= 0
    st = s[np.arange(n), np.where(has, r, 0)][:, None]
    valid = (np.arange(R)[None, :] != r[:, None]) & has[:, None]
    if excl is not None:
        valid = valid & ~excl
    ranks = np.where(has, 1 + (valid & (s > st)).sum(1), 0).astype(np.int64)
    ties = (valid & (s == st)).sum(1).astype(np.int32)
    return ranks, ties


@lru_cache(maxsize=None)
def reference(case, filtered):
    ranks, ties = count(scores(case), queries(case)[:, 1], excluded(case) if filtered else None)
    ranks.setflags(write=False)
    ties.setflags(write=False)
    return ranks, ties


def float_ord(x):
    """Monotone integer image of fp32 values (±0 → 0): ulp distances by subtraction."""
    b = np.asarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(b >= 0, b, -(b & 0x7fffffff))


def excusable(case, ulps=4):
    """[nq] bool: the oracle has a relation other than the true one within `ulps`
    of the true score (pRotatE: the device's sin may differ from the oracle's in
    the last bit there)."""
    s, r = scores(case), queries(case)[:, 1]
    has = r >= 0
    st = s[np.arange(case.nq), np.where(has, r, 0)][:, None]
    near = np.abs(float_ord(s) - float_ord(st)) <= ulps
    other = np.arange(case.R)[None, :] != r[:, None]
    return (near & other).any(1) & has


def topk_reference(s, k, excl=None):
    """(ids [n, k] int64, scores [n, k] float32): a stable sort of the score rows
    by (score descending, id ascending) over the relations `excl` does not
    exclude and whose score is not NaN, padded with (-1, -inf)."""
    n, R = s.shape
    ids = np.full((n, k), -1, dtype=np.int64)
    sc = np.full((n, k), -np.inf, dtype=np.float32)
    for i in range(n):
        ok = ~np.isnan(s[i]) & (True if excl is None else ~excl[i])
        cand = np.nonzero(ok)[0]
        o = cand[np.argsort(-s[i, cand].astype(np.float64), kind="stable")][:k]
        ids[i, :len(o)], sc[i, :len(o)] = o, s[i, o]
    return ids, sc
