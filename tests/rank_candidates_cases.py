"""Shared inputs of the candidate-list ranking tests (test_rank_candidates_ref.py
on the CPU, test_rank_candidates_gpu.py on the device): per case the tables,
the queries, each direction's candidate lists [nq, C] and the ranks and tie
counts the fp32 reference-order oracle gives them.

Expected values: oracle.ref_order_scores on the sample (queries, [true id |
cand]) in the call's mode — column 0 is the true score — counted over the
columns whose id is >= 0:  rank = 1 + #{s > s_true}, ties = #{s == s_true}.
Nothing else is excluded: a candidate equal to the true id is a tie.

Candidate rows are drawn with replacement from [0, E) and the true id is
written into one place of every third row, so lists hold duplicates and copies
of the true id.  `pad` cases carry -1 padding at the start, in the middle and
at the end of rows, and one row of padding only (rank 1, ties 0).

`plant` cases (TransE, DistMult, ComplEx, RotatE only) lay out the table as
  rows 0..15      the true rows: query j < 8 is (h = 2j, r, t = 2j + 1)
  rows 16..79     exact copies: 16 + 4·e + c, c < 4, is a copy of true row e
  rows 80..127    nudged copies: 80 + 3·e + k, k < 3, is true row e with three
                  coordinates scaled by 1 ± 2^-(8 + (3e + k) mod 14)
  rows 128..      untouched background
and query j's list holds 1 + j mod 4 exact copies of its true row, the true
id itself when j is odd, the three nudged copies and background ids — so the
exact copies give it 1 + j mod 4 + (j odd) ties (planned_ties); a nudged copy
is a near-tie that may round onto the true score as well.

pRotatE: the oracle takes sin as the float64 sin rounded once to fp32 (`rn`,
the device's sin_rn).  A query could be excused from exact agreement only if
the oracle has a candidate, other than a copy of the true id, within 4 ulp of
the true score; these inputs have no such query (test_rank_candidates_ref.py).
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

from conftest import dims, synth_tables
from oracle import kge_oracle as O

MODES = ("head-batch", "tail-batch")
GAMMA = 12.0
R = 7
N_TRUE, N_COPY, N_NUDGE, BG0 = 16, 4, 3, 128


@dataclass(frozen=True)
class Case:
    name: str
    d: int
    E: int = 301
    nq: int = 24
    C: int = 97
    seed: int = 5
    pad: bool = False
    plant: bool = False
    aligned: bool = True  # False: the entity table one float past a 16-byte boundary

    @property
    def id(self):
        return (f"{self.name}-d{self.d}-E{self.E}-nq{self.nq}-C{self.C}" + ("-pad" if self.pad else "")
                + ("-plant" if self.plant else "") + ("" if self.aligned else "-unaligned"))


# all five models: single-float slots (TransE 37), one full cascade row plus a
# tail vector (DistMult 40), tail vectors plus a scalar tail (ComplEx / RotatE 20)
BASE = (Case("TransE", 37), Case("DistMult", 40), Case("ComplEx", 20), Case("RotatE", 20), Case("pRotatE", 40),
        Case("pRotatE", 37))
# lists of one chunk, of several, with a partial last chunk
LENGTHS = tuple(Case("DistMult", 40, nq=5, C=c) for c in (1, 2, 31, 64, 65, 1500)) + \
    (Case("TransE", 37, nq=5, C=65), Case("TransE", 37, nq=5, C=1500))
PADDED = (Case("DistMult", 40, pad=True), Case("RotatE", 20, pad=True), Case("TransE", 37, pad=True))
# every staging variant of the kernel: 16-byte slots prefetched in 4 / 8 / 16
# registers per lane (rows of <= 128 / 256 / 512 slots: BASE, d = 600, RotatE
# 1000) or staged without prefetch (DistMult 2400); single-float slots
# likewise (TransE 37 / 203 / 301 / 2051); rows read in place (RotatE 9000:
# a 72 KB row).  TransE 2051 and RotatE 9000 sit either side of the LDS
# staging threshold.
WIDTHS = (Case("RotatE", 1000, nq=8, C=70), Case("DistMult", 600, nq=6, C=40), Case("DistMult", 2400, E=64, nq=4, C=20),
          Case("TransE", 203, nq=6, C=40), Case("TransE", 301, nq=6, C=40), Case("TransE", 2051, E=64, nq=4, C=20),
          Case("RotatE", 9000, E=64, nq=4, C=20))
UNALIGNED = (Case("DistMult", 40, aligned=False), Case("RotatE", 20, aligned=False))
# rows of exactly 128 | 129 slots, the first step of the prefetch ladder, of
# both slot kinds (rank_relations_cases.BOUNDARY has 256 | 257, rank_shard_cases
# 512 | 513 and over): two chunks of 35, more items than half-waves
BOUNDARY = (Case("DistMult", 512, E=200, nq=5, C=70), Case("DistMult", 516, E=200, nq=5, C=70),
            Case("DistMult", 128, E=200, nq=5, C=70, aligned=False), Case("DistMult", 129, E=200, nq=5, C=70))
PLANTED =tuple(Case(n, d, plant=True) for n, d in (("TransE", 37), ("DistMult", 40), ("ComplEx", 20), ("RotatE", 20)))
# one call past the 65,535-query ceiling of the other ranking entry points
MANY = (Case("TransE", 8, E=50, nq=70001, C=3),)
EXACT_CASES = tuple(c for c in BASE if c.name != "pRotatE") + LENGTHS + PADDED + WIDTHS + UNALIGNED + BOUNDARY + \
    PLANTED + MANY
PROTATE_CASES = tuple(c for c in BASE if c.name == "pRotatE")
ALL_CASES = EXACT_CASES + PROTATE_CASES


def sin_rn(a):
    """The float64 sin rounded once to fp32: the device's sin_rn."""
    return np.sin(np.asarray(a, dtype=np.float64)).astype(np.float32)


@lru_cache(maxsize=None)
def tables(case):
    """(ent [E, Le], rel [R, Lr], modulus or None, erange), float32, read-only."""
    ent, rel, mod, erange = synth_tables(case.name, case.E, R, case.d, GAMMA, case.seed)
    if case.plant:
        assert case.name != "pRotatE" and case.E > BG0 + 32
        le = dims(case.name, case.d)[0]
        for e in range(N_TRUE):
            ent[N_TRUE + N_COPY * e:N_TRUE + N_COPY * (e + 1)] = ent[e]
            for k in range(N_NUDGE):
                i = N_NUDGE * e + k
                row = ent[e].copy()
                f = np.float32(2.0 ** -(8 + i % 14))
                f = np.float32(1.0) + f if i % 2 == 0 else np.float32(1.0) - f
                for c in range(3):
                    row[(7 * i + 11 * c) % le] *= f
                ent[N_TRUE + N_COPY * N_TRUE + i] = row
    for x in (ent, rel):
        x.setflags(write=False)
    return ent, rel, mod, erange


@lru_cache(maxsize=None)
def queries(case):
    g = np.random.default_rng(case.seed + 100)
    lo = BG0 if case.plant else 0
    q = np.stack([g.integers(lo, case.E, case.nq), g.integers(0, R, case.nq), g.integers(lo, case.E, case.nq)],
                 1).astype(np.int64)
    if case.plant:
        j = np.arange(N_TRUE // 2)
        q[j, 0], q[j, 2] = 2 * j, 2 * j + 1
    q.setflags(write=False)
    return q


def true_ids(case, mode):
    return queries(case)[:, 0 if mode == "head-batch" else 2]


def planned_ties(case, mode):
    """[N_TRUE / 2] the ties the planted queries' exact copies (and the true id itself) give."""
    j = np.arange(N_TRUE // 2)
    return 1 + j % N_COPY + (j % 2 == 1)


@lru_cache(maxsize=None)
def cand(case, mode):
    """[nq, C] int64 candidate ids (-1: padding)."""
    g = np.random.default_rng(case.seed + (200 if mode == "head-batch" else 300))
    tid = true_ids(case, mode)
    c = g.integers(0, case.E, (case.nq, case.C)).astype(np.int64)
    for j in range(0, case.nq, 3):
        c[j, (5 * j) % case.C] = tid[j]
    if case.plant:
        assert case.C >= 16
        for j in range(N_TRUE // 2):
            e = int(tid[j])
            row = [N_TRUE + N_COPY * e + k for k in range(1 + j % N_COPY)]
            row += [e] if j % 2 == 1 else []
            row += [N_TRUE + N_COPY * N_TRUE + N_NUDGE * e + k for k in range(N_NUDGE)]
            row += g.integers(BG0, case.E, case.C - len(row)).tolist()
            c[j] = g.permutation(np.asarray(row, dtype=np.int64))
    if case.pad:
        assert case.nq >= 6 and case.C >= 16
        c[0, :5] = -1                           # start
        c[1, case.C // 2 - 3:case.C // 2 + 4] = -1  # middle
        c[2, -9:] = -1                          # end
        c[3, ::2] = -1                          # every other place
        c[4, :] = -1                            # padding only: rank 1, ties 0
        c[5, 0] = c[5, -1] = -1
    c.setflags(write=False)
    return c


@lru_cache(maxsize=None)
def scores(case, mode):
    """[nq, 1 + C] float32: the oracle's reference-order scores of [true id | cand]
    (padding places hold entity 0's score and are masked by the callers)."""
    ent, rel, mod, erange = tables(case)
    c = cand(case, mode)
    ids = np.concatenate([true_ids(case, mode)[:, None], np.where(c >= 0, c, 0)], 1)
    sample = (torch.from_numpy(queries(case).copy()), torch.from_numpy(ids))
    trig = (None, sin_rn) if case.name == "pRotatE" else None
    s = O.ref_order_scores(case.name, ent.copy(), rel.copy(), mod, sample, mode, GAMMA, erange, trig=trig)
    s = np.ascontiguousarray(s, dtype=np.float32)
    assert s.shape == ids.shape
    s.setflags(write=False)
    return s


def count(s, valid):
    """(ranks int64, ties int32) of score rows [n, 1 + C] over the valid columns."""
    st = s[:, :1]
    ranks = 1 + (valid & (s[:, 1:] > st)).sum(1).astype(np.int64)
    ties = (valid & (s[:, 1:] == st)).sum(1).astype(np.int32)
    return ranks, ties


@lru_cache(maxsize=None)
def reference(case, mode):
    ranks, ties = count(scores(case, mode), cand(case, mode) >= 0)
    ranks.setflags(write=False)
    ties.setflags(write=False)
    return ranks, ties


def float_ord(x):
    """Monotone integer image of fp32 values (±0 → 0): ulp distances by subtraction."""
    b = np.asarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(b >= 0, b, -(b & 0x7fffffff))


def excusable(case, mode, ulps=4):
    """[nq] bool: the oracle has a candidate, other than a copy of the true id,
    within `ulps` of the true score (pRotatE: the device's sin may differ from
    the oracle's in the last bit there)."""
    s, c = scores(case, mode), cand(case, mode)
    near = np.abs(float_ord(s[:, 1:]) - float_ord(s[:, :1])) <= ulps
    other = (c >= 0) & (c != true_ids(case, mode)[:, None])
    return (near & other).any(1)
