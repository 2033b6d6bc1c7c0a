"""Shared inputs of the near-tie list tests (test_rank_ties_ref.py on the CPU,
test_rank_ties_gpu.py on the device): one table per case whose queries put a
chosen number of candidates into the ranking's near-tie list, at and past its
1024-entry cap (KGE_RANK_LIST_CAP), and the ranks and tie counts the fp32
reference-order oracle gives them.

The table (entity ids in this order):
  plants      C = 1100 exact copies of one row A (synth row 0): every one
              scores exactly the true score of a query whose true entity is a
              plant;
  nudged      U + D = 24 + 24 copies of A with three coordinates scaled by
              1 ± 2^-(8 + k mod 14) (+ for the first U): near-ties of mixed
              outcome (above, equal, below) once re-scored in reference order;
  shelf       (pRotatE only) copies of A with one phase coordinate moved so
              that the float64 score leaves the true score by ± T·f;
  background  B untouched synthetic rows;
  last        one more exact copy of A as entity E − 1, never filtered and
              never a query's true entity: with E odd it is the candidate
              that k_rank_exact's two-candidates-per-step loop takes alone.
E = C + U + D + shelf + B + 1 is odd and no multiple of 32.  Every relation
row is a copy of relation row 0 and query j is (h_j, r = j, t_j) with both
ends plants, so all queries of a direction share one score row but each has
its own filter key.  Query j's filter removes C − 1 − p_j of the other plants
(a seeded permutation: filtered and unfiltered bits interleave inside the
32-bit filter words and the 64-candidate tiles) and leaves p_j of them, so
the query lists p_j + x candidates, x the non-plants inside the path's
window, 1 ≤ x ≤ N_other = E − C.  The ladder of p_j holds a few small values
and every integer of [1024 − N_other, 1030]: whatever x a path has, one query
lists exactly 1024 and one 1025.
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

from conftest import dims, synth_tables
from oracle import kge_oracle as O

MODES = ("head-batch", "tail-batch")
CAP = 1024  # KGE_RANK_LIST_CAP
C = 1100
GAMMA = 12.0
SEED = 3
SMALL_P = (0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1099)


@dataclass(frozen=True)
class Case:
    name: str
    d: int
    paths: tuple = ("auto",)
    U: int = 24
    D: int = 24
    B: int = 48
    shelf: int = 0        # pRotatE: shelf rows
    shelf_T: float = 0.0  # their distance scale, in units of 2^-24 · |modulus|
    aligned: bool = True  # False: the entity table one float past a 16-byte boundary

    @property
    def id(self):
        return f"{self.name}-d{self.d}" + ("" if self.aligned else "-unaligned") + ("-shelf" if self.shelf else "")

    @property
    def n_other(self):
        return self.U + self.D + self.shelf + self.B + 1

    @property
    def n_loose(self):
        """Non-plants that a window may or may not list (the shelf rows are
        always inside the fast window and always decided by the screen)."""
        return self.U + self.D + self.B + 1

    @property
    def E(self):
        return C + self.n_other


def _wide(name, d, paths=("auto",)):
    # rows of 1000 floats and more: plants and background only (the oracle row
    # and the kernels stay under a few seconds), N_other = 17
    return Case(name, d, paths, U=0, D=0, B=16)


BIL = ("auto", "mfma32", "tile", "scan")
CASES = (
    Case("TransE", 32, ("auto", "scan")),
    Case("DistMult", 32, BIL),
    Case("DistMult", 37, ("auto", "scan")),
    Case("ComplEx", 16, BIL),
    Case("RotatE", 16, ("auto", "scan")),
    _wide("RotatE", 1000),
    _wide("DistMult", 1100, ("auto", "mfma32", "scan")),
    _wide("RotatE", 1500),
    _wide("TransE", 2051),
    _wide("RotatE", 3700),
    Case("DistMult", 32, ("auto",), aligned=False),
)
BOTH_CASES = tuple(c for c in CASES if c.aligned and (c.name, c.d) in (("DistMult", 32), ("RotatE", 16),
                                                                         ("TransE", 32)))
# shelf_T: see test_rank_ties_gpu.test_protate_shelf
PROTATE_PLANTS = Case("pRotatE", 32, ("auto",), U=0, D=0)
PROTATE_SHELF = Case("pRotatE", 32, ("auto",), U=0, D=0, shelf=1100, shelf_T=1000.0)
ALL_CASES = CASES + (PROTATE_PLANTS, PROTATE_SHELF)


def ladder(case):
    """p_j per query: the small values, then every integer of
    [1024 − N_other, 1030] (N_other without pRotatE's shelf rows); one more
    query when the count is a multiple of 4 (k_rank_exact ranks four queries
    per block: the last block stays partial)."""
    p = list(SMALL_P) + list(range(CAP - case.n_loose, CAP + 7))
    if len(p) % 4 == 0:
        p.append(700)
    return np.asarray(p, dtype=np.int64)


def _shelf_rows(case, ent, rel, mod, erange):
    """case.shelf copies of A = ent[0] with one phase coordinate each moved by
    a bisected amount: the float64 tail-batch score of (A, rel 0, row)
    leaves the true score by sign_i · T · f_i, T = shelf_T · 2^-24 · |modulus|,
    f_i log-uniform in [0.5, 2], sign alternating.  (Head-batch scores the same
    phase differences up to sign, so the rows sit at the same distances there.)"""
    g = np.random.default_rng(SEED + 41)
    m = abs(float(mod[0, 0]))
    T = case.shelf_T * 2.0 ** -24 * m
    div = float(np.float32(erange / O.PI_PROTATE))
    a64, r64 = ent[0].astype(np.float64), rel[0].astype(np.float64)

    def score(row):  # γ − |modulus| Σ |sin((h + r − t) / div)|
        return GAMMA - m * np.abs(np.sin((a64 + r64 - row) / div)).sum()

    true64 = score(a64)
    rows = np.repeat(ent[:1], case.shelf, 0)
    # coordinates whose |sin| is monotone over the whole step below (away from
    # its kink at 0 and its flat top)
    ph = r64 / div
    good = np.nonzero((np.abs(np.cos(ph)) > 0.25) & (np.abs(np.sin(ph)) > 0.1))[0]
    assert len(good) >= 8
    for i in range(case.shelf):
        want = (1.0 if i % 2 == 0 else -1.0) * T * 2.0 ** g.uniform(-1.0, 1.0)
        k = good[(5 * i) % len(good)]
        base = a64.copy()
        # find the direction that moves the score the wanted way
        step = 64.0 * abs(want) * div / m
        sgn = None
        for s in (1.0, -1.0):
            base[k] = a64[k] + s * step
            if (score(base) - true64) * want > 0 and abs(score(base) - true64) > abs(want):
                sgn = s
                break
        assert sgn is not None, (i, k)
        lo, hi = 0.0, step
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            base[k] = a64[k] + sgn * mid
            if abs(score(base) - true64) < abs(want):
                lo = mid
            else:
                hi = mid
        rows[i, k] = np.float32(a64[k] + sgn * hi)
    return rows


@lru_cache(maxsize=None)
def tables(case):
    """(ent [E, Le], rel [nq, Lr], modulus or None, erange), float32, read-only."""
    nq = len(ladder(case))
    ent, rel, mod, erange = synth_tables(case.name, case.E, nq, case.d, GAMMA, SEED)
    le = dims(case.name, case.d)[0]
    a = ent[0].copy()
    ent[:C] = a
    for k in range(case.U + case.D):
        row = a.copy()
        f = np.float32(2.0 ** -(8 + k % 14))
        f = np.float32(1.0) + f if k < case.U else np.float32(1.0) - f
        for c in range(3):
            row[(7 * k + 11 * c) % le] *= f
        ent[C + k] = row
    ent[case.E - 1] = a
    rel[:] = rel[0]
    if case.shelf:
        s0 = C + case.U + case.D
        ent[s0:s0 + case.shelf] = _shelf_rows(case, ent, rel, mod, erange)
    for x in (ent, rel):
        x.setflags(write=False)
    return ent, rel, mod, erange


@lru_cache(maxsize=None)
def queries(case):
    """[nq, 3]: (h_j, j, t_j), both ends plants, h_j ≠ t_j."""
    j = np.arange(len(ladder(case)), dtype=np.int64)
    q = np.stack([(37 * j + 5) % C, j, (53 * j + 611) % C], 1)
    assert (q[:, 0] != q[:, 2]).all()
    q.setflags(write=False)
    return q


@lru_cache(maxsize=None)
def filtered_mask(case, mode):
    """[nq, E] bool: query j's filtered candidates — C − 1 − p_j plants other
    than its true entity, the first ones of a per-query seeded permutation."""
    q, p = queries(case), ladder(case)
    m = np.zeros((len(q), case.E), dtype=bool)
    col = 0 if mode == "head-batch" else 2
    for j in range(len(q)):
        others = np.delete(np.arange(C), q[j, col])
        g = np.random.default_rng(1000 * (col + 1) + j)
        m[j, g.permutation(others)[:C - 1 - p[j]]] = True
    m.setflags(write=False)
    return m


@lru_cache(maxsize=None)
def true_triples(case):
    """all_true_triples: (e, j, t_j) for query j's filtered heads e and
    (h_j, j, e) for its filtered tails; the queries themselves are not in it."""
    q = queries(case)
    out = []
    for mode in MODES:
        j, e = np.nonzero(filtered_mask(case, mode))
        out.append(np.stack([e, j, q[j, 2]], 1) if mode == "head-batch" else np.stack([q[j, 0], j, e], 1))
    t = np.concatenate(out).astype(np.int64)
    t.setflags(write=False)
    return t


def _sample(case, mode):
    pos = torch.from_numpy(queries(case)[:1].copy())
    neg = torch.arange(case.E, dtype=torch.int64).unsqueeze(0)
    return pos, neg


@lru_cache(maxsize=None)
def score_row(case, mode):
    """(s [E] float32, s_true): the fp32 reference-order scores of every
    candidate, the same for every query of the direction (one q vector), from
    oracle.ref_order_scores (pinned bit for bit by test_oracle_golden.py)."""
    ent, rel, mod, erange = tables(case)
    s = O.ref_order_scores(case.name, ent.copy(), rel.copy(), mod, _sample(case, mode), mode, GAMMA, erange)
    s = np.ascontiguousarray(s.reshape(-1))
    assert s.dtype == np.float32 and s.shape == (case.E,)
    s.setflags(write=False)
    return s, s[0]


def forward_row(case, mode):
    """The same row from oracle.forward on the float32 tables."""
    ent, rel, mod, erange = tables(case)
    modt = None if mod is None else torch.from_numpy(mod)
    with torch.no_grad():
        s = O.forward(case.name, torch.from_numpy(ent.copy()), torch.from_numpy(rel.copy()), modt, _sample(case, mode), mode,
                      GAMMA, erange)
    return s.numpy().reshape(-1)


@lru_cache(maxsize=None)
def reference(case, mode):
    """(ranks int64 [nq], ties int32 [nq]): rank = 1 + #{kept: s > s_true},
    ties = #{kept: s == s_true}, kept = not filtered and not the true id."""
    s, st = score_row(case, mode)
    q = queries(case)
    keep = ~filtered_mask(case, mode)
    keep[np.arange(len(q)), q[:, 0 if mode == "head-batch" else 2]] = False
    ranks = 1 + (keep & (s > st)[None, :]).sum(1).astype(np.int64)
    ties = (keep & (s == st)[None, :]).sum(1).astype(np.int32)
    ranks.setflags(write=False)
    ties.setflags(write=False)
    return ranks, ties
