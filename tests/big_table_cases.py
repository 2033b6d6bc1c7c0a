"""Shared inputs and references of the big-table tests (test_big_table_ref.py on
the CPU, test_big_table_gpu.py on the device).  Importable without a GPU.

The table: pooled rows.  A table of E rows is `pool[idx]`: a pool of P = 8192
distinct rows drawn on the host like tests/topk_cases.tables (U(-range, range)
at the model's init range, gamma 12) and an index vector idx[E] of
pseudo-random pool indices; the device builds the table with one index_select.
A candidate's score depends on its row's contents alone, so the scores of all
E candidates are the [nq, P] pool scores expanded through idx, and a
reference exists on the CPU at any E.  Every duplicate of the true entity's
pool row is an exact tie: E / P of them per query on average.

The rows the queries point at (the `specials`: row 0, row E - 1 and, for
every line L the table crosses, the straddling row r_L = L // (4 * entity_dim)
and its two neighbours; and high rows) hold distinct pool rows of their own
choosing (_built: every true row is half a fit to its query, so it scores far
above the drawn rows and its near-ties are its own copies; planted rows that
fit better are what the ranks count), so a wrapped address, which lands on a
pseudo-random row, changes the result.  Pool row P - 1 is reserved: no idx entry draws it; the sentinel
case (S2 DistMult) writes +-3e38 into the four floats that lie at table byte
offset 0x7FFFFFF0 and gives it to the row at that offset.

Lines: L1 = 2^31 bytes, L2 = 2^32 bytes, L3 = 2^31 floats (2^33 bytes).
Every id list (query h and t = the true ids, negatives, candidates, filter
ids, training positives) takes at least half of its entries from rows at or
past r_L1 and includes every special.
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

from conftest import erange_of
from knowledgegraphembedding_amd import synth
from oracle import kge_oracle as O
from test_slot_matrix_ref import RHO_CAP, RTOL_MIN, rho_of

NAMES = ("TransE", "DistMult", "ComplEx", "RotatE", "pRotatE")
MODES = ("head-batch", "tail-batch")
DOUBLE = {"TransE": (1, 1), "DistMult": (1, 1), "ComplEx": (2, 2), "RotatE": (2, 1), "pRotatE": (1, 1)}
P, R, GAMMA = 8192, 6, 12.0
NQ, B, N, NCAND = 16, 8, 16, 40
KS = (10, 128)
L1, L2, L3 = 2 ** 31, 2 ** 32, 2 ** 33  # bytes; L3 is 2^31 floats
LINES = (L1, L2, L3)
SENTINEL = 0x7FFFFFF0  # the fp32 MFMA tile's former "no row" offset (kge_rank_mfma.hip OOB2)
HUGE = 3e38


@dataclass(frozen=True)
class Table:
    key: str
    E: int
    Le: int          # floats per row (entity_dim)
    P: int = P

    @property
    def nbytes(self):
        return self.E * self.Le * 4

    @property
    def lines(self):
        return tuple(L for L in LINES if L < self.nbytes)

    def straddle(self, L):
        return L // (4 * self.Le)

    @property
    def low(self):
        """The first row of the "high" half of every id list: the row straddling the
        lowest line the table crosses (a table under every line: its middle row)."""
        return self.straddle(self.lines[0]) if self.lines else self.E // 2

    @property
    def specials(self):
        out = [0, self.E - 1]
        for L in self.lines:
            r = self.straddle(L)
            out += [r - 1, r, r + 1]
        return np.array(out, dtype=np.int64)


TABLES = {t.key: t for t in (Table("S2", 540_000, 1000), Table("S4", 1_080_000, 1000), Table("S4odd", 1_080_000, 1001),
                             Table("S4wide", 530_000, 2051), Table("S8", 2_100_000, 1024))}
CROSSES = {"S2": (L1,), "S4": (L1, L2), "S4odd": (L1, L2), "S4wide": (L1, L2), "S8": (L1, L2, L3)}
SMALL = Table("small", 5000, 64, 256)  # the CPU check of the pooled reference materialises this one


def check_sizes():
    """The arithmetic of the issue's "crosses" column: a later edit of a shape cannot
    silently drop under its line."""
    for key, t in TABLES.items():
        assert t.lines == CROSSES[key], (key, t.nbytes)
        assert t.E < 2 ** 31 and t.nbytes < 2 ** 34  # (the 2^32-element line is out of scope)
        for L in t.lines:
            r = t.straddle(L)
            assert r * t.Le * 4 <= L < (r + 1) * t.Le * 4 and 1 <= r and r + 1 < t.E - 1, (key, L)
        assert len(set(t.specials.tolist())) == len(t.specials)
    s2, s4 = TABLES["S2"], TABLES["S4"]
    assert SENTINEL + 16 <= s2.nbytes < 0xFFFFFF00  # the fp32 MFMA tile admits S2, and the old sentinel is inside it
    assert s4.nbytes >= 0xFFFFFF00                  # ... and refuses S4
    assert TABLES["S4odd"].Le % 4 and TABLES["S4wide"].Le > 2048 and TABLES["S4wide"].Le % 4
    assert s2.straddle(L1) == (SENTINEL // 4) // s2.Le and (SENTINEL // 4) % s2.Le + 4 <= s2.Le


check_sizes()


@dataclass(frozen=True)
class Spec:
    """A model on a table."""
    table: Table
    name: str
    sentinel: bool = False

    @property
    def id(self):
        return f"{self.table.key}-{self.name}" + ("-sentinel" if self.sentinel else "")

    @property
    def d(self):
        return self.table.Le // DOUBLE[self.name][0]

    @property
    def Lr(self):
        return self.d * DOUBLE[self.name][1]

    @property
    def erange(self):
        return erange_of(GAMMA, self.d)

    @property
    def seed(self):
        return 1000 + 31 * (list(TABLES) + ["small"]).index(self.table.key) + NAMES.index(self.name)


def mod_of(sp):
    """pRotatE's modulus [1, 1] (tests/topk_cases.tables), None for the other models."""
    return np.array([[0.5 * sp.erange]], dtype=np.float32) if sp.name == "pRotatE" else None


def spec(key, name, sentinel=False):
    return Spec(TABLES[key] if key != "small" else SMALL, name, sentinel)


Q_TRUE, Q_PLANT = 0.5, 0.75  # how much of the fitted row a true row / a planted better row holds


def _rotation(sp, rel_row):
    ph = rel_row / (sp.erange / O.PI)
    return np.cos(ph), np.sin(ph)


def fitted(sp, other, rel_row, head):
    """The row (float64) that fits `other` and the relation best as the tail (head: as the
    head) of a triple: zero distance for TransE, RotatE and pRotatE, the direction of the
    largest score for DistMult and ComplEx."""
    name = sp.name
    if name in ("TransE", "pRotatE"):
        return other - rel_row if head else other + rel_row
    if name == "DistMult":
        return other * rel_row
    d = len(other) // 2
    xr, xi = other[:d], other[d:]
    c, s_ = _rotation(sp, rel_row) if name == "RotatE" else (rel_row[:d], rel_row[d:])
    if head:  # (c, s) conjugate times t
        return np.concatenate([c * xr + s_ * xi, c * xi - s_ * xr])
    return np.concatenate([xr * c - xi * s_, xr * s_ + xi * c])


def blended(sp, fit, drawn, q):
    """q of the fitted row and 1 - q of the drawn one (DistMult, ComplEx: the fitted
    direction at the drawn row's length), as float32."""
    if sp.name in ("DistMult", "ComplEx"):
        fit = fit * (np.linalg.norm(drawn) / np.linalg.norm(fit))
    return (q * fit + (1.0 - q) * drawn).astype(np.float32)


@lru_cache(maxsize=4)
def _built(sp):
    """(pool, rel, {id: pool row}).  The pool is drawn, then the rows the queries point at
    are chosen.  A query's h holds the row its id already has (the chain's earlier query made
    it) or a drawn row; its t holds a new row, Q_TRUE of the fit to (h, r) and the rest a
    drawn row, so the true score lies far above the drawn rows' in both directions and a
    query's near-ties are its true row's copies: the kernels' near-tie lists stay under their
    cap (at the init range a mid-ranked query lists thousands and takes the exact rescan of
    all E candidates, seconds per query at these sizes).  j % 3 planted rows per query and
    direction hold Q_PLANT of the fit: like every pool row they are drawn by idx all over
    the table, and their copies are what the ranks count."""
    t = sp.table
    assert t.Le % DOUBLE[sp.name][0] == 0
    pool, rel = synth.kge_tables(sp.seed, t.P, R, t.Le, sp.Lr, sp.erange)
    r64 = rel.astype(np.float64)
    rows, k = {}, 0

    def make(fit, q):
        nonlocal k
        slot, k = 3 * k + 1, k + 1
        pool[slot] = blended(sp, fit, pool[slot].astype(np.float64), q)
        return slot

    for j, (h, r, tl) in enumerate(queries(sp).tolist()):
        if h not in rows:
            rows[h] = t.P - 2 - j
        assert tl not in rows
        a = pool[rows[h]].astype(np.float64)
        rows[tl] = make(fitted(sp, a, r64[r], False), Q_TRUE)
        b = pool[rows[tl]].astype(np.float64)
        for _ in range(j % 3):
            make(fitted(sp, a, r64[r], False), Q_PLANT)
            make(fitted(sp, b, r64[r], True), Q_PLANT)
    assert 3 * k + 1 < t.P - 2 - NQ and len(set(rows.values())) == len(rows)
    if sp.sentinel:
        c = (SENTINEL // 4) % t.Le
        pool[t.P - 1, c:c + 4] = np.array([HUGE, -HUGE, HUGE, -HUGE], dtype=np.float32)
    assert len(np.unique(pool[:, :4], axis=0)) == t.P  # distinct rows
    pool.setflags(write=False)
    rel.setflags(write=False)
    return pool, rel, rows


def pool_of(sp):
    """(pool [P, Le], rel [R, Lr]) float32, read-only."""
    return _built(sp)[:2]


def rows_of(sp):
    return _built(sp)[2]


@lru_cache(maxsize=4)
def idx_of(sp):
    """idx [E] int64: the pool row every table row holds; the rows the queries point at
    hold the pool rows rows_of chooses."""
    t = sp.table
    idx = synth.randint(sp.seed + 500, (t.E,), t.P - 1)
    rows = rows_of(sp)
    idx[np.fromiter(rows.keys(), dtype=np.int64)] = np.fromiter(rows.values(), dtype=np.int64)
    if sp.sentinel:
        idx[(SENTINEL // 4) // t.Le] = t.P - 1
    idx.setflags(write=False)
    return idx


def wrapped_rows(t, L):
    """[E]: the row a byte offset e * 4 * Le truncated at line L addresses (2^31 and 2^32
    bytes: a 32-bit byte offset, signed or not; 2^33 bytes: a 31-bit element offset)."""
    off = np.arange(t.E, dtype=np.int64) * (4 * t.Le)
    return (off % L) // (4 * t.Le)


def eff_of(sp, line=None):
    """idx, or with `line` the pool row a kernel whose offsets wrap at that line would read."""
    idx = idx_of(sp)
    return idx if line is None else idx[wrapped_rows(sp.table, line)]


def materialise(sp):
    """The table itself (small tables only)."""
    assert sp.table.nbytes < 1 << 28
    return pool_of(sp)[0][idx_of(sp)]


# ------------------------------------------------------------------ id lists
def fill_ids(t, n, seed, must):
    """n ids: `must`, then pseudo-random rows at or past t.low; at least half are high."""
    must = np.asarray(must, dtype=np.int64)
    assert len(must) <= n
    out = np.concatenate([must, t.low + synth.randint(seed, (n - len(must),), t.E - t.low)])
    assert 2 * int((out >= t.low).sum()) >= n
    return out


def check_list(t, ids):
    """An id list as the issue wants it: every special, at least half from the high rows."""
    ids = np.asarray(ids).reshape(-1)
    ids = ids[ids >= 0]
    assert set(t.specials.tolist()) <= set(ids.tolist())
    assert 2 * int((ids >= t.low).sum()) >= len(ids)
    assert ids.max() < t.E


def shuffled(a, seed):
    return a[np.argsort(synth.randint(seed, (len(a),), 1 << 40), kind="stable")]


def distinct_high(t, seed, n):
    """n distinct pseudo-random rows at or past t.low, no special among them."""
    draw = t.low + synth.randint(seed, (8 * n,), t.E - t.low)
    draw = draw[~np.isin(draw, t.specials)]
    out = draw[np.sort(np.unique(draw, return_index=True)[1])][:n]
    assert len(out) == n
    return out


@lru_cache(maxsize=None)
def queries(sp, nq=NQ):
    """[nq, 3] with every id distinct.  The specials form a chain: query j + 1 is
    (s_j, r, s_j+1), between a high row in front and one behind, so h and t each hold every
    special (the sentinel case: but the huge row, whose own products overflow); the other
    queries pair high rows."""
    t = sp.table
    s = t.specials
    if sp.sentinel:
        s = np.where(s == (SENTINEL // 4) // t.Le, s + 2, s)
    rnd = distinct_high(t, sp.seed + 1, 2 * nq)
    rnd = rnd[~np.isin(rnd, s)]
    chain = np.concatenate([rnd[:1], s, rnd[1:2]])
    rest = rnd[2:2 + 2 * (nq - len(chain) + 1)].reshape(-1, 2)
    h, tl = np.concatenate([chain[:-1], rest[:, 0]]), np.concatenate([chain[1:], rest[:, 1]])
    q = np.stack([h, np.arange(nq) % R, tl], 1).astype(np.int64)
    assert q.shape == (nq, 3) and len(set(q[:, [0, 2]].reshape(-1).tolist())) == len(chain) + 2 * len(rest)
    if not sp.sentinel:
        check_list(t, q[:, 0]), check_list(t, q[:, 2])
    q.setflags(write=False)
    return q


ALL_FILTERED = 3  # the query whose filter holds every id but the true one


@lru_cache(maxsize=None)
def filters(sp, mode, nq=NQ):
    """Per-query lists (offsets [nq + 1], ids): three specials and three high rows each,
    the true id too on even queries; query ALL_FILTERED: everything but the true id."""
    t = sp.table
    q = queries(sp, nq)
    true = q[:, 0 if mode == "head-batch" else 2]
    s = t.specials
    lists = []
    for i in range(nq):
        if i == ALL_FILTERED:
            ids = np.delete(np.arange(t.E, dtype=np.int64), true[i])
        else:
            ids = fill_ids(t, 6, sp.seed + 40 + 2 * i + (mode == "head-batch"), s[(3 * i + np.arange(3)) % len(s)])
            if i % 2 == 0:
                ids = np.append(ids, true[i])
            ids = np.unique(ids)
        lists.append(ids)
    off = np.zeros(nq + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    ids = np.concatenate(lists)
    check_list(t, np.concatenate([x for i, x in enumerate(lists) if i != ALL_FILTERED]))
    for a in (off, ids):
        a.setflags(write=False)
    return off, ids


def id_matrix(sp, rows, n, seed, hot=0):
    """[rows, n] ids holding every special; `hot`: that many places hold row E - 1."""
    t = sp.table
    flat = shuffled(fill_ids(t, rows * n, seed, t.specials), seed + 1)
    if hot:
        flat[np.nonzero(~np.isin(flat, t.specials))[0][:hot]] = t.E - 1
        flat = shuffled(flat, seed + 2)
    check_list(t, flat)
    return flat.reshape(rows, n)


@lru_cache(maxsize=None)
def negatives(sp, rows=NQ, n=N, hot=0):
    m = id_matrix(sp, rows, n, sp.seed + 80 + n, hot)
    m.setflags(write=False)
    return m


@lru_cache(maxsize=None)
def candidates(sp, mode):
    """[NQ, NCAND]: ids with every special, -1 padding in three places and a copy of the
    true id in every fourth row."""
    q = queries(sp)
    c = id_matrix(sp, NQ, NCAND, sp.seed + 90 + (mode == "head-batch")).copy()
    free = ~np.isin(c, sp.table.specials)  # (the places written below hold no special)
    for row, k in ((1, 0), (5, 17), (9, -1)):
        c[row, np.nonzero(free[row])[0][k]] = -1
    for row in range(0, NQ, 4):
        c[row, np.nonzero(free[row])[0][7]] = q[row, 0 if mode == "head-batch" else 2]
    check_list(sp.table, c)
    c.setflags(write=False)
    return c


@lru_cache(maxsize=None)
def train_batch(sp, n=N, hot=0):
    """(pos [B, 3], neg [B, n], w [B]): h and t together hold every special; with `hot`,
    row E - 1 occurs more than 64 times among the negatives (a hot bucket)."""
    t = sp.table
    ht = shuffled(fill_ids(t, 2 * B, sp.seed + 60, t.specials), sp.seed + 61)
    if (ht[:B] == ht[B:]).any():
        ht[B:] = np.roll(ht[B:], 1)
    assert (ht[:B] != ht[B:]).all()
    pos = np.stack([ht[:B], np.arange(B) % R, ht[B:]], 1).astype(np.int64)
    check_list(t, ht)
    neg = np.array(negatives(sp, B, max(n, 16), hot))[:, :n] if n >= 16 else None
    if neg is None:  # few negatives cannot hold every special: the positives do
        neg = t.low + synth.randint(sp.seed + 62, (B, n), t.E - t.low)
        neg[0, 0], neg[1, 0] = t.E - 1, t.straddle(t.lines[-1])
    if hot:
        assert int((neg == t.E - 1).sum()) > 64
    w = synth.uniform(sp.seed + 63, (B,), 0.1, 0.4)
    for a in (pos, neg, w):
        a.setflags(write=False)
    return pos, neg, w


# -------------------------------------------------------- pooled references
def _pool_queries(q, eff):
    qp = np.array(q, dtype=np.int64)
    qp[:, 0], qp[:, 2] = eff[q[:, 0]], eff[q[:, 2]]
    return qp


@lru_cache(maxsize=1024)
def _pool_row(sp, mode, h, r, t, double):
    """[P] scores of every pool row as the candidate of one query whose other entity is
    pool row h (tail-batch) or t (head-batch); the predicted column is not read."""
    pool, rel = pool_of(sp)
    mod = mod_of(sp)
    pos = torch.tensor([[h, r, t]], dtype=torch.int64)
    neg = torch.arange(pool.shape[0], dtype=torch.int64).unsqueeze(0)
    if double:
        m64 = None if mod is None else torch.from_numpy(mod.astype(np.float64))
        out = O.forward(sp.name, torch.from_numpy(pool.astype(np.float64)), torch.from_numpy(rel.astype(np.float64)),
                        m64, (pos, neg), mode, GAMMA, sp.erange).numpy()[0]
    else:
        out = np.ascontiguousarray(O.ref_order_scores(sp.name, pool.copy(), rel.copy(), mod, (pos, neg), mode, GAMMA,
                                                      sp.erange)[0], dtype=np.float32)
    out.setflags(write=False)
    return out


def pool_scores(sp, qp, mode, double):
    """[nq, P] scores of every pool row as the candidate of queries `qp` (h and t already
    pool rows): reference-order fp32 (oracle.ref_order_scores) or the fp64 oracle.  One
    query at a time ([P, Le] temporaries), each computed once."""
    head = mode == "head-batch"
    return np.stack([_pool_row(sp, mode, 0 if head else int(h), int(r), int(t) if head else 0, double)
                     for h, r, t in qp])


@lru_cache(maxsize=8)
def pool_s32(sp, mode, line=None):
    s = pool_scores(sp, _pool_queries(queries(sp), eff_of(sp, line)), mode, False)
    s.setflags(write=False)
    return s


@lru_cache(maxsize=8)
def pool_s64(sp, mode, line=None, nq=NQ):
    s = pool_scores(sp, _pool_queries(queries(sp)[:nq], eff_of(sp, line)), mode, True)
    s.setflags(write=False)
    return s


def counts_from_pool(S, eff, true, off, ids):
    """(ranks int64, ties int32) from pool scores S [nq, P]: the unfiltered candidates
    other than the true id, counted per pool row."""
    Pn = S.shape[1]
    every = np.bincount(eff, minlength=Pn)
    ranks, ties = np.empty(len(S), dtype=np.int64), np.empty(len(S), dtype=np.int32)
    for i in range(len(S)):
        out = np.union1d(ids[off[i]:off[i + 1]], true[i:i + 1])
        cnt = every - np.bincount(eff[out], minlength=Pn)
        assert (cnt >= 0).all()
        st = S[i, eff[true[i]]]
        ranks[i] = 1 + cnt[S[i] > st].sum()
        ties[i] = cnt[S[i] == st].sum()
    return ranks, ties


@lru_cache(maxsize=None)
def rank_reference(sp, mode, line=None):
    """Filtered ranks and tie counts in the reference's fp32 score order."""
    q = queries(sp)
    off, ids = filters(sp, mode)
    out = counts_from_pool(pool_s32(sp, mode, line), eff_of(sp, line), q[:, 0 if mode == "head-batch" else 2], off, ids)
    for a in out:
        a.setflags(write=False)
    return out


def filter_mask(sp, mode, nq=NQ):
    off, ids = filters(sp, mode)
    m = np.zeros((nq, sp.table.E), dtype=bool)
    for i in range(nq):
        m[i, ids[off[i]:off[i + 1]]] = True
    return m


def topk_reference(sp, mode, k, line=None, nq=NQ):
    """(ids [nq, k], scores) of the fp64 scores in (score descending, id ascending) order,
    padded with (-1, -inf)."""
    eff = eff_of(sp, line)
    S = pool_s64(sp, mode, line, nq)
    mask = filter_mask(sp, mode, nq)
    out_i = np.full((nq, k), -1, dtype=np.int64)
    out_s = np.full((nq, k), -np.inf)
    for i in range(nq):
        s = np.where(mask[i], -np.inf, S[i][eff])
        n = min(k, int((~mask[i]).sum()))
        if n == 0:
            continue
        part = np.nonzero(s >= np.partition(s, len(s) - n)[len(s) - n])[0]  # every tie of the n-th best too
        part = part[np.lexsort((part, -s[part]))][:n]
        out_i[i, :n], out_s[i, :n] = part, s[part]
    return out_i, out_s


# ---------------------------------------------------------------- compaction
def compact(sp, arrays, line=None):
    """The compacted problem of some id arrays: (uniq, ent [U, Le], the arrays with every
    id >= 0 replaced by its place in uniq).  uniq is sorted: the map preserves order."""
    valid = np.concatenate([np.asarray(a).reshape(-1) for a in arrays])
    uniq = np.unique(valid[valid >= 0])
    ent = pool_of(sp)[0][eff_of(sp, line)[uniq]]
    mapped = [np.where(np.asarray(a) >= 0, np.searchsorted(uniq, np.maximum(np.asarray(a), 0)), -1) for a in arrays]
    return uniq, ent, mapped


def _t(a, dtype):
    return torch.from_numpy(np.array(a)).to(dtype)


def score_reference(sp, mode, line=None):
    """fp64 scores of ops.score's three modes on the gather inputs: queries as the
    positives, negatives() as the candidates."""
    q, neg = queries(sp), negatives(sp)
    _, ent, (h, tl, ng) = compact(sp, [q[:, 0], q[:, 2], neg], line)
    pos = torch.from_numpy(np.stack([h, q[:, 1], tl], 1))
    sample = pos if mode == "single" else (pos, torch.from_numpy(ng))
    return O.forward(sp.name, _t(ent, torch.float64), _t(pool_of(sp)[1], torch.float64), None, sample, mode, GAMMA,
                     sp.erange).numpy()


def candidates_reference(sp, mode, line=None):
    """(ranks, ties) of ops.rank_candidates as tests/rank_candidates_cases.py defines them."""
    q, c = queries(sp), candidates(sp, mode)
    true = q[:, 0 if mode == "head-batch" else 2]
    _, ent, (h, tl, cm, tm) = compact(sp, [q[:, 0], q[:, 2], c, true], line)
    ids = np.concatenate([tm[:, None], np.where(cm >= 0, cm, 0)], 1)
    pos = torch.from_numpy(np.stack([h, q[:, 1], tl], 1))
    s = O.ref_order_scores(sp.name, ent, np.array(pool_of(sp)[1]), None, (pos, torch.from_numpy(ids)), mode, GAMMA,
                           sp.erange)
    valid = c >= 0
    return (1 + (valid & (s[:, 1:] > s[:, :1])).sum(1).astype(np.int64),
            (valid & (s[:, 1:] == s[:, :1])).sum(1).astype(np.int32))


def relations_reference(sp, line=None):
    """(ranks, ties, fp32 reference-order scores [nq, R], fp64 scores) of ops.rank_relations
    without a filter, as tests/rank_relations_cases.py defines them."""
    q = queries(sp)
    _, ent, (h, tl) = compact(sp, [q[:, 0], q[:, 2]], line)
    tr = np.stack([np.repeat(h, R), np.tile(np.arange(R), len(q)), np.repeat(tl, R)], 1)
    rel = np.array(pool_of(sp)[1])
    s = O.ref_order_scores(sp.name, ent, rel, None, torch.from_numpy(tr), "single", GAMMA, sp.erange).reshape(len(q), R)
    s64 = O.forward(sp.name, _t(ent, torch.float64), _t(rel, torch.float64), None, torch.from_numpy(tr), "single",
                    GAMMA, sp.erange).numpy().reshape(len(q), R)
    st = s[np.arange(len(q)), q[:, 1]][:, None]
    other = np.arange(R)[None, :] != q[:, 1:2]
    return (1 + (other & (s > st)).sum(1).astype(np.int64), (other & (s == st)).sum(1).astype(np.int32), s, s64)


# ------------------------------------------------------------------ training
@dataclass(frozen=True)
class Train:
    key: str
    name: str
    mode: str
    n: int = N
    hot: int = 0
    regularization: float = 0.0
    entry: str = "grads"  # grads | adam | lazy | adagrad-row | adagrad-elem

    @property
    def spec(self):
        return spec(self.key, self.name)

    @property
    def id(self):
        return f"{self.entry}-{self.key}-{self.name}-{self.mode}-n{self.n}" + ("-hot" if self.hot else "") + \
            ("-reg" if self.regularization else "")


ADV_T = 0.75  # the adversarial temperature of every training case (test_slot_matrix_ref's)
GRAD_CASES = [Train("S4", "RotatE", "tail-batch", hot=70), Train("S4", "DistMult", "head-batch", regularization=1e-4),
              Train("S4odd", "TransE", "head-batch", n=3), Train("S4wide", "TransE", "tail-batch")]


STEP_CASES = [Train("S4", "RotatE", "head-batch", entry="adam"), Train("S4", "RotatE", "tail-batch", entry="lazy"),
              Train("S8", "TransE", "tail-batch", entry="adagrad-row", hot=70),
              Train("S8", "RotatE", "head-batch", entry="adagrad-row"),
              Train("S4", "RotatE", "head-batch", entry="adagrad-elem")]


@dataclass
class TrainRef:
    uniq: np.ndarray
    ent: np.ndarray     # [U, Le] the compacted table
    pos: np.ndarray
    neg: np.ndarray
    w: np.ndarray
    gout: dict          # mode -> the upstream gradient of kge_score_backward
    losses: np.ndarray  # fp64 (positive, negative, loss) of the compacted problem (its own regulariser left out)
    grads: list         # fp64 [entity [U, Le], relation]
    backward: dict      # mode -> fp64 [entity, relation] under gout
    rho: float
    rtol: float


def _train_grads(ref_in, tc, dtype):
    sp, (ent, pos, neg, w) = tc.spec, ref_in
    log, ge, gr, _ = O.train_grads(tc.name, _t(ent, dtype), _t(pool_of(sp)[1], dtype), None, torch.from_numpy(pos),
                                   torch.from_numpy(neg), _t(w, dtype), tc.mode, adversarial=True, temperature=ADV_T,
                                   uni_weight=False, regularization=tc.regularization, gamma=GAMMA, erange=sp.erange)
    # (the regulariser of the compacted table is not the big table's: the callers add reg_reference)
    data_loss = (log["positive_sample_loss"] + log["negative_sample_loss"]) / 2
    return np.array([log["positive_sample_loss"], log["negative_sample_loss"], data_loss]), [ge.numpy(), gr.numpy()]


def _backward(ref_in, tc, mode, gout, dtype):
    sp, (ent, pos, neg, _) = tc.spec, ref_in
    E_, R_ = _t(ent, dtype).requires_grad_(True), _t(pool_of(sp)[1], dtype).requires_grad_(True)
    s = O.forward(tc.name, E_, R_, None, (torch.from_numpy(pos), torch.from_numpy(neg)), mode, GAMMA, sp.erange)
    s.backward(_t(gout, dtype))
    return [E_.grad.numpy(), R_.grad.numpy()]


@lru_cache(maxsize=2)
def train_reference(tc, backward=True):
    """The compacted problem of a training case, its fp64 oracle results and rtol_case
    (tests/test_slot_matrix_ref.py: max(8 rho_case, 32 * 2^-24), rho_case the fp32 oracle's
    own distance from fp64 on the same inputs, at most 5e-5)."""
    sp = tc.spec
    pos, neg, w = train_batch(sp, tc.n, tc.hot)
    uniq, ent, (h, tl, ng) = compact(sp, [pos[:, 0], pos[:, 2], neg])
    posc = np.stack([h, pos[:, 1], tl], 1)
    rin = (ent, posc, ng, np.array(w))
    l64, g64 = _train_grads(rin, tc, torch.float64)
    _, g32 = _train_grads(rin, tc, torch.float32)
    rho = max(rho_of(a, b) for a, b in zip(g32, g64))
    gout, bwd = {}, {}
    if backward:
        gout[tc.mode] = synth.uniform(sp.seed + 70, ng.shape, -1.0, 1.0)
        bwd[tc.mode] = _backward(rin, tc, tc.mode, gout[tc.mode], torch.float64)
        b32 = _backward(rin, tc, tc.mode, gout[tc.mode], torch.float32)
        rho = max([rho] + [rho_of(a, b) for a, b in zip(b32, bwd[tc.mode])])
    assert rho <= RHO_CAP, rho
    return TrainRef(uniq, ent, posc, ng, np.array(w), gout, l64, g64, bwd, rho, max(8.0 * rho, RTOL_MIN))


def reg_reference(sp, regularization):
    """regularization * (sum |e|^3 over the whole table + sum |r|^3) in double, from the pool
    and the number of rows that hold each pool row."""
    pool, rel = pool_of(sp)
    per_row = (np.abs(pool.astype(np.float64)) ** 3).sum(1)
    cnt = np.bincount(idx_of(sp), minlength=len(pool))
    return regularization * (float((cnt * per_row).sum()) + float((np.abs(rel.astype(np.float64)) ** 3).sum()))


# ------------------------------------------------------------- the GPU cases
RANK_CASES = {  # spec -> (paths that must agree, paths that must be refused)
    spec("S2", "DistMult"): (("mfma32", "tile", "scan", "auto"), ("mfma",)),
    spec("S2", "ComplEx"): (("mfma32", "tile", "scan", "auto"), ("mfma",)),
    spec("S4", "DistMult"): (("tile", "scan", "auto"), ("mfma", "mfma32")),
    spec("S4", "TransE"): (("tile", "scan", "auto"), ()),
    spec("S4", "RotatE"): (("tile", "scan", "auto"), ()),
    spec("S4odd", "TransE"): (("scan", "auto"), ("tile",)),
    spec("S4wide", "TransE"): (("auto",), ()),
    spec("S8", "TransE"): (("tile", "scan", "auto"), ()),
    spec("S8", "RotatE"): (("tile", "scan", "auto"), ()),
}
SENTINEL_CASE = spec("S2", "DistMult", sentinel=True)
TOPK_CASES = [spec("S4", "TransE"), spec("S4", "DistMult"), spec("S8", "RotatE")]
GATHER_CASES = [spec("S8", "TransE"), spec("S8", "RotatE"), spec("S4wide", "TransE")]
