"""Near-tie lists at and past their 1024-entry cap (KGE_RANK_LIST_CAP) against
the fp32 reference-order oracle: the tables of tests/rank_tie_cases.py, whose
queries list p_j + x candidates each (p_j unfiltered plants — exact copies of
the true row — and x >= 1 others inside a path's window), with p_j laddered so that on
every path one query lists exactly 1024 candidates, one 1025, a dozen fewer
and some more.  Each path's ranks and tie counts are compared with the
oracle's directly (no tolerance, no path against another):

  * listed <= 1024: k_rank_refine re-scores the list — hundreds of items per
    half-wave slot, some above, some equal, some below the true score — at
    each of its row variants (prefetched float4 rows, PQ = 16 and 0; the
    scalar copy of odd rows; wide geometry; rows read in place);
  * listed > 1024: k_rank_exact rescans all E candidates (E odd: the last
    step of its two-candidates loop holds one, an exact tie) under a filter whose bits
    interleave with unfiltered ones inside the tie block, and k_rank_emit
    takes its counts — in the same launch as queries that did not overflow;
  * both directions in one call (BOTH_DIRS forms), with the device filter
    table and with per-query lists;
  * pRotatE's list stage: k_rank_exact_iv's "fits the list after the rescan"
    branch, at namb == cap and cap + 1.

The `listed` assertions are conditions on the input, not on the kernel: they
prove that the path crossed the cap edge.
"""
import numpy as np
import pytest
import torch

import rank_tie_cases as T
from knowledgegraphembedding_amd import _lib, ops
from knowledgegraphembedding_amd.filters import FilterIndex
from test_gpu_parity import DEV, build_model
from test_slot_matrix_gpu import unaligned

pytestmark = pytest.mark.gpu
SEEN = []  # (case, path, mode, min and max of listed − p_j, overflowed queries)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nrank ties: case, path, mode, min / max listed − p_j, queries past the cap")
    for row in SEEN:
        print("rank ties: %-22s %-12s %-10s %4d %4d %4d" % row)


def make(case):
    """(model, queries, filter index) of a case: build_model's KGEModel holding
    the case's tables."""
    ent, rel, mod, _ = T.tables(case)
    q = T.queries(case).copy()
    m, _, _, mod0, _ = build_model(case.name, case.E, len(q), case.d, T.GAMMA, T.SEED)
    assert mod is None or float(mod0[0, 0]) == float(mod[0, 0])
    with torch.no_grad():
        m.entity_embedding.copy_(torch.from_numpy(ent.copy()))
        m.relation_embedding.copy_(torch.from_numpy(rel.copy()))
    if not case.aligned:
        m.entity_embedding.data = unaligned(m.entity_embedding.data)
    assert (m.entity_embedding.data_ptr() % 16 == 0) == case.aligned
    return m, q, FilterIndex(T.true_triples(case), case.E, len(q))


def check_ref(case, mode, ranks, ties, what):
    r_rank, r_ties = T.reference(case, mode)
    bad = np.nonzero((ranks != r_rank) | (ties != r_ties))[0]
    assert not len(bad), (f"{what}: queries {bad[:8]} (p = {T.ladder(case)[bad[:8]]}): ranks {ranks[bad[:8]]} vs "
                          f"{r_rank[bad[:8]]}, ties {ties[bad[:8]]} vs {r_ties[bad[:8]]}")


def check_crossed(listed, what):
    assert (listed == T.CAP).any(), what
    assert (listed == T.CAP + 1).any(), what
    assert (listed <= T.CAP).sum() >= 12, what
    assert (listed > T.CAP + 1).any(), what


@pytest.mark.parametrize("case", T.CASES, ids=[c.id for c in T.CASES])
def test_paths_vs_reference(case):
    m, q, index = make(case)
    p = T.ladder(case)
    for mode in T.MODES:
        for path in case.paths:
            what = f"{case.id} {mode} {path}"
            ranks, ties, listed = m.rank_queries(q, index, mode, path=path, listed=True)
            x = listed.astype(np.int64) - p
            print(f"{what}: listed − p_j in [{x.min()}, {x.max()}]")
            SEEN.append((case.id, path, mode, int(x.min()), int(x.max()), int((listed > T.CAP).sum())))
            # every unfiltered plant and the last row are exact ties in the fast pass too
            assert x.min() >= 1 and x.max() <= case.n_other, what
            check_crossed(listed, what)
            check_ref(case, mode, ranks, ties, what)
    if not case.aligned:  # the table's alignment forced the wave scan
        for path in ("mfma", "mfma32", "tile"):
            with pytest.raises(_lib.KGEHipError, match="status 4"):
                m.rank_queries(q, index, "tail-batch", path=path)
        ops.raise_on_device_error(DEV)


@pytest.mark.parametrize("ftab", ["1", "0"])
@pytest.mark.parametrize("case", T.BOTH_CASES, ids=[c.id for c in T.BOTH_CASES])
def test_both_directions_vs_reference(case, ftab, monkeypatch):
    """rank_queries_both: k_rank_window, k_rank_refine and k_rank_exact in
    their BOTH_DIRS form, overflowed and listed queries in both halves of the
    grid; the filter as the device table and as per-query lists."""
    monkeypatch.setenv("KGE_RANK_FILTER_TABLE", ftab)
    m, q, index = make(case)
    for path in case.paths:
        out = m.rank_queries_both(q, index, path=path)
        if ftab == "1":
            assert index.device_table("head-batch", DEV) is not None
        for mode, (ranks, ties) in zip(T.MODES, out):
            check_ref(case, mode, ranks, ties, f"{case.id} both/{mode} {path} table={ftab}")


def _counting_sin(monkeypatch):
    calls, real = [], torch.sin

    def sin(x, *a, **k):
        calls.append(int(x.numel()))
        return real(x, *a, **k)

    monkeypatch.setattr(torch, "sin", sin)
    return calls, lambda: monkeypatch.setattr(torch, "sin", real)


def _protate_reference_mode(case, m, q, index, mode, monkeypatch):
    """One library-sin ranking with the host sin's elements counted: a query
    with 1 <= listed <= 1024 undecided candidates delivers 1 + listed items of
    K elements (none when nothing is listed: the device's counts are final),
    one past the cap none — it is ranked on the device and reported."""
    calls, restore = _counting_sin(monkeypatch)
    m.rank_trig = "reference"
    ops.device_sin_queries(DEV)  # reset
    ranks, ties, listed = m.rank_queries(q, index, mode, listed=True)
    restore()
    l64 = listed.astype(np.int64)
    assert sum(calls) == case.d * int((1 + l64[(l64 >= 1) & (l64 <= T.CAP)]).sum()), (case.id, mode)
    assert ops.device_sin_queries(DEV) == int((l64 > T.CAP).sum())
    return ranks, ties, l64


@pytest.mark.parametrize("mode", T.MODES)
def test_protate_plants(mode, monkeypatch):
    """pRotatE d = 32, plants and background only.  The background rows are
    far outside the one-ulp sin intervals, the exact copies (the plants and
    the last row) are never decided: after the list stage a query lists
    exactly its n_j = p_j + 1 copies (n_j <= 1024: from the screen in
    k_rank_refine, or from k_rank_exact_iv when the raw window had overflowed)
    or keeps its overflow mark."""
    case = T.PROTATE_PLANTS
    m, q, index = make(case)
    p = T.ladder(case)
    n = p + 1
    ranks, ties, listed = _protate_reference_mode(case, m, q, index, mode, monkeypatch)
    print(f"{case.id} {mode} reference: listed − p_j in [{(listed - p).min()}, {(listed - p).max()}]")
    assert np.array_equal(listed[n <= T.CAP], n[n <= T.CAP]) and (listed[n > T.CAP] > T.CAP).all()
    assert (listed == T.CAP).any() and (listed < T.CAP).sum() >= 12 and (n == T.CAP + 1).any()
    check_ref(case, mode, ranks, ties, f"{case.id} {mode} reference")
    m.rank_trig = "device"
    ranks, ties, listed = m.rank_queries(q, index, mode, listed=True)
    x = listed.astype(np.int64) - p
    print(f"{case.id} {mode} device: listed − p_j in [{x.min()}, {x.max()}]")
    SEEN.append((case.id, "auto/device", mode, int(x.min()), int(x.max()), int((listed > T.CAP).sum())))
    assert x.min() >= 1 and x.max() <= case.n_other
    check_crossed(listed, f"{case.id} {mode} device")
    check_ref(case, mode, ranks, ties, f"{case.id} {mode} device")


@pytest.mark.parametrize("mode", T.MODES)
def test_protate_shelf(mode, monkeypatch):
    """pRotatE d = 32, plants plus 1100 shelf rows whose float64 score leaves
    the true score by ± T·f, f log-uniform in [0.5, 2], T = 1000 · 2^-24 ·
    |modulus|: wider than the score interval under any one-ulp sin (± 2 floats
    of each of K = 32 |sin| values, for the candidate and the true score:
    < 130 · 2^-24 · |modulus|), narrower than the fast window δ (k_rank_window,
    pRotatE on the register tile: ≈ 4000 · 2^-24 · |modulus| here).  T is the
    first estimate; both regime checks below held with it on an MI355X:
      * rank_trig "device": the raw fast-pass count `listed` is 1100 + n_j for
        every query, n_j = p_j + 1 its exact copies (the unfiltered plants and
        the last row): 1101 … 2200, the whole shelf and no background row —
        every query's window overflows;
      * rank_trig "reference": k_rank_exact_iv rescans each query in the list
        stage and decides every shelf row by its interval (about half of them
        above the true score: the rank is ≈ 551), which leaves the n_j copies.
        n_j <= 1024 fits the list after the rescan (namb <= cap, up to namb ==
        cap): `listed` = n_j (1 … 1024) and the query goes on to the library
        sin.  n_j >= 1025 (namb == cap + 1 and more) is ranked on the device
        and keeps the raw count as its overflow mark (2125 … 2200).  A query
        never reports listed == 1025 here — k_rank_exact_iv rewrites the count
        only when the undecided candidates fit the list — so the cap's far
        side is asserted as n_j == 1025 carrying the overflow mark, being
        counted by ops.device_sin_queries and delivering no item."""
    case = T.PROTATE_SHELF
    m, q, index = make(case)
    p = T.ladder(case)
    m.rank_trig = "device"
    ranks, ties, raw = m.rank_queries(q, index, mode, listed=True)
    print(f"{case.id} {mode} device: listed in [{raw.min()}, {raw.max()}]")
    assert (raw > T.CAP).all()  # the whole shelf is inside the fast window
    assert (raw - p >= case.shelf).all() and (raw - p <= case.n_other).all()
    check_ref(case, mode, ranks, ties, f"{case.id} {mode} device")
    ranks, ties, listed = _protate_reference_mode(case, m, q, index, mode, monkeypatch)
    n = p + 1
    fits = n <= T.CAP
    print(f"{case.id} {mode} reference: listed in [{listed[fits].min()}, {listed[fits].max()}] where n_j <= 1024, "
          f"[{listed[~fits].min()}, {listed[~fits].max()}] past it")
    # every shelf row decided by the screen, every exact copy left undecided
    assert np.array_equal(listed[fits], n[fits]) and np.array_equal(listed[~fits], raw[~fits])
    assert (listed == T.CAP).any() and (listed < T.CAP).sum() >= 12 and (n == T.CAP + 1).any()
    r_rank, _ = T.reference(case, mode)
    assert (r_rank > case.shelf // 4).all()  # the rescan's own count carries the rank
    check_ref(case, mode, ranks, ties, f"{case.id} {mode} reference")
