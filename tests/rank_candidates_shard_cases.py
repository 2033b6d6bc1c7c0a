"""Shared inputs of the sharded candidate-list ranking tests
(test_rank_candidates_shard_ref.py on the CPU; test_rank_candidates_shard_gpu.py
and test_rank_candidates_shard_arena_gpu.py on the device).

Cases (K.ALL_CASES and one more, OWN), tables, queries, candidate lists and the
oracle's reference-order scores are rank_candidates_cases' (K); the row splits ("worlds" w1..w4) are
rank_shard_cases.splits(E): one shard, two halves, three uneven ones with a
one-row shard and an empty shard, and EntityRowPartition's own split at four.

Expected counts of the shard [b, e), from K.scores (column 0 is the true score
s_true) and K.cand:
    counts[0][q] = #{j : b <= cand[q, j] < e, s[q, 1 + j] > s_true[q]}
    counts[1][q] = the same with ==
Padding (-1) lies in no shard.  Nothing else is left out: a copy of the true id
counts as a tie in the shard that owns it.  Summed over a world's shards the
counts are K.reference's (rank - 1, ties).
"""
import numpy as np

import rank_candidates_cases as K
import rank_shard_cases as S

MODES = K.MODES
WORLDS = ("w1", "w2", "w3", "w4")
# one case of this file's own: in w3 = ([0, 1), [1, 1), [1, E)) a query's true row and its fixed
# side's row lie on different ranks only if one of them is row 0, which none of K's 24-query cases
# has for a query that lists its true id; this seed has two (test_rank_candidates_shard_ref.py)
OWN = (K.Case("ComplEx", 20, nq=150, C=33, seed=8),)
ALL_CASES = K.ALL_CASES + OWN
CHUNK_MAX = 1024  # list places per chunk at most (kge_internal.h CAND_SHARD_CPC_MAX)


def splits(case, world):
    return S.splits(case.E)[world]


def owned(case, mode, b, e, cand=None):
    """[nq, C] bool: the list places whose id lies in [b, e)."""
    c = K.cand(case, mode) if cand is None else cand
    return (c >= b) & (c < e)


def shard_counts(case, mode, b, e, cand=None):
    """[2, nq] int64: the oracle's counts of the shard [b, e) (cand: the lists, if not the case's —
    ids in the same places as the case's or turned invalid)."""
    s = K.scores(case, mode)
    own = owned(case, mode, b, e, cand)
    st = s[:, :1]
    return np.stack([(own & (s[:, 1:] > st)).sum(1), (own & (s[:, 1:] == st)).sum(1)]).astype(np.int64)


def owner(case, world, ids):
    """index of the shard of `world` that owns each id of `ids`"""
    out = np.full(np.shape(ids), -1, dtype=np.int64)
    for i, (b, e) in enumerate(splits(case, world)):
        out[(np.asarray(ids) >= b) & (np.asarray(ids) < e)] = i
    return out
