"""Row splits of topk_cases' table (E = 1003) for the sharded top-k tests, and
the numpy model of the protocol they share: per-shard k-lists in (score
descending, id ascending) with the documented padding, merged in the same order.

No boundary but 0 is a multiple of 64; at w8 every shard has fewer than 128
rows, so k = 128 pads every list; the tie rows (3, 5, 64, 700, 1002) fall in
shards 0, 0, 0, 5, 7 of w8 and 0, 1 of w2, so the id-ascending rule is decided
across ranks.
"""
import numpy as np

import topk_cases as T

PAD_ID = 0x7FFFFFFF  # an unused place of a shard's list: score -inf, id INT32_MAX


def splits(nentity=T.E):
    rows8 = -(-nentity // 8)  # EntityRowPartition's own split: rows = ceil(E / world)
    half = nentity // 2
    return {
        "w1": [(0, nentity)],
        "w2": [(0, half), (half, nentity)],
        "w3": [(0, 1), (1, 1), (1, nentity)],  # a one-row shard, an empty shard and the rest
        "w8": [(min(r * rows8, nentity), min((r + 1) * rows8, nentity)) for r in range(8)],
    }


SPLITS = splits()
assert SPLITS["w2"] == [(0, 501), (501, 1003)] and SPLITS["w8"][0] == (0, 126) and SPLITS["w8"][7] == (882, 1003)
WORLDS = tuple(SPLITS)


def shard_of(e, ranges):
    return next(i for i, (b, en) in enumerate(ranges) if b <= e < en)


def shard_list(s, mask, b, e, k):
    """The k best unexcluded rows of [b, e) per query of the scores s [nq, E]:
    (scores [nq, k], ids [nq, k] int64) sorted by (score descending, id
    ascending), padded with (-inf, PAD_ID).  NaN and -inf scores are never listed."""
    nq = s.shape[0]
    sc = np.full((nq, k), -np.inf, dtype=s.dtype)
    ids = np.full((nq, k), PAD_ID, dtype=np.int64)
    for i in range(nq):
        row = s[i, b:e]
        ok = ~mask[i, b:e] & ~np.isnan(row) & ~np.isneginf(row)
        cand = np.nonzero(ok)[0]
        order = cand[np.argsort(-row[cand], kind="stable")][:k]  # stable: equal scores stay in ascending id
        sc[i, :len(order)] = row[order]
        ids[i, :len(order)] = order + b
    return sc, ids


def merge_lists(lists, k):
    """The ranks' lists [(scores, ids)] merged per query in (score descending,
    id ascending): (ids [nq, k] int64 with -1 for padding, scores [nq, k])."""
    sc = np.concatenate([l[0] for l in lists], axis=1)
    ids = np.concatenate([l[1] for l in lists], axis=1)
    out_i = np.empty((sc.shape[0], k), dtype=np.int64)
    out_s = np.empty((sc.shape[0], k), dtype=sc.dtype)
    for i in range(sc.shape[0]):
        order = np.lexsort((ids[i], -sc[i]))[:k]
        out_i[i], out_s[i] = ids[i, order], sc[i, order]
    out_i[out_i == PAD_ID] = -1
    return out_i, out_s


def whole_topk(s, mask, k):
    """The one-table result in the same form."""
    return merge_lists([shard_list(s, mask, 0, s.shape[1], k)], k)
