"""The sharded top-k protocol as a numpy model on topk_cases' float64 scores (no
device): each shard's k-list in (score descending, id ascending) with its
padding, merged in the same order, equals the whole-table top-k for every
split, k and filter — the property the device tests hold kge_topk_shard to bit
for bit — and the inputs cannot pass vacuously: under w2 and w8 a tie group
spans shards.
"""
import numpy as np
import pytest

import topk_cases as T
import topk_shard_cases as TS
from knowledgegraphembedding_amd import _lib

KS = (1, 10, 128)


def test_padding_id_is_the_binding_s():
    assert TS.PAD_ID == _lib.TOPK_PAD_ID == np.iinfo(np.int32).max


@pytest.mark.parametrize("ties", (False, True), ids=("plain", "ties"))
@pytest.mark.parametrize("world", TS.WORLDS)
@pytest.mark.parametrize("name", T.NAMES)
def test_merged_lists_equal_the_whole_table(name, world, ties):
    for mode in T.MODES:
        s = T.s64_of(name, mode, ties=ties)
        for mask in (np.zeros(s.shape, dtype=bool), T.mask_of(mode)):
            for k in KS:
                want = TS.whole_topk(s, mask, k)
                lists = [TS.shard_list(s, mask, b, e, k) for b, e in TS.SPLITS[world]]
                for (sc, ids), (b, e) in zip(lists, TS.SPLITS[world]):
                    real = ids != TS.PAD_ID
                    assert ((ids[real] >= b) & (ids[real] < e)).all()
                    assert np.isneginf(sc[~real]).all() and real.sum(1).max(initial=0) <= e - b
                got = TS.merge_lists(lists, k)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, mode, world, k)
                n = np.minimum(k, (~mask).sum(1))  # padded exactly where candidates run out
                assert ((got[0] >= 0).sum(1) == n).all() and (np.isneginf(got[1]).sum(1) == k - n).all()


def test_w8_pads_every_list_at_k_128():
    assert max(e - b for b, e in TS.SPLITS["w8"]) < 128
    assert not any(b % 64 == 0 for w in TS.WORLDS for b, e in TS.SPLITS[w] if b)
    assert TS.SPLITS["w3"] == [(0, 1), (1, 1), (1, T.E)]


@pytest.mark.parametrize("world", ("w2", "w8"))
def test_a_tie_group_spans_shards(world):
    """The tied rows lie in more than one shard, and some query's merged top-k
    takes tied rows of two shards next to each other: the id-ascending rule is
    decided by the merge, not inside a shard."""
    ranges = TS.SPLITS[world]
    owners = [TS.shard_of(r, ranges) for r in T.TIE_ROWS]
    assert len(set(owners)) > 1
    assert owners == ([0, 0, 0, 5, 7] if world == "w8" else [0, 0, 0, 1, 1])
    s = T.s64_of("TransE", "tail-batch", ties=True)
    ids, sc = TS.whole_topk(s, np.zeros(s.shape, dtype=bool), 128)
    crossing = 0
    for i in range(len(ids)):
        at = np.nonzero(np.isin(ids[i], T.TIE_ROWS))[0]
        if len(at) == 5:
            assert ids[i, at].tolist() == list(T.TIE_ROWS) and len(set(sc[i, at].tolist())) == 1
            crossing += len({TS.shard_of(int(e), ranges) for e in ids[i, at]}) > 1
    assert crossing >= 3
