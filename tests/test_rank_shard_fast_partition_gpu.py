"""EntityRowPartition.rank_queries through the fast counting pass
(kge_rank_shard_fast, the default) and through the exact stage
(KGE_EVAL_SHARD_FAST=0): two ranks (gloo, both on cuda:0), each ranking its own
half of the entity rows in place.  Both give identical ranks and tie counts on
both ranks, equal to single-process KGEModel.rank_queries on the same model —
exactly: the shards' integer counts sum to the one-table rank.  One distance
model (RotatE, the register tile) and one bilinear model (DistMult, the
split-bf16 tile); the worker checks which entry ran and which path it took.
"""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import spawn_ranks
from test_partition_gpu import _free_port
from test_rank_shard_partition_gpu import DIMS, NAMES, _boom, _model, _triples

pytestmark = pytest.mark.gpu
MODES = ("head-batch", "tail-batch")
WANT_PATH = {"RotatE": 2, "DistMult": 1}


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from knowledgegraphembedding_amd import ops
    from knowledgegraphembedding_amd.partition import EntityRowPartition
    EntityRowPartition.materialize = _boom
    calls = {"fast": 0, "exact": 0}
    fast, exact = ops.rank_shard_count_fast, ops.rank_shard_count

    def count_fast(*a, **k):
        calls["fast"] += 1
        return fast(*a, **k)

    def count_exact(*a, **k):
        calls["exact"] += 1
        return exact(*a, **k)

    ops.rank_shard_count_fast, ops.rank_shard_count = count_fast, count_exact
    test, true = _triples()
    res = {}
    for name in NAMES:
        model = _model(name)
        part = EntityRowPartition(model, dist.group.WORLD, exchange="queries")
        part.RANK_BLOCK = 32  # several blocks of queries, the last one partial
        desc, own = part._own_desc(model)
        res[name] = {"path": ops.rank_shard_fast_path(desc, own)}
        for key, env in (("fast", None), ("exact", "0"), ("on", "1")):
            if env is None:
                os.environ.pop("KGE_EVAL_SHARD_FAST", None)
            else:
                os.environ["KGE_EVAL_SHARD_FAST"] = env
            before = dict(calls)
            res[name][key] = {m: part.rank_queries(model, test, true, m) for m in MODES}
            res[name][key + "_calls"] = {k: calls[k] - before[k] for k in calls}
    os.environ.pop("KGE_EVAL_SHARD_FAST", None)
    torch.cuda.synchronize()
    out[rank] = res
    dist.destroy_process_group()


def test_fast_and_exact_evaluation_two_ranks():
    assert set(NAMES) == set(WANT_PATH) == set(DIMS)
    world = 2
    out = mp.Manager().dict()
    spawn_ranks(_worker, (world, _free_port(), out), world)
    test, true = _triples()
    blocks = 2 * -(-len(test) // 32)  # per key: both modes
    for name in NAMES:
        model = _model(name)
        want = {m: model.rank_queries(test, true, m) for m in MODES}
        for rank in range(world):
            got = out[rank][name]
            assert got["path"] == WANT_PATH[name], (name, rank)  # no silent fallback to the exact kernel
            assert got["fast_calls"] == {"fast": blocks, "exact": 0}, (name, rank)
            assert got["exact_calls"] == {"fast": 0, "exact": blocks}, (name, rank)
            assert got["on_calls"] == {"fast": blocks, "exact": 0}, (name, rank)
            for mode in MODES:
                ranks, ties = want[mode]
                for key in ("fast", "exact", "on"):
                    r, t = got[key][mode]
                    assert r.dtype == np.int64 and t.dtype == np.int32
                    assert np.array_equal(r, ranks), (name, rank, mode, key)
                    assert np.array_equal(t, ties), (name, rank, mode, key)
