"""EntityRowPartition.rank_candidates / the sampled test_step: two ranks (gloo,
both on cuda:0), each scoring the candidates whose rows it owns in place,
against single-process KGEModel.rank_candidates / test_step under
KGE_EVAL_CANDIDATES on the same model.  Ranks, tie counts and the five metrics
must be equal on both ranks — exactly: the shards' integer counts sum to the
one-table rank.  materialize() is patched to raise: the whole table is never
gathered.  Once with exchange "queries" (each rank holds only its shard) and
once with "factors" (each rank scores from its own range of the replica).
"""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import spawn_ranks
from knowledgegraphembedding_amd import KGEModel
from test_partition_gpu import _free_port

pytestmark = pytest.mark.gpu

E, R, D, GAMMA = 301, 7, 20, 12.0
DIMS = {"RotatE": (True, False), "TransE": (False, False)}
NAMES = ("RotatE", "TransE")
C, N_EVAL, SEED = 97, 50, 3


def _model(name):
    torch.manual_seed(0)
    de, dr = DIMS[name]
    return KGEModel(name, E, R, D, GAMMA, de, dr).to("cuda:0")


def _triples():
    g = np.random.default_rng(12)
    true = np.unique(np.stack([g.integers(0, E, 2500), g.integers(0, R, 2500), g.integers(0, E, 2500)], 1)
                     .astype(np.int64), axis=0)
    test = true[g.permutation(len(true))[:70]]
    return [tuple(x) for x in test.tolist()], [tuple(x) for x in true.tolist()]


def _cand(test, mode):
    """[70, C] lists over both halves of the table, with duplicates, padding at either end of some
    rows, one row of padding only and the true id in every third row."""
    g = np.random.default_rng(31 if mode == "head-batch" else 32)
    q = np.asarray(test, dtype=np.int64)
    c = g.integers(0, E, (len(q), C)).astype(np.int64)
    tid = q[:, 0 if mode == "head-batch" else 2]
    c[::3, 5] = tid[::3]
    c[1, :9] = -1
    c[4, -20:] = -1
    c[7, :] = -1
    return c


def _args():
    return Namespace(countries=False, nentity=E, nrelation=R, test_batch_size=16, cpu_num=2, test_log_steps=10 ** 9,
                     cuda=True)


def _boom(self):
    raise AssertionError("materialize() called: the sharded evaluation must not gather the table")


def _worker(rank, world, port, exchange, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.pop("KGE_EVAL_CANDIDATES", None)
    os.environ["KGE_EVAL_SEED"] = str(SEED)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from knowledgegraphembedding_amd.partition import EntityRowPartition
    EntityRowPartition.materialize = _boom
    test, true = _triples()
    res = {}
    for name in NAMES:
        model = _model(name)
        part = EntityRowPartition(model, dist.group.WORLD, exchange=exchange)
        assert (part.e0, part.e1) == ((0, 151), (151, 301))[rank]
        if exchange == "queries":
            assert model.entity_embedding.shape[0] == 0  # only the shard is held
        part.RANK_BLOCK = 32  # several blocks of queries, the last one partial
        os.environ["KGE_EVAL_SHARD_CANDIDATES"] = str(N_EVAL)
        metrics = part.test_step(model, test, true, _args())
        os.environ["KGE_EVAL_SHARD_CANDIDATES"] = str(E)  # as many candidates as entities: refused before any launch
        try:
            part.test_step(model, test, true, _args())
            refused = False
        except ValueError:
            refused = True
        del os.environ["KGE_EVAL_SHARD_CANDIDATES"]
        res[name] = {"metrics": metrics, "refused": refused,
                     "ranks": {m: part.rank_candidates(model, test, _cand(test, m), m)
                               for m in ("head-batch", "tail-batch")},
                     # a tensor on the device for the lists
                     "tensor": part.rank_candidates(model, test, torch.from_numpy(_cand(test, "tail-batch")).cuda(),
                                                    "tail-batch")}
    torch.cuda.synchronize()
    out[rank] = res
    dist.destroy_process_group()


@pytest.mark.parametrize("exchange", ["queries", "factors"])
def test_sharded_candidates_two_ranks(exchange, monkeypatch):
    world = 2
    out = mp.Manager().dict()
    spawn_ranks(_worker, (world, _free_port(), exchange, out), world)
    test, true = _triples()
    monkeypatch.setenv("KGE_EVAL_CANDIDATES", str(N_EVAL))
    monkeypatch.setenv("KGE_EVAL_SEED", str(SEED))
    monkeypatch.delenv("KGE_EVAL_RELATIONS", raising=False)
    for name in NAMES:
        model = _model(name)
        metrics = KGEModel.test_step(model, test, true, _args())
        assert set(metrics) == {"MRR", "MR", "HITS@1", "HITS@3", "HITS@10"} and metrics["MR"] <= N_EVAL + 1
        for rank in range(world):
            got = out[rank][name]
            assert got["metrics"] == metrics, (name, rank)
            assert got["refused"], (name, rank)
            for mode in ("head-batch", "tail-batch"):
                ranks, ties = model.rank_candidates(test, _cand(test, mode), mode)
                assert ranks[7] == 1 and ties[7] == 0  # the list of padding only
                assert ties[::3].min() >= 1            # the listed true id is a tie
                assert got["ranks"][mode][0].dtype == np.int64 and got["ranks"][mode][1].dtype == np.int32
                assert np.array_equal(got["ranks"][mode][0], ranks), (name, rank, mode)
                assert np.array_equal(got["ranks"][mode][1], ties), (name, rank, mode)
            assert np.array_equal(got["tensor"][0], got["ranks"]["tail-batch"][0])
            assert np.array_equal(got["tensor"][1], got["ranks"]["tail-batch"][1])
