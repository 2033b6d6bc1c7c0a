#!/usr/bin/env python
"""Timing of the sharded top-k's two stages (ops.topk_shard_list /
ops.topk_shard_merge, kge_topk_shard) against what users have today for the
same queries: ops.topk over the whole table on one GPU.

Shape: synthetic, YAGO3-10-like, as tools/bench_rank_shard.py — E = 123,182,
R = 37, RotatE d = 500 (-de: rows of 1000 floats), 8,192 tail-batch queries, the
filter the whole index of 1,000,000 random true triples plus the queries,
k = 10 and k = 128.  One process on one GPU times, per k:
  (a) stage LIST on the shard of rank 3 of world 8 — EntityRowPartition's split,
      rows [46194, 61592): 15,398 rows;
  (b) stage LIST at world 1, rows [0, E);
  (c) ops.topk on the whole table;
  (m) stage MERGE of the 8 lists of world 8 (each shard's LIST run once before).
fixed_rows comes from stage ROWS at world 1, run once before the timing (it
costs the same at any world and is reported as rows_ms).  The claims under test:
(b) ≈ (c), since both run the same scan kernels over the same rows, and
(a) ≤ (c).  The paths alternate in `--windows` windows of `--reps` calls after a
warm-up call of each; a window's time is the median of its calls, a path's time
the median of its windows, and the spread the fastest and slowest window.
Whether (b) merged at world 1 and the world-8 merge equal (c) bit for bit is
reported, not asserted.

    python tools/bench_topk_shard.py [--windows 5] [--reps 3] [--jsonl profiles/topk_shard_bench.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from knowledgegraphembedding_amd import KGEModel, ops  # noqa: E402
from knowledgegraphembedding_amd.filters import FilterIndex  # noqa: E402

E, R, D, GAMMA, NQ, NTRUE = 123182, 37, 500, 24.0, 8192, 1_000_000
WORLD, RANK = 8, 3
MODE = "tail-batch"
KS = (10, 128)


def window(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def same(a, b):
    return bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--jsonl", default=None)
    ap.add_argument("--model", default="RotatE")
    ap.add_argument("--nq", type=int, default=NQ)
    ap.add_argument("--path", default="auto", choices=sorted(ops.TOPK_PATHS))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    nq = a.nq
    de = a.model in ("RotatE", "ComplEx")
    torch.manual_seed(3)
    m = KGEModel(a.model, E, R, D, GAMMA, de, a.model == "ComplEx").to(dev)
    desc, le = m.desc(), int(m.entity_dim)
    g = np.random.default_rng(11)
    true = np.stack([g.integers(0, E, NTRUE + nq), g.integers(0, R, NTRUE + nq), g.integers(0, E, NTRUE + nq)],
                    1).astype(np.int64)
    q = torch.from_numpy(true[:nq].copy()).to(dev)
    tab = FilterIndex(true, E, R, device=dev).device_table(MODE, dev)
    rows = -(-E // WORLD)
    ranges = [(min(r * rows, E), min((r + 1) * rows, E)) for r in range(WORLD)]
    shard, whole = ranges[RANK], (0, E)
    fixed = torch.empty(nq, le, device=dev)
    out_rows = []
    with torch.no_grad():
        ops.rank_shard_rows(desc, MODE, q, whole, dev, fixed)
        torch.cuda.synchronize()
        rows_ms = window(lambda: ops.rank_shard_rows(desc, MODE, q, whole, dev, fixed), a.reps)
        for k in KS:
            res = {}
            kw = dict(filt=tab, filter_table=True, path=a.path)

            def lst(own, key):
                res[key] = ops.topk_shard_list(desc, MODE, q, own, k, dev, fixed, **kw)

            every = [ops.topk_shard_list(desc, MODE, q, own, k, dev, fixed, **kw) for own in ranges]
            all_s, all_i = torch.stack([x[0] for x in every]), torch.stack([x[1] for x in every])

            def merge():
                res["m"] = ops.topk_shard_merge(desc, MODE, q, k, dev, all_s, all_i)

            def today():
                res["c"] = ops.topk(desc, MODE, q, k, dev, **kw)

            paths = {"a": lambda: lst(shard, "a"), "b": lambda: lst(whole, "b"), "c": today, "m": merge}
            for fn in paths.values():
                fn()
            torch.cuda.synchronize()
            w = {key: [] for key in paths}
            for _ in range(a.windows):
                for key, fn in paths.items():
                    w[key].append(window(fn, a.reps))
            b_merged = ops.topk_shard_merge(desc, MODE, q, k, dev, res["b"][0][None].contiguous(),
                                            res["b"][1][None].contiguous())
            ms = {key: float(np.median(v)) for key, v in w.items()}
            row = dict(model=a.model, d=D, entity_dim=le, E=E, R=R, nq=nq, mode=MODE, k=k, path=a.path, world=WORLD,
                       rank=RANK, shard_rows=shard[1] - shard[0], windows=a.windows, reps=a.reps, rows_ms=rows_ms,
                       world1_equals_topk=same(b_merged, res["c"]), world8_equals_topk=same(res["m"], res["c"]))
            for key, what in (("a", "list_shard"), ("b", "list_world1"), ("c", "topk_whole_table"),
                              ("m", "merge_world8")):
                row.update({f"{key}_{what}_ms": ms[key], f"{key}_ms_min": min(w[key]), f"{key}_ms_max": max(w[key])})
            row.update(a_over_c=ms["a"] / ms["c"], b_over_c=ms["b"] / ms["c"], c_over_a=ms["c"] / ms["a"])
            print(json.dumps(row), flush=True)
            out_rows.append(row)
        ops.raise_on_device_error(dev)
    if a.jsonl:
        with open(a.jsonl, "a") as out:
            for row in out_rows:
                out.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
