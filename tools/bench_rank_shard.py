#!/usr/bin/env python
"""Timing of the sharded filtered ranking's counting stage (ops.rank_shard_count,
kge_rank_shard stage COUNT) against what users have today for the same queries:
ops.rank_filtered_both over the whole table on one GPU.

Shape: synthetic, YAGO3-10-like — E = 123,182, R = 37, RotatE d = 500 (-de: rows
of 1000 floats), 10,000 test triples ranked in both directions, the filter the
whole index of 1,000,000 random true triples plus the test triples.  One process
on one GPU times, per evaluation (head-batch + tail-batch):
  (a) stage COUNT on the shard of rank 3 of world 8 — EntityRowPartition's split,
      rows [46194, 61592): 15,398 rows — as shipped (one query per workgroup), and
      (a2, a4) with KGE_RANK_SHARD_QPW = 2 and 4 queries per staged row;
  (b) stage COUNT at world 1, rows [0, E);
  (c) ops.rank_filtered_both on the whole table;
  (f) the fast counting pass (ops.rank_shard_count_fast, kge_rank_shard_fast) on
      the shard of (a), and (g) at world 1 — the same tiles as (c), s_true given.
fixed_rows and s_true come from stages ROWS and TRUE at world 1, run once before
the timing (they cost the same at any world and are reported as rows_true_ms).
The paths alternate in `--windows` windows of `--reps` calls after a warm-up call
of each; a window's time is the median of its calls, a path's time the median of
its windows, and the spread the fastest and slowest window.  The number of
queries whose (b) counts differ from (c)'s ranks and ties is reported, not
asserted (it is 0 when both are the reference's bits).  (g)'s counts of all
2 x nq queries are asserted equal to (b)'s, and (f)'s to (a)'s.

    python tools/bench_rank_shard.py [--windows 5] [--reps 3] [--jsonl profiles/rank_shard_bench.jsonl]
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

E, R, D, GAMMA, NQ, NTRUE = 123182, 37, 500, 24.0, 10000, 1_000_000
WORLD, RANK = 8, 3
MODES = ("head-batch", "tail-batch")


def window(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--jsonl", default=None)
    ap.add_argument("--model", default="RotatE")
    ap.add_argument("--nq", type=int, default=NQ)
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
    q_host = torch.from_numpy(true[:nq].copy())
    q = q_host.to(dev)
    index = FilterIndex(true, E, R, device=dev)
    tabs = {mode: index.device_table(mode, dev) for mode in MODES}
    trig = m._rank_rotation(dev)
    rows = -(-E // WORLD)
    shard = (RANK * rows, min(E, (RANK + 1) * rows))
    whole = (0, E)
    fixed = {mode: torch.empty(nq, le, device=dev) for mode in MODES}
    s_true = {mode: torch.empty(nq, device=dev) for mode in MODES}
    counts = {mode: torch.empty(2, nq, dtype=torch.int64, device=dev) for mode in MODES}
    res = {}

    def rows_true():
        for mode in MODES:
            ops.rank_shard_rows(desc, mode, q, whole, dev, fixed[mode])
            ops.rank_shard_true(desc, mode, q, whole, dev, fixed[mode], s_true[mode], relation_trig=trig)

    def count(own, qpw=1):
        os.environ["KGE_RANK_SHARD_QPW"] = str(qpw)  # (read per call) queries per workgroup
        for mode in MODES:
            ops.rank_shard_count(desc, mode, q, own, dev, fixed[mode], s_true[mode], tabs[mode], counts[mode],
                                 filter_table=True, relation_trig=trig)

    fcounts = {mode: torch.empty(2, nq, dtype=torch.int64, device=dev) for mode in MODES}
    listed = {mode: torch.empty(nq, dtype=torch.int32, device=dev) for mode in MODES}

    def count_fast(own):
        for mode in MODES:
            ops.rank_shard_count_fast(desc, mode, q, own, dev, fixed[mode], s_true[mode], tabs[mode], fcounts[mode],
                                      filter_table=True, relation_trig=trig, listed=listed[mode])

    def today():
        res["c"] = ops.rank_filtered_both(desc, q, tabs["head-batch"], tabs["tail-batch"], dev, relation_trig=trig,
                                          filter_table=True)

    paths = {"a": lambda: count(shard), "a2": lambda: count(shard, 2), "a4": lambda: count(shard, 4),
             "b": lambda: count(whole), "c": today, "f": lambda: count_fast(shard), "g": lambda: count_fast(whole)}
    with torch.no_grad():
        rows_true()
        for fn in paths.values():
            fn()
        torch.cuda.synchronize()
        rt_ms = window(rows_true, a.reps)
        w = {k: [] for k in paths}
        for _ in range(a.windows):
            for k, fn in paths.items():
                w[k].append(window(fn, a.reps))
        count(whole)
        got = torch.cat([counts[mode] for mode in MODES], 1)  # [2, 2·nq]: head-batch then tail-batch
        differ = int(((got[0] + 1 != res["c"][0]) | (got[1] != res["c"][1].long())).sum())
        # the fast entry's counts are the exact stage's, at world 1 and on the shard: all 2·nq queries
        count_fast(whole)
        fgot = torch.cat([fcounts[mode] for mode in MODES], 1)
        assert fgot.shape == got.shape == (2, 2 * nq) and torch.equal(fgot, got), "fast entry != exact stage at world 1"
        listed_w1 = float(torch.cat([listed[mode] for mode in MODES]).float().mean())
        count(shard)
        count_fast(shard)
        for mode in MODES:
            assert torch.equal(fcounts[mode], counts[mode]), f"fast entry != exact stage on the shard, {mode}"
        listed_shard = float(torch.cat([listed[mode] for mode in MODES]).float().mean())
        fast_path = {"shard": ops.rank_shard_fast_path(desc, shard, relation_trig=trig),
                     "world1": ops.rank_shard_fast_path(desc, whole, relation_trig=trig)}
        ops.raise_on_device_error(dev)
    ms = {k: float(np.median(v)) for k, v in w.items()}
    row = dict(model=a.model, d=D, entity_dim=le, E=E, R=R, nq=nq, directions=2, world=WORLD, rank=RANK,
               shard_rows=shard[1] - shard[0], windows=a.windows, reps=a.reps, rows_true_ms=rt_ms,
               queries_differing_b_vs_c=differ, fast_path=fast_path, fast_counts_equal_exact=2 * nq,
               fast_listed_per_query_shard=listed_shard, fast_listed_per_query_world1=listed_w1)
    for k, what in (("a", "count_shard"), ("a2", "count_shard_2_queries_per_workgroup"),
                    ("a4", "count_shard_4_queries_per_workgroup"), ("b", "count_world1"),
                    ("c", "rank_filtered_both"), ("f", "count_fast_shard"), ("g", "count_fast_world1")):
        row.update({f"{k}_{what}_ms": ms[k], f"{k}_ms_min": min(w[k]), f"{k}_ms_max": max(w[k])})
    scanned = 2 * nq * (shard[1] - shard[0]) * le * 4
    # the fast entry against the rows of the same run; a ratio's spread: slowest / fastest and fastest / slowest windows
    for name, x, y in (("a_over_f", "a", "f"), ("b_over_g", "b", "g"), ("g_over_c", "g", "c")):
        row.update({name: ms[x] / ms[y], name + "_min": min(w[x]) / max(w[y]), name + "_max": max(w[x]) / min(w[y])})
    row.update(a_over_c=ms["a"] / ms["c"], b_over_c=ms["b"] / ms["c"], b_over_a=ms["b"] / ms["a"],
               a_l2_read_tb=scanned / 1e12, a_l2_tb_per_s=scanned / (ms["a"] * 1e-3) / 1e12)
    print(json.dumps(row), flush=True)
    if a.jsonl:
        with open(a.jsonl, "a") as out:
            out.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
