#!/usr/bin/env python
"""Timing of the sharded ranking against candidate lists
(ops.rank_candidates_shard_count, kge_rank_candidates_shard) against what users
have today for the same queries and lists: ops.rank_candidates over the whole
table on one GPU.

Shape: tools/bench_rank_candidates.py's, synthetic, ogbl-wikikg2-like —
E = 2,500,000, R = 535, RotatE d = 250 (-de), TransE d = 500, DistMult d = 500
(rows of 500 floats, a 5 GB table), nq = 65,536 queries with C = 500 uniformly
drawn candidates each, both modes.  One process on one GPU times, per (model,
mode):
  (a) the new call on the shard of rank 3 of world 8 — EntityRowPartition's
      split, rows [937500, 1250000): an eighth of every list is owned;
  (b) the new call at world 1, rows [0, E): every candidate is owned, so the
      call scores what (c) scores and pays for the compaction besides;
  (c) ops.rank_candidates on the whole table.
fixed_rows and s_true come from kge_rank_shard's stages ROWS and TRUE at world
1, run once before the timing (they cost the same at any world) and reported,
untimed by the windows, as rows_true_ms.  The paths alternate in `--windows`
windows of `--reps` calls after a warm-up call of each; a window's time is the
median of its calls, a path's time the median of its windows, and the spread
the fastest and slowest window.  Asserted: (b)'s counts equal (c)'s ranks and
ties, and so does the sum of the counts of all eight shards, run once, untimed.
Per path the algorithmic bytes — the ids every rank reads, nq·C·8, plus the
rows it scores × entity_dim·4 — and the rate they were moved at.

    python tools/bench_rank_candidates_shard.py [--windows 5] [--reps 3] [--jsonl profiles/rank_candidates_shard_bench.jsonl]
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

E, R, NQ, C = 2_500_000, 535, 65536, 500
WORLD, RANK = 8, 3
SHAPES = [
    # name, double entity, double relation, d, gamma
    ("DistMult", False, False, 500, 12.0),
    ("RotatE", True, False, 250, 12.0),
    ("TransE", False, False, 500, 12.0),
]


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
    ap.add_argument("--shapes", default=None, help="comma-separated model names (default: all)")
    ap.add_argument("--nentity", type=int, default=E)
    ap.add_argument("--nq", type=int, default=NQ)
    ap.add_argument("--ncand", type=int, default=C)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    nE, nq, nc = a.nentity, a.nq, a.ncand
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    rows = -(-nE // WORLD)
    ranges = [(min(r * rows, nE), min(nE, (r + 1) * rows)) for r in range(WORLD)]
    shard, whole = ranges[RANK], (0, nE)
    out = open(a.jsonl, "a") if a.jsonl else None
    for name, de, dr, d, gamma in SHAPES:
        if a.shapes and name not in a.shapes.split(","):
            continue
        m = KGEModel(name, nE, R, d, gamma, de, dr).to(dev)
        desc = m.desc()
        le = int(m.entity_dim)
        q = torch.stack([torch.randint(0, nE, (nq,), device=dev, generator=g),
                         torch.randint(0, R, (nq,), device=dev, generator=g),
                         torch.randint(0, nE, (nq,), device=dev, generator=g)], 1).contiguous()
        cand = torch.randint(0, nE, (nq, nc), device=dev, generator=g)
        trig = m._rank_rotation(dev)
        fixed = torch.empty(nq, le, device=dev)
        s_true = torch.empty(nq, device=dev)
        counts = torch.empty(2, nq, dtype=torch.int64, device=dev)
        for mode in ("head-batch", "tail-batch"):
            res = {}

            def rows_true():
                ops.rank_shard_rows(desc, mode, q, whole, dev, fixed)
                ops.rank_shard_true(desc, mode, q, whole, dev, fixed, s_true, relation_trig=trig)

            def count(own):
                ops.rank_candidates_shard_count(desc, mode, q, own, dev, fixed, s_true, cand, counts,
                                                relation_trig=trig)

            def today():
                res["c"] = ops.rank_candidates(desc, mode, q, cand, dev, relation_trig=trig)

            paths = {"a": lambda: count(shard), "b": lambda: count(whole), "c": today}
            with torch.no_grad():
                rows_true()
                rows_true()
                torch.cuda.synchronize()
                rt_ms = window(rows_true, 1)
                for fn in paths.values():
                    fn()
                torch.cuda.synchronize()
                w = {k: [] for k in paths}
                for _ in range(a.windows):
                    for k, fn in paths.items():
                        w[k].append(window(fn, a.reps))
                ranks, ties = res["c"][0], res["c"][1].long()
                count(whole)
                assert torch.equal(counts[0] + 1, ranks) and torch.equal(counts[1], ties), \
                    f"{name} {mode}: world 1 counts != ops.rank_candidates"
                tot = torch.zeros_like(counts)
                for own in ranges:
                    count(own)
                    tot += counts
                assert torch.equal(tot[0] + 1, ranks) and torch.equal(tot[1], ties), \
                    f"{name} {mode}: the eight shards' counts do not sum to ops.rank_candidates"
                owned = int(((cand >= shard[0]) & (cand < shard[1])).sum())
                ops.raise_on_device_error(dev)
            ms = {k: float(np.median(v)) for k, v in w.items()}
            row = dict(model=name, d=d, entity_dim=le, E=nE, R=R, nq=nq, C=nc, mode=mode, world=WORLD, rank=RANK,
                       shard_rows=shard[1] - shard[0], owned_candidates=owned, windows=a.windows, reps=a.reps,
                       rows_true_ms=rt_ms, world1_counts_equal_rank_candidates=nq, shards_sum_equal_rank_candidates=nq)
            ids = nq * nc * 8
            scored = {"a": owned, "b": nq * nc, "c": nq * (nc + 1)}  # (c) scores the true row of every chunk too
            for k, what in (("a", "shard"), ("b", "world1"), ("c", "rank_candidates")):
                b = ids + scored[k] * le * 4
                row.update({f"{k}_{what}_ms": ms[k], f"{k}_ms_min": min(w[k]), f"{k}_ms_max": max(w[k]),
                            f"{k}_bytes": b, f"{k}_tb_per_s": b / (ms[k] * 1e-3) / 1e12})
            # a ratio's spread: fastest / slowest and slowest / fastest windows
            for r_, x in (("a_over_c", "a"), ("b_over_c", "b")):
                row.update({r_: ms[x] / ms["c"], r_ + "_min": min(w[x]) / max(w["c"]),
                            r_ + "_max": max(w[x]) / min(w["c"])})
            print(json.dumps(row), flush=True)
            if out:
                out.write(json.dumps(row) + "\n")
                out.flush()
        del m, cand, q, fixed
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
