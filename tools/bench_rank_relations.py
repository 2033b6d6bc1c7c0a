#!/usr/bin/env python
"""Timing of relation prediction (ops.rank_relations) against the path users
had before it: KGEModel.forward(mode='single') over the same nq·R triples
(h, r', t) — ops.score in chunks of whole queries — plus the torch comparison
of every [chunk, R] score block with its true relation's column.

Shape: synthetic, FB15k-like — E = 14,951, R = 1,345, nq = 8,192 queries;
RotatE d = 1000 (-de), DistMult d = 2000, TransE d = 1000.  The tables are the
models' own random initialisation; no dataset is read.  The forward path's
triples are built once, outside the timed region (its users would build them
per call).  The two paths run in alternating windows of `--reps` calls in one
process, after a warm-up call of each; a window's time is the median of its
calls, a path's time the median of its windows, and the spread the fastest and
slowest window.  Reported per model: ms per call of both paths, scored triples
per second, and the number of queries whose (rank, ties) differ between the
paths — reported, not asserted: the forward path's scores are the fast score
kernel's (held to 1e-4, not to the reference's bits).

    python tools/bench_rank_relations.py [--windows 5] [--reps 3] [--jsonl out.jsonl]
    python tools/bench_rank_relations.py --only-new --shapes RotatE --windows 1   # under a kernel profiler
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

E, R, NQ = 14951, 1345, 8192
SHAPES = [
    # name, double entity, double relation, d, gamma
    ("RotatE", True, False, 1000, 24.0),
    ("DistMult", False, False, 2000, 24.0),
    ("TransE", False, False, 1000, 24.0),
    ("pRotatE", False, False, 1000, 24.0),
]
DEFAULT_SHAPES = "RotatE,DistMult,TransE"
CHUNK_TRIPLES = 1 << 20  # the forward path's triples per ops.score call (whole queries)


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
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="comma-separated model names")
    ap.add_argument("--only-new", action="store_true", help="time ops.rank_relations alone (kernel profiling)")
    ap.add_argument("--nentity", type=int, default=E)
    ap.add_argument("--nrelation", type=int, default=R)
    ap.add_argument("--nq", type=int, default=NQ)
    ap.add_argument("--dim", type=int, default=None, help="hidden dimension of every chosen model (default: its own)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    nE, nR, nq = a.nentity, a.nrelation, a.nq
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    out = open(a.jsonl, "a") if a.jsonl else None
    for name, de, dr, d, gamma in SHAPES:
        if name not in a.shapes.split(","):
            continue
        d = a.dim or d
        m = KGEModel(name, nE, nR, d, gamma, de, dr).to(dev)
        desc = m.desc()
        q = torch.stack([torch.randint(0, nE, (nq,), device=dev, generator=g),
                         torch.randint(0, nR, (nq,), device=dev, generator=g),
                         torch.randint(0, nE, (nq,), device=dev, generator=g)], 1).contiguous()
        trig = m._rank_rotation(dev)
        per = max(1, min(nq, CHUNK_TRIPLES // nR))  # queries per forward chunk
        chunks = []
        if not a.only_new:
            rr = torch.arange(nR, device=dev)
            for c0 in range(0, nq, per):
                qc = q[c0:c0 + per]
                tr = torch.stack([qc[:, :1].expand(-1, nR), rr[None, :].expand(len(qc), -1),
                                  qc[:, 2:].expand(-1, nR)], 2).reshape(-1, 3).contiguous()
                chunks.append((tr, qc[:, 1:2]))
        res = {}

        def new():
            res["new"] = ops.rank_relations(desc, q, dev, relation_trig=trig)

        def forward():
            ranks, ties = [], []
            for tr, rc in chunks:
                s = ops.score(desc, "single", tr, None, dev).view(-1, nR)
                st = s.gather(1, rc)
                ranks.append(1 + (s > st).sum(1))
                ties.append((s == st).sum(1) - 1)  # (the true relation's own column)
            res["forward"] = (torch.cat(ranks), torch.cat(ties))

        with torch.no_grad():
            new()
            if not a.only_new:
                forward()
            torch.cuda.synchronize()
            wn, wf = [], []
            for _ in range(a.windows):
                wn.append(window(new, a.reps))
                if not a.only_new:
                    wf.append(window(forward, a.reps))
            ops.raise_on_device_error(dev)
        ms = float(np.median(wn))
        row = dict(model=name, d=d, entity_dim=int(m.entity_dim), E=nE, R=nR, nq=nq, windows=a.windows, reps=a.reps,
                   new_ms=ms, new_ms_min=min(wn), new_ms_max=max(wn), new_triples_per_s=nq * nR / (ms * 1e-3))
        if wf:
            fms = float(np.median(wf))
            differ = int(((res["new"][0] != res["forward"][0]) | (res["new"][1] != res["forward"][1])).sum())
            row.update(forward_ms=fms, forward_ms_min=min(wf), forward_ms_max=max(wf),
                       forward_triples_per_s=nq * nR / (fms * 1e-3), forward_chunk_queries=per,
                       new_over_forward=ms / fms, queries_differing_from_forward=differ)
        print(json.dumps(row), flush=True)
        if out:
            out.write(json.dumps(row) + "\n")
            out.flush()
        del m, q, chunks
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
