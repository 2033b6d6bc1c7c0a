#!/usr/bin/env python
"""Timing of ranking against per-query candidate lists (ops.rank_candidates)
against the path users had before it: KGEModel.forward over the same
candidates — ops.score in query chunks whose [chunk, C] score block fits —
plus the torch comparison with the 'single' score of the true triple.

Shape: synthetic, ogbl-wikikg2-like — E = 2,500,000, R = 535, RotatE d = 250
(-de), TransE d = 500, DistMult d = 500 (rows of 500 floats, a 5 GB table),
nq = 65,536 queries with C = 500 uniformly drawn candidates each, both modes.
The two paths run in alternating windows of `--reps` calls in one process,
after a warm-up call of each; a window's time is the median of its calls, a
path's time the median of its windows, and the spread the fastest and slowest
window.  Reported per (model, mode): ms per call, candidate rows per second,
and the algorithmic gather rate nq·C·entity_dim·4 bytes / time as a share of
`--gather-tbps` — the measured chip-wide rate of random whole rows gathered
from a buffer far larger than the Infinity Cache (5.5-5.8 TB/s for 1-2 KB
rows; the table here is 5 GB).  The forward path's ranks use the fast path's
arithmetic (held to 1e-4, not to the reference's bits): the number of queries
whose (rank, ties) differ from the new call's is reported, not asserted.

    python tools/bench_rank_candidates.py [--windows 5] [--reps 3] [--jsonl out.jsonl]
    python tools/bench_rank_candidates.py --only-new --shapes RotatE --windows 1   # under a kernel profiler
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
SHAPES = [
    # name, double entity, double relation, d, gamma
    ("RotatE", True, False, 250, 12.0),
    ("TransE", False, False, 500, 12.0),
    ("DistMult", False, False, 500, 12.0),
]
CHUNK_BYTES = 16 << 20  # the forward path's [chunk, C] fp32 score block


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
    ap.add_argument("--only-new", action="store_true", help="time ops.rank_candidates alone (kernel profiling)")
    ap.add_argument("--nentity", type=int, default=E)
    ap.add_argument("--nq", type=int, default=NQ)
    ap.add_argument("--ncand", type=int, default=C)
    ap.add_argument("--gather-tbps", type=float, default=5.6)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    nE, nq, nc = a.nentity, a.nq, a.ncand
    g = torch.Generator(device=dev)
    g.manual_seed(11)
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
        chunk = max(1, min(nq, CHUNK_BYTES // (4 * nc)))
        for mode in ("head-batch", "tail-batch"):
            res = {}

            def new():
                res["new"] = ops.rank_candidates(desc, mode, q, cand, dev, relation_trig=trig)

            def forward():
                ranks, ties = [], []
                for c0 in range(0, nq, chunk):
                    pos = q[c0:c0 + chunk]
                    s = ops.score(desc, mode, pos, cand[c0:c0 + chunk], dev)
                    st = ops.score(desc, "single", pos, None, dev)
                    ranks.append(1 + (s > st).sum(1))
                    ties.append((s == st).sum(1))
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
            gather_bytes = nq * nc * le * 4
            ms = float(np.median(wn))
            row = dict(model=name, d=d, entity_dim=le, E=nE, R=R, nq=nq, C=nc, mode=mode, windows=a.windows,
                       reps=a.reps, new_ms=ms, new_ms_min=min(wn), new_ms_max=max(wn),
                       new_rows_per_s=nq * nc / (ms * 1e-3), new_gather_tb_per_s=gather_bytes / (ms * 1e-3) / 1e12,
                       new_share_of_gather_rate=gather_bytes / (ms * 1e-3) / 1e12 / a.gather_tbps,
                       gather_tbps_ref=a.gather_tbps)
            if wf:
                fms = float(np.median(wf))
                differ = int(((res["new"][0] != res["forward"][0]) | (res["new"][1] != res["forward"][1])).sum())
                row.update(forward_ms=fms, forward_ms_min=min(wf), forward_ms_max=max(wf),
                           forward_rows_per_s=nq * nc / (fms * 1e-3), forward_chunk=chunk,
                           new_over_forward=ms / fms, queries_differing_from_forward=differ)
            print(json.dumps(row), flush=True)
            if out:
                out.write(json.dumps(row) + "\n")
                out.flush()
        del m, cand, q
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
