#!/usr/bin/env python
"""Timing of top-k link prediction (ops.topk) against the composite it
replaces — ops.score over all entities in query chunks that fit memory, then
torch.topk — in the same process and the same pass loop.

Shapes: FB15k-shape RotatE and TransE (E=14951, R=1345, d=1000) at nq = 8192,
wn18rr-shape DistMult (E=40943, R=11, d=500) at nq = 6268; k = 10 and 128;
filtered with a synthetic index (the composite applies no filter: it is the
cheaper side of the comparison).  Fastest and median of 10 passes, after one
warm-up pass.  For orientation it also times the ranking's counting pass
(path "tile", ranking stage timer, stage 1) for the same model and shape.

    python tools/bench_topk.py [--passes 10] [--json out.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from knowledgegraphembedding_amd import KGEModel, _lib, ops, synth  # noqa: E402
from knowledgegraphembedding_amd.filters import FilterIndex  # noqa: E402

SHAPES = [
    # name, double entity, double relation, d, gamma, E, R, true triples, nq, label
    ("RotatE", True, False, 1000, 24.0, 14951, 1345, 592213, 8192, "FB15k"),
    ("TransE", False, False, 1000, 24.0, 14951, 1345, 592213, 8192, "FB15k"),
    ("DistMult", False, False, 500, 200.0, 40943, 11, 93003, 6268, "wn18rr"),
]
CHUNK_BYTES = 1 << 30  # the composite's [chunk, E] fp32 score block


def timed(dev, fn, passes):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(passes)]
    fn()  # warm-up (workspace growth, first launches)
    torch.cuda.synchronize(dev)
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize(dev)
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return ms[0], float(np.median(ms))


def counting_pass_ms(model, q, index, mode, passes):
    """The ranking's fast counting pass alone (stage 1 of the ranking timer), per direction."""
    lib = _lib.load()
    model.rank_queries(q, index, mode, path="tile")  # warm-up
    _lib.check(lib.kge_stage_timer(4, None, 0), "kge_stage_timer")
    for _ in range(passes):
        model.rank_queries(q, index, mode, path="tile")
    out = np.zeros(4, dtype=np.float32)
    _lib.check(lib.kge_stage_timer(5, out.ctypes.data_as(ctypes.c_void_p), 4), "kge_stage_timer")
    lib.kge_stage_timer(0, None, 0)
    return float(out[1] / max(out[3], 1))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--shapes", default=None, help="comma-separated model names (default: all)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows = []
    for name, de, dr, d, gamma, E, R, ntrue, nq, label in SHAPES:
        if a.shapes and name not in a.shapes.split(","):
            continue
        m = KGEModel(name, E, R, d, gamma, de, dr).to(dev)
        true, _, _ = synth.kge_batch(7, ntrue, 1, E, R)
        index = FilterIndex(true, E, R)
        mode = "tail-batch"
        q = true[:nq].copy()
        qd = torch.from_numpy(q).to(dev)
        tab = index.device_table(mode, dev)
        if tab is None:
            off, ids = index.filter_csr(np.where(np.arange(3) == 2, -1, q), mode)
            filt, table = (torch.from_numpy(off).to(dev), torch.from_numpy(ids).to(dev)), False
        else:
            filt, table = tab, True
        desc = m.desc()
        allent = torch.arange(E, dtype=torch.int64, device=dev)
        chunk = max(1, min(nq, CHUNK_BYTES // (4 * E)))

        # the candidate ids of a chunk, built once (not part of the composite's time)
        negs = {n: allent.unsqueeze(0).expand(n, E).contiguous() for n in {min(chunk, nq - c0)
                                                                           for c0 in range(0, nq, chunk)}}

        def composite(k):
            outs = []
            for c0 in range(0, nq, chunk):
                pos = qd[c0:c0 + chunk]
                outs.append(torch.topk(ops.score(desc, mode, pos, negs[len(pos)], dev), k, dim=1))
            return outs

        with torch.no_grad():
            count_ms = counting_pass_ms(m, q, index, mode, 3)
            for k in (10, 128):
                new = timed(dev, lambda: ops.topk(desc, mode, qd, k, dev, filt=filt, filter_table=table), a.passes)
                base = timed(dev, lambda: composite(k), a.passes)
                ops.raise_on_device_error(dev)
                row = dict(model=name, shape=label, E=E, nq=nq, k=k, topk_ms_fastest=new[0], topk_ms_median=new[1],
                           composite_ms_fastest=base[0], composite_ms_median=base[1],
                           counting_pass_ms=count_ms, topk_over_counting=new[1] / count_ms if count_ms else None)
                rows.append(row)
                print(json.dumps(row), flush=True)
        del m, index
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
