#!/usr/bin/env python
"""Timing of the fused Adagrad step (KGEAdagrad, kge_train_step_adagrad), element-wise
and row-wise, against the lazy entity Adam (KGELazyAdam, kge_train_step_lazy) in one
process: after a warm-up the three run in alternating windows of --steps fused train
steps each (default 200), --windows times each, on the same pre-built batches
(uniform negatives, the modes alternating).  The two shapes of tools/bench_lazy.py:

  fb15k   RotatE E=14951 R=1345 d=1000 b=1024 n=256 (bench.py's shape);
  2m      RotatE E=2,000,000 R=1345 d=200 b=1024 n=256, a synthetic table.

One JSON line per window is appended to --out (profiles/adagrad_bench.jsonl): the
shape, the optimizer, the window's ms per step, the optimizer state's bytes computed
from the shape (Adam 8·E·Le, Adagrad 4·E·Le, row-wise 4·E) and the table bytes a
touched element moves (24 / 16 / ~8, computed).  Then one summary line per shape
and optimizer: median, spread (max - min over the windows), the entity launch's
time from the stage timer (stage 4, a separate short run: the timer's events cost
time), and whether the element-wise step met the acceptance rule
(ms/step <= lazy Adam's + lazy Adam's own spread).

    python tools/bench_adagrad.py [--shapes fb15k,2m] [--steps 200] [--windows 3] [--out FILE]
"""
from __future__ import annotations

import argparse
import functools
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_lazy import SHAPES, Runner, make_batches, stats  # noqa: E402
from knowledgegraphembedding_amd import KGEAdagrad, KGELazyAdam, ops  # noqa: E402

OPTIMIZERS = {
    # name: (factory, state bytes per (E, Le), table bytes moved per touched element)
    "lazy_adam": (KGELazyAdam, lambda E, Le: 8 * E * Le, 24.0),
    "adagrad": (KGEAdagrad, lambda E, Le: 4 * E * Le, 16.0),
    "adagrad_rowwise": (functools.partial(KGEAdagrad, rowwise_entity=True), lambda E, Le: 4 * E, 8.0),
}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="fb15k,2m")
    ap.add_argument("--steps", type=int, default=200, help="steps per window (>= 200 for a number worth quoting)")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "adagrad_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        def emit(row):
            line = json.dumps(row)
            f.write(line + "\n")
            f.flush()
            print(line, flush=True)

        for label in a.shapes.split(","):
            shape = SHAPES[label]
            E, R, d, gamma, B, n = shape
            Le = 2 * d
            batches = make_batches(E, R, B, n, dev)
            runs = {k: Runner(v[0], shape, dev, True, batches) for k, v in OPTIMIZERS.items()}
            for r in runs.values():
                for _ in range(a.warmup):
                    r.step()
            torch.cuda.synchronize(dev)
            ops.raise_on_device_error(dev)
            base = dict(shape=label, model="RotatE", E=E, R=R, d=d, batch=B, nneg=n, steps_per_window=a.steps)
            times = {k: [] for k in runs}
            for w in range(a.windows):
                for k, r in runs.items():  # lazy_adam, adagrad, adagrad_rowwise, lazy_adam, ...
                    times[k].append(r.window(a.steps, dev))
                    emit(dict(base, kind="window", optimizer=k, window=w, ms_per_step=round(times[k][-1], 5),
                              state_bytes=OPTIMIZERS[k][1](E, Le), table_bytes_per_touched_element=OPTIMIZERS[k][2]))
            ent = {k: r.entity_launch_ms(40, dev) for k, r in runs.items()}
            ops.raise_on_device_error(dev)
            adam = stats(times["lazy_adam"])
            for k in runs:
                s = stats(times[k])
                row = dict(base, kind="summary", optimizer=k, **s, entity_launch_ms=ent[k][0],
                           state_bytes=OPTIMIZERS[k][1](E, Le),
                           touched_rows_mean=float(np.mean([b[4] for b in batches])))
                if k == "adagrad":
                    row["accepted"] = bool(s["median_ms"] <= adam["median_ms"] + adam["spread_ms"])
                emit(row)
            del runs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
