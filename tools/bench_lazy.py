#!/usr/bin/env python
"""Timing of the lazy entity Adam (KGELazyAdam, kge_train_step_lazy) against the
dense fused step (KGEAdam, kge_train_step) in one process: after a warm-up the
two run in alternating windows of --steps fused train steps each (default 200),
--windows times, on the same pre-built batches (uniform negatives, the modes
alternating).  Two shapes:

  fb15k   RotatE E=14951 R=1345 d=1000 b=1024 n=256 (bench.py's shape): the
          batch touches essentially every row, so lazy should cost what dense
          costs plus the touched-row compaction;
  2m      RotatE E=2,000,000 R=1345 d=200 b=1024 n=256, a synthetic table
          (entity table and moments 9.6 GB): dense streams all of it every
          step, lazy the <= 266,240 rows the batch touches.

Per shape one JSON line: every window's ms per step for both, their medians and
spreads (max - min over the windows), the entity launch's time for both from
the stage timer (stage 4, a separate short run: the timer's events cost time),
the mean number of touched rows, and the bytes each entity pass moves, computed
from the shapes (dense: 24 B per table element, 28 with the gradient kept;
lazy: 24 B per element of a touched row plus 8 B of CSR offsets per entity for
the compaction).

    python tools/bench_lazy.py [--shapes fb15k,2m] [--steps 200] [--windows 3] [--json out.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
from argparse import Namespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from knowledgegraphembedding_amd import KGEAdam, KGELazyAdam, KGEModel, _lib, ops  # noqa: E402

SHAPES = {
    # E, R, d, gamma, B, n
    "fb15k": (14951, 1345, 1000, 24.0, 1024, 256),
    "2m": (2_000_000, 1345, 200, 12.0, 1024, 256),
}
NBATCH = 8


def make_model(E, R, d, gamma, dev, seed):
    """RotatE with an [E, 2d] table initialised on the device (the reference's
    uniform range; a CPU init of a 3.2 GB table would dominate the run)."""
    m = KGEModel("RotatE", 8, R, d, gamma, True, False).to(dev)
    r = m.embedding_range.item()
    g = torch.Generator(device=dev).manual_seed(seed)
    m.nentity = E
    m.entity_embedding = torch.nn.Parameter(torch.empty(E, 2 * d, device=dev).uniform_(-r, r, generator=g))
    return m


def make_batches(E, R, B, n, dev):
    g = torch.Generator().manual_seed(11)
    out = []
    for k in range(NBATCH):
        pos = torch.stack([torch.randint(0, E, (B,), generator=g), torch.randint(0, R, (B,), generator=g),
                           torch.randint(0, E, (B,), generator=g)], 1)
        neg = torch.randint(0, E, (B, n), generator=g)
        w = torch.rand(B, generator=g) + 0.2
        touched = int(torch.unique(torch.cat([pos[:, 0], pos[:, 2], neg.reshape(-1)])).numel())
        out.append((pos.to(dev), neg.to(dev), w.to(dev), "head-batch" if k % 2 == 0 else "tail-batch", touched))
    return out


class Runner:
    def __init__(self, cls, shape, dev, keep_grads, batches):
        E, R, d, gamma, B, n = shape
        self.m = make_model(E, R, d, gamma, dev, seed=1)
        self.m.keep_grads = keep_grads
        self.opt = cls([self.m.entity_embedding, self.m.relation_embedding], lr=1e-4)
        self.args = Namespace(negative_adversarial_sampling=True, adversarial_temperature=1.0, uni_weight=False,
                              regularization=0.0)
        self.batches = batches
        self.k = 0

    def step(self):
        pos, neg, w, mode, _ = self.batches[self.k % NBATCH]
        self.k += 1
        self.m.compute_train_grads(pos, neg, w, mode, self.args, optimizer=self.opt)
        self.opt.step()

    def window(self, steps, dev):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            self.step()
        b.record()
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b) / steps

    def entity_launch_ms(self, steps, dev):
        """Stage 4 of the training stage timer (entity-major pass + fused Adam), per call."""
        lib = _lib.load()
        _lib.check(lib.kge_stage_timer(1, None, 1), "kge_stage_timer")
        for _ in range(steps):
            self.step()
        torch.cuda.synchronize(dev)
        out = np.zeros(7, dtype=np.float32)
        _lib.check(lib.kge_stage_timer(2, out.ctypes.data_as(ctypes.c_void_p), 7), "kge_stage_timer")
        lib.kge_stage_timer(0, None, 0)
        return float(out[4] / max(out[6], 1)), float(out[3] / max(out[6], 1))


def stats(xs):
    return dict(windows_ms=[round(x, 5) for x in xs], median_ms=float(np.median(xs)), spread_ms=float(max(xs) - min(xs)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="fb15k,2m")
    ap.add_argument("--steps", type=int, default=200, help="steps per window (>= 200 for a number worth quoting)")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--keep-grads", type=int, default=1, help="dense: leave the gradients in .grad, as bench.py does")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows = []
    for label in a.shapes.split(","):
        shape = SHAPES[label]
        E, R, d, gamma, B, n = shape
        batches = make_batches(E, R, B, n, dev)
        runs = {"dense": Runner(KGEAdam, shape, dev, bool(a.keep_grads), batches),
                "lazy": Runner(KGELazyAdam, shape, dev, bool(a.keep_grads), batches)}
        for r in runs.values():
            for _ in range(a.warmup):
                r.step()
        torch.cuda.synchronize(dev)
        ops.raise_on_device_error(dev)
        times = {k: [] for k in runs}
        for _ in range(a.windows):
            for k, r in runs.items():  # dense, lazy, dense, lazy, ...
                times[k].append(r.window(a.steps, dev))
        ent = {k: r.entity_launch_ms(40, dev) for k, r in runs.items()}
        ops.raise_on_device_error(dev)
        touched = float(np.mean([b[4] for b in batches]))
        Le = 2 * d
        row = dict(shape=label, model="RotatE", E=E, R=R, d=d, batch=B, nneg=n, steps_per_window=a.steps,
                   keep_grads=bool(a.keep_grads), dense=stats(times["dense"]), lazy=stats(times["lazy"]),
                   lazy_over_dense=float(np.median(times["lazy"]) / np.median(times["dense"])),
                   entity_launch_ms=dict(dense=ent["dense"][0], lazy=ent["lazy"][0]),
                   csr_wait_ms=dict(dense=ent["dense"][1], lazy=ent["lazy"][1]),
                   touched_rows_mean=touched, launch_row_places=min(E, B * n + 2 * B),
                   entity_pass_bytes=dict(dense=E * Le * (28 if a.keep_grads else 24),
                                          lazy=int(touched * Le * 24 + 8 * E)))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del runs
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
