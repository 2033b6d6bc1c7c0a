"""The child of tests/test_graph_gpu.py::test_cold_capture_in_a_fresh_process.

A fresh process in which the library has made no call that touches the device:
its first is kge_rank_filtered_ex under KGE_RANK_SIDE=1 inside a stream capture
(side_for_device() creates the side stream and its six events there, the call
forks the table's work onto the new stream and joins it, the ranking kernels'
code objects load there), its second kge_topk with k = 128 inside another
capture (launch_topk_tile's hipFuncSetAttribute).  (The issue's first call,
kge_train_step_grads, is left out with the rest of the training family: see
tests/test_graph_gpu.py.)  Both graphs are replayed, and only
then the same programs are run eagerly on other buffers: the bits must agree.
A failed capture is an error return (printed), not a fault.  Prints one line
starting "cold capture:" for the parent to assert on.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (HERE, os.path.dirname(HERE)) if p not in sys.path]

import torch  # noqa: E402

import graph_cases as G  # noqa: E402
from test_arena_gpu import MODES, Bufs, same  # noqa: E402
from test_gpu_parity import DEV  # noqa: E402
from test_graph_gpu import eager, make_rank, make_topk  # noqa: E402


def cold(make, shape, name):
    p = make(Bufs(True), shape)
    p.reset(shape)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize(DEV)
    try:
        with torch.cuda.graph(graph):
            p.run()
    except (AssertionError, RuntimeError) as e:
        return None, f"{name} capture failed: {str(e).splitlines()[0]}"
    torch.cuda.synchronize(DEV)
    p.b.arenas[p.probe].poisoned()
    graph.replay()
    p.b.verify(f"{name} cold replay")
    return (p, graph, p.snapshot()), f"{name} ok"


def main():
    shape = G.E257[1]  # DistMult: the MFMA tile, whose table work KGE_RANK_SIDE=1 moves to the side stream
    os.environ["KGE_RANK_SIDE"] = "1"  # (read by the library at each call)
    runs, notes = [], []
    for make, name in ((make_rank(MODES[1], 1), "kge_rank_filtered_ex"),
                       (make_topk(MODES[1], 128, 0), "kge_topk k=128")):
        r, note = cold(make, shape, name)
        runs.append((make, name, r))
        notes.append(note)
        if r is None:
            break
    for make, name, r in runs:
        if r is None:
            continue
        want = eager(make(Bufs(True), shape), shape)[0]
        bad = [k for k in want if not same(r[2][k], want[k])]
        if bad:
            notes[[n for _, n, _ in runs].index(name)] = f"{name} differs from the eager call in {bad}"
    print("cold capture: " + ", ".join(notes))


if __name__ == "__main__":
    main()
