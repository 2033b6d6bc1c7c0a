"""The shapes of tests/test_arena_gpu.py and the workspace-size queries its
arenas are sized from (shared with tests/test_arena_ref.py, which needs no GPU).

Shapes: the smallest at which a bound can still be missed.  E = 257 is odd and
no multiple of 32, 64 or 128 (a 9-word filter bitmap with one live bit in the
last word, 5 tiles of 64, 3 MFMA blocks of 128 with the last almost empty);
E = 256 is the exact-multiple edge.  Spans (floats per half-row): 36 = 9
16-byte slots, 37 = single-float slots, 280 = 70 slots (RotatE: the sliced
entity pass picks 2 slices), 2052 = the wide-row kernels (E = 64 there).
"""
from dataclasses import dataclass

NAMES = ("TransE", "DistMult", "ComplEx", "RotatE", "pRotatE")
MODES = ("head-batch", "tail-batch")
DOUBLE = {"TransE": (1, 1), "DistMult": (1, 1), "ComplEx": (2, 2), "RotatE": (2, 1), "pRotatE": (1, 1)}
R = 5
R_REL = 65        # relation prediction also with more relations than a wave
B = 5             # not the 4 rows of a block
NNEG = (3, 65)    # k_row's four waves; more than one wave of negatives
NQS = (1, 65)
KS = (1, 128)
PARTS = (0, 2, 5)  # 5 tiles at E = 257: 5 is the "one part per tile" limit
NCAND = (1, 65)
GAMMA = 12.0
WIDE = 2052
WIDE_E = 64


@dataclass(frozen=True)
class Shape:
    name: str
    E: int
    d: int          # the span: floats per half-row
    R: int = R
    seed: int = 7

    @property
    def id(self):
        return f"{self.name}-E{self.E}-d{self.d}" + (f"-R{self.R}" if self.R != R else "")

    @property
    def le(self):
        return self.d * DOUBLE[self.name][0]

    @property
    def lr(self):
        return self.d * DOUBLE[self.name][1]


# (pRotatE 256 / 37 with seed 7 and n = 65: the fp32 oracle itself is 8.9e-5 from fp64 on one
# gradient row, above test_slot_matrix_ref's cap of 5e-5 on rho_case; seed 9 gives 1.7e-6.  The
# cap stays, the case gets another seed — that module's rule.)
SEEDS = {("pRotatE", 256, 37): 9}
SMALL = tuple(Shape(nm, E, d, seed=SEEDS.get((nm, E, d), 7)) for nm in NAMES for E, d in ((257, 36), (256, 37)))
SLICED = (Shape("RotatE", 257, 280),)
WIDE_SHAPES = (Shape("TransE", WIDE_E, WIDE), Shape("RotatE", WIDE_E, WIDE))
REL_SHAPES = tuple(Shape(nm, 257, 36, R=R_REL) for nm in NAMES) + (Shape("RotatE", 256, 37, R=R_REL),
                                                                    Shape("DistMult", WIDE_E, WIDE))
ALL_SHAPES = SMALL + SLICED + WIDE_SHAPES + REL_SHAPES


def workspace_queries(lib, desc):
    """{label: bytes} of every *_workspace_bytes query at every shape the GPU module calls it with."""
    out = {}
    for n in NNEG:
        out[f"train B{B} n{n}"] = lib.kge_train_workspace_bytes(desc, B, n)
        out[f"train B{B // 2} n{n}"] = lib.kge_train_workspace_bytes(desc, B // 2, n)
        out[f"train B{B - B // 2} n{n}"] = lib.kge_train_workspace_bytes(desc, B - B // 2, n)
        out[f"lazy B{B} n{n}"] = lib.kge_train_lazy_workspace_bytes(desc, B, n)
        for mode in (1, 2):
            out[f"backward m{mode} n{n}"] = lib.kge_backward_workspace_bytes(desc, mode, B, n)
    out["lazy B2 n3"] = lib.kge_train_lazy_workspace_bytes(desc, 2, 3)
    out["backward m0"] = lib.kge_backward_workspace_bytes(desc, 0, B, 1)
    for nq in NQS:
        out[f"rank nq{nq}"] = lib.kge_rank_workspace_bytes(desc, nq)
        out[f"rank nq{2 * nq}"] = lib.kge_rank_workspace_bytes(desc, 2 * nq)
        out[f"rel nq{nq}"] = lib.kge_rank_relations_workspace_bytes(desc, nq)
        for c in NCAND:
            out[f"cand nq{nq} C{c}"] = lib.kge_rank_candidates_workspace_bytes(desc, nq, c)
        for k in KS:
            for parts in PARTS:
                out[f"topk nq{nq} k{k} parts{parts}"] = lib.kge_topk_workspace_bytes(desc, nq, k, parts)
    return out
