"""kge_rank_candidates_shard on exactly sized, guard-banded device buffers
(tests/arena.py): every rank's shard sits alone inside a poisoned allocation,
the descriptor's entity pointer own_begin rows before it; queries, candidate
lists, fixed_rows, s_true, counts and the error flag are exactly sized, the
workspace poisoned and of exactly the queried size.  No guard byte may change,
the inputs keep their bytes, and the counts are the oracle's — a read outside
the shard would meet poison (NaN rows), a read outside a list ids far above the
entity count, which raise the error flag.

fixed_rows and s_true are the reduced stage outputs, written here from the host:
the fixed side's table rows and the oracle's true scores, the bits
kge_rank_shard's ROWS and TRUE stages give (test_rank_candidates_shard_gpu.py).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import rank_candidates_cases as K
import rank_candidates_shard_cases as X
from arena import arena, arena_of
from knowledgegraphembedding_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


# RotatE 20: 16-byte slots; TransE 37 (with padding): single-float slots; DistMult 40 with lists of
# two chunks; RotatE 9000: rows read in place, q in the workspace
@pytest.mark.parametrize("case,world", [(K.BASE[3], "w4"), (K.PADDED[2], "w3"), (K.LENGTHS[5], "w2"), (K.WIDTHS[6], "w2")],
                         ids=lambda x: x if isinstance(x, str) else x.id)
def test_entry_in_arenas(case, world):
    ent, rel, mod, erange = K.tables(case)
    le, nq = ent.shape[1], case.nq
    a_rel = arena_of(rel.copy(), DEV, name="relation")
    trig = ops.reference_rotation(torch.from_numpy(rel.copy()), erange) if case.name == "RotatE" else None
    a_trig = None if trig is None else arena_of(trig, DEV, name="trig")
    a_q = arena_of(K.queries(case).copy(), DEV, name="queries")
    a_err = arena_of(torch.zeros(1, dtype=torch.int32), DEV, name="err")
    ranges = X.splits(case, world)
    lib = _lib.load()
    for mode in X.MODES:
        cand = K.cand(case, mode)
        a_cand = arena_of(cand.copy(), DEV, name="cand")
        fixed_h = np.ascontiguousarray(ent[K.queries(case)[:, 2 if mode == "head-batch" else 0]])
        st_h = np.ascontiguousarray(K.scores(case, mode)[:, 0])
        a_fixed = arena_of(fixed_h, DEV, name="fixed_rows")
        a_st = arena_of(st_h, DEV, name="s_true")
        held = [a_rel, a_q, a_err, a_cand, a_fixed, a_st] + ([a_trig] if a_trig is not None else [])
        outs = []
        for b, e in ranges:
            rows = ent[b:e].copy() if e > b else np.full((1, le), np.nan, np.float32)  # (empty: a row never read)
            a_ent = arena_of(rows, DEV, name=f"shard [{b}, {e})")
            d = ops.make_desc(case.name, a_ent.view, a_rel.view, K.GAMMA, erange, None)
            d.entity_embedding = a_ent.ptr() - b * le * 4
            d.nentity = case.E
            if a_trig is not None:
                d.relation_trig = a_trig.ptr()
            need = lib.kge_rank_candidates_shard_workspace_bytes(C.byref(d), nq, case.C)
            assert need >= 256 and (need == 256) == (le < 9000)
            ws = arena((need,), torch.uint8, DEV, name="workspace")
            o = arena((2, nq), torch.int64, DEV, name="counts")
            sh = _lib.RankCandShardDesc()
            sh.own_begin, sh.own_end = b, e
            sh.fixed_rows, sh.s_true, sh.counts = a_fixed.ptr(), a_st.ptr(), o.ptr()
            st = lib.kge_rank_candidates_shard(C.byref(d), _lib.MODE_IDS[mode], C.byref(sh), a_q.ptr(), nq, a_cand.ptr(),
                                               case.C, ws.ptr(), ws.nbytes, a_err.ptr(), ops._stream(DEV))
            assert st == 0, lib.kge_status_string(st).decode()
            outs.append((o, a_ent, ws, rows))
        torch.cuda.synchronize(DEV)
        assert int(a_err.view.item()) == 0
        for x in held:
            x.check()
        for (b, e), (o, a_ent, ws, rows) in zip(ranges, outs):
            for x in (o, a_ent, ws):
                x.check()
            o.unchanged(X.shard_counts(case, mode, b, e))
            a_ent.unchanged(rows)
        for x, src in ((a_rel, rel), (a_q, K.queries(case)), (a_cand, cand), (a_fixed, fixed_h), (a_st, st_h)):
            x.unchanged(src.copy())
