"""kge_rank_shard_fast on exactly sized, guard-banded device buffers
(tests/arena.py), as test_rank_shard_arena_gpu.py runs the exact stages: every
rank's shard sits alone inside a poisoned allocation, the descriptor's entity
pointer own_begin rows before it; queries, filter, fixed_rows, s_true, counts,
listed_out and the error flag are exactly sized, the workspace poisoned and of
exactly the queried size.  No guard byte may change, the inputs keep their
bytes, and the counts are the oracle's — a read outside [own_begin, own_end)
would meet poison (NaN rows would surface in the counts; ids far above the
entity count would raise the error flag), and so would a workspace word the
call read before a kernel of its own wrote it.  The split-bf16 tile (path 1) and
the register tile (path 2).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import rank_shard_cases as S
from arena import arena, arena_of
from knowledgegraphembedding_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TRANSE36 = S.Case("TransE", 36, plant=True)

# (case, world, path): DistMult 40 on both tiles; RotatE 20 and TransE 36 (a zero window) on the register tile;
# w3 has the one-row shard and the empty one
RUNS = [(S.BASE[1], "w4", 1), (S.BASE[1], "w3", 2), (S.BASE[2], "w2", 1), (S.BASE[3], "w4", 2), (TRANSE36, "w3", 2)]


@pytest.mark.parametrize("case,world,path", RUNS, ids=lambda x: getattr(x, "id", x))
@pytest.mark.parametrize("form", S.FORMS)
def test_fast_entry_in_arenas(case, world, path, form):
    lib = _lib.load()
    ent, rel, mod, erange = S.tables(case)
    le, nq = ent.shape[1], case.nq
    a_rel = arena_of(rel.copy(), DEV, name="relation")
    trig = ops.reference_rotation(torch.from_numpy(rel.copy()), erange) if case.name == "RotatE" else None
    a_trig = None if trig is None else arena_of(trig, DEV, name="trig")
    a_q = arena_of(S.queries(case).copy(), DEV, name="queries")
    a_err = arena_of(torch.zeros(1, dtype=torch.int32), DEV, name="err")
    ranges = S.splits(case.E)[world]
    for mode in S.MODES:
        off, ids = S.filt(case, mode, form)
        a_off = arena_of(off.copy(), DEV, name="filt_off")
        a_ids = arena_of(ids.copy(), DEV, name="filt_ids")
        x = S.queries(case)[:, 2 if mode == "head-batch" else 0]
        fixed_h = np.ascontiguousarray(ent[x])
        st_h = np.ascontiguousarray(S.scores(case, mode)[:, 0])
        a_fixed = arena_of(fixed_h, DEV, name="fixed_rows")  # the reduced stage buffers (pinned bit for bit by
        a_st = arena_of(st_h, DEV, name="s_true")            # test_rank_shard_arena_gpu.py): the oracle's
        held = [a_rel, a_q, a_err, a_off, a_ids, a_fixed, a_st] + ([a_trig] if a_trig is not None else [])
        for b, e in ranges:
            rows = ent[b:e].copy() if e > b else np.full((1, le), np.nan, np.float32)  # (empty: a row never read)
            a_ent = arena_of(rows, DEV, name=f"shard [{b}, {e})")
            d = ops.make_desc(case.name, a_ent.view, a_rel.view, S.GAMMA, erange, None)
            d.entity_embedding = a_ent.ptr() - b * le * 4
            d.nentity = case.E
            if a_trig is not None:
                d.relation_trig = a_trig.ptr()
            a_counts = arena((2, nq), torch.int64, DEV, name="counts")
            a_listed = arena((nq,), torch.int32, DEV, name="listed")
            sh = _lib.RankShardDesc()
            sh.own_begin, sh.own_end = b, e
            sh.flags = path | (_lib.RANK_FILTER_TABLE if form == "table" else 0)
            sh.filt_off, sh.filt_ids = a_off.ptr(), a_ids.ptr()
            sh.fixed_rows, sh.s_true, sh.counts = a_fixed.ptr(), a_st.ptr(), a_counts.ptr()
            assert lib.kge_rank_shard_fast_path(C.byref(d), C.byref(sh)) == path
            need = lib.kge_rank_shard_fast_workspace_bytes(C.byref(d), C.byref(sh), nq)
            assert need > 0
            ws = arena((need,), torch.uint8, DEV, name="workspace")
            st = lib.kge_rank_shard_fast(C.byref(d), _lib.MODE_IDS[mode], C.byref(sh), a_q.ptr(), nq, a_listed.ptr(),
                                         ws.ptr(), ws.nbytes, a_err.ptr(), ops._stream(DEV))
            assert st == 0, lib.kge_status_string(st).decode()
            torch.cuda.synchronize(DEV)
            for o in held + [a_ent, a_counts, a_listed, ws]:
                o.check()
            assert int(a_err.view.item()) == 0
            a_counts.unchanged(S.shard_counts(case, mode, b, e))
            listed = a_listed.host().numpy()
            assert (listed >= 0).all() and (listed <= max(e - b, 0)).all()
            a_ent.unchanged(rows)
            # one byte short: refused before any launch
            bad = arena((2, nq), torch.int64, DEV, name="counts (refused)")
            sh.counts = bad.ptr()
            assert lib.kge_rank_shard_fast(C.byref(d), _lib.MODE_IDS[mode], C.byref(sh), a_q.ptr(), nq, None, ws.ptr(),
                                           ws.nbytes - 1, a_err.ptr(), ops._stream(DEV)) == 5  # KGE_ERR_WORKSPACE
            torch.cuda.synchronize(DEV)
            bad.poisoned()
        a_fixed.unchanged(fixed_h)
        a_st.unchanged(st_h)
        for o, src in ((a_rel, rel), (a_q, S.queries(case)), (a_off, off), (a_ids, ids)):
            o.unchanged(src.copy())
