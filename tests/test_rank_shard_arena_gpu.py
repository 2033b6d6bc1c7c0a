"""kge_rank_shard's three stages on exactly sized, guard-banded device buffers
(tests/arena.py): every rank's shard sits alone inside a poisoned allocation,
the descriptor's entity pointer own_begin rows before it; queries, filter,
fixed_rows, s_true, counts and the error flag are exactly sized, the workspace
poisoned and of exactly the queried size.  No guard byte may change, the inputs
keep their bytes, and the counts are the oracle's — a read outside the shard
would meet poison (NaN rows, ids far above the entity count).
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


def _call(desc, mode, sh, stage, q, nq, ws, err):
    st = _lib.load().kge_rank_shard(C.byref(desc), _lib.MODE_IDS[mode], C.byref(sh), stage, q.ptr(), nq, ws.ptr(),
                                    ws.nbytes, err.ptr(), ops._stream(DEV))
    assert st == 0, _lib.load().kge_status_string(st).decode()


# RotatE 20: 16-byte slots; TransE 37: single-float slots; RotatE 9000: rows read in place, q in the workspace
@pytest.mark.parametrize("case,world", [(S.BASE[3], "w4"), (S.BASE[0], "w3"), (S.BASE[1], "w2"), (S.WIDTHS[3], "w2")],
                         ids=lambda x: x if isinstance(x, str) else x.id)
@pytest.mark.parametrize("form", S.FORMS)
def test_stages_in_arenas(case, world, form):
    ent, rel, mod, erange = S.tables(case)
    le, nq = ent.shape[1], case.nq
    a_rel = arena_of(rel.copy(), DEV, name="relation")
    a_mod = None if mod is None else arena_of(mod.copy(), DEV, name="modulus")
    trig = ops.reference_rotation(torch.from_numpy(rel.copy()), erange) if case.name == "RotatE" else None
    a_trig = None if trig is None else arena_of(trig, DEV, name="trig")
    a_q = arena_of(S.queries(case).copy(), DEV, name="queries")
    a_err = arena_of(torch.zeros(1, dtype=torch.int32), DEV, name="err")
    ranges = S.splits(case.E)[world]
    for mode in S.MODES:
        off, ids = S.filt(case, mode, form)
        a_off = arena_of(off.copy(), DEV, name="filt_off")
        a_ids = arena_of(ids.copy(), DEV, name="filt_ids")
        shards = []
        for b, e in ranges:
            rows = ent[b:e].copy() if e > b else np.full((1, le), np.nan, np.float32)  # (empty: a row never read)
            a_ent = arena_of(rows, DEV, name=f"shard [{b}, {e})")
            d = ops.make_desc(case.name, a_ent.view, a_rel.view, S.GAMMA, erange, None if a_mod is None else a_mod.view)
            d.entity_embedding = a_ent.ptr() - b * le * 4
            d.nentity = case.E
            if a_trig is not None:
                d.relation_trig = a_trig.ptr()
            need = _lib.load().kge_rank_shard_workspace_bytes(C.byref(d), nq)
            sh = _lib.RankShardDesc()
            sh.own_begin, sh.own_end = b, e
            sh.flags = _lib.RANK_FILTER_TABLE if form == "table" else 0
            sh.filt_off, sh.filt_ids = a_off.ptr(), a_ids.ptr()
            shards.append((a_ent, d, sh, arena((need,), torch.uint8, DEV, name="workspace"), rows))
        held = [a_rel, a_q, a_err, a_off, a_ids] + [x for x in (a_mod, a_trig) if x is not None]

        def stage(k, field, shape, dtype):
            """Stage k on every shard into a fresh poisoned buffer each; returns the buffers."""
            outs = []
            for a_ent, d, sh, ws, _ in shards:
                o = arena(shape, dtype, DEV, name=field)
                setattr(sh, field, o.ptr())
                _call(d, mode, sh, k, a_q, nq, ws, a_err)
                outs.append(o)
            torch.cuda.synchronize(DEV)
            for o in outs + held + [x for s in shards for x in (s[0], s[3])]:
                o.check()
            return outs

        def reduced(outs, shape):
            tot = sum(o.view.view(torch.int32) for o in outs).view(torch.float32)
            r = arena_of(tot.cpu().reshape(shape), DEV, name="reduced")
            for _, _, sh, _, _ in shards:
                setattr(sh, "fixed_rows" if len(shape) == 2 else "s_true", r.ptr())
            return r

        fixed = reduced(stage(_lib.RSHARD_ROWS, "fixed_rows", (nq, le), torch.float32), (nq, le))
        x = S.queries(case)[:, 2 if mode == "head-batch" else 0]
        fixed.unchanged(np.ascontiguousarray(ent[x]))
        s_true = reduced(stage(_lib.RSHARD_TRUE, "s_true", (nq,), torch.float32), (nq,))
        fixed.unchanged(np.ascontiguousarray(ent[x]))
        s_true.unchanged(np.ascontiguousarray(S.scores(case, mode)[:, 0]))
        held += [fixed, s_true]
        counts = stage(_lib.RSHARD_COUNT, "counts", (2, nq), torch.int64)
        assert int(a_err.view.item()) == 0
        for (b, e), o, (a_ent, _, _, _, rows) in zip(ranges, counts, shards):
            o.unchanged(S.shard_counts(case, mode, b, e))
            a_ent.unchanged(rows)
        fixed.unchanged(np.ascontiguousarray(ent[x]))
        s_true.unchanged(np.ascontiguousarray(S.scores(case, mode)[:, 0]))
        for o, src in ((a_rel, rel), (a_q, S.queries(case)), (a_off, off), (a_ids, ids)):
            o.unchanged(src.copy())
