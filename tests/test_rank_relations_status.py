"""The status every bad kge_rank_relations call returns, one row per host-side
check in the order the header documents (no device work: each row returns
before any launch; the pointers are host addresses the library never
dereferences).  Where two checks could both fire, the row shows which wins.
"""
import ctypes as C
import re
from pathlib import Path

import pytest

from knowledgegraphembedding_amd import _lib

OK, MODEL, MODE, SHAPE, ARG, WORKSPACE, DIM, ABI = range(8)

_RAW = C.create_string_buffer(8192 + 128)
_BASE = (C.addressof(_RAW) + 127) & ~127
ENT, REL, MOD, P = _BASE, _BASE + 1024, _BASE + 2048, _BASE + 3072
AMPLE = 1 << 40
SHORT = "short"  # one byte under kge_rank_relations_workspace_bytes
NULL = None
GRID = 1 << 31   # one work item more than grid.x holds


def _model(**over):
    if over.get("null"):
        return None
    d = _lib.ModelDesc()
    f = dict(model=3, entity_dim=16, relation_dim=8, nentity=10, nrelation=3, gamma=12.0, phase_divisor=0.1,
             phase_divisor_p=0.1, entity_embedding=ENT, relation_embedding=REL, modulus=MOD, relation_trig=0)
    f.update(over)
    for k, v in f.items():
        setattr(d, k, v)
    return d


MANY_REL = dict(nrelation=65 * 1024)  # 65 chunks of at most 1024 relations
VALID = dict(m={}, queries=P, nq=4, off=NULL, ids=NULL, ranks=P, ties=P, scores=NULL, ws=P, ws_bytes=AMPLE, err=P,
             stream=NULL)

# (overrides of the valid call, status), in the order the checks run
CASES = [
    # 1. the model, as every entry
    (dict(m=dict(null=True)), ARG),
    (dict(m=dict(struct_size=C.sizeof(_lib.ModelDesc) - 8)), ABI),
    (dict(m=dict(model=5)), MODEL),
    (dict(m=dict(relation_dim=16)), SHAPE),
    (dict(m=dict(model=5), queries=NULL), MODEL),        # the model before the pointers
    (dict(m=dict(relation_dim=16), nq=-1), SHAPE),
    # 2. null queries / ranks_out / err_flag
    (dict(queries=NULL), ARG),
    (dict(ranks=NULL), ARG),
    (dict(err=NULL), ARG),
    (dict(queries=NULL, nq=0), ARG),                     # the pointers before the empty call
    (dict(ranks=NULL, nq=GRID), ARG),                    # ... and before the grid
    # 3. nq < 0
    (dict(nq=-1), ARG),
    (dict(nq=-1, ws=NULL, ws_bytes=0), ARG),
    # 4. the filter: both or neither
    (dict(off=P), ARG),
    (dict(ids=P), ARG),
    (dict(off=P, nq=0), ARG),                            # the filter before the empty call
    (dict(ids=P, nq=GRID), ARG),                         # ... and before the grid
    # 5. the empty call
    (dict(nq=0), OK),
    (dict(nq=0, ws=NULL, ws_bytes=0), OK),               # ... before the workspace
    (dict(nq=0, off=P, ids=P), OK),
    # 6. the grid
    (dict(nq=GRID), DIM),
    (dict(nq=GRID // 2, m=MANY_REL), DIM),               # 2^30 queries × 65 chunks
    (dict(nq=GRID, ws=NULL, ws_bytes=0), DIM),           # the grid before the workspace
    # 7. the workspace
    (dict(ws_bytes=SHORT), WORKSPACE),
    (dict(ws=NULL), WORKSPACE),
    (dict(m=dict(relation_trig=P), ws_bytes=SHORT), WORKSPACE),
    (dict(nq=70001, ws_bytes=SHORT), WORKSPACE),         # past the other ranking calls' 65,535 queries: no KGE_ERR_DIM
    (dict(ties=NULL, ws_bytes=SHORT), WORKSPACE),        # ties_out is optional
    (dict(scores=P, off=P, ids=P, ws_bytes=SHORT), WORKSPACE),  # scores_out and a filter: a valid call so far
]


def _call(over):
    a = dict(VALID)
    a.update(over)
    m = _model(**a["m"])
    lib = _lib.load()
    if a["ws_bytes"] == SHORT:
        need = lib.kge_rank_relations_workspace_bytes(m, a["nq"])
        assert need > 0
        a["ws_bytes"] = need - 1
    return lib.kge_rank_relations(m, a["queries"], a["nq"], a["off"], a["ids"], a["ranks"], a["ties"], a["scores"],
                                  a["ws"], a["ws_bytes"], a["err"], a["stream"])


@pytest.mark.parametrize("over,status", CASES, ids=[f"{i:02d}" for i in range(len(CASES))])
def test_status(over, status):
    assert _call(over) == status


def test_workspace_never_holds_a_score_matrix():
    """[nq, R] fp32 would be 4·nq·R bytes; the workspace is two int32 counters
    per query, plus RotatE's [R, 2, relation_dim] table when the caller gives
    none — it does not grow with R beyond that table."""
    lib = _lib.load()
    nq = 65536
    small = _model(model=0, entity_dim=64, relation_dim=64, nentity=1 << 20, nrelation=3)
    need = lib.kge_rank_relations_workspace_bytes(small, nq)
    assert 8 * nq <= need <= 8 * nq + 4096
    for R in (1345, 100000):
        m = _model(model=0, entity_dim=64, relation_dim=64, nentity=1 << 20, nrelation=R)
        assert lib.kge_rank_relations_workspace_bytes(m, nq) == need  # does not grow with R
        assert need < 4 * nq * R
        rot = _model(model=3, entity_dim=128, relation_dim=64, nentity=1 << 20, nrelation=R)
        table = R * 2 * 64 * 4
        got = lib.kge_rank_relations_workspace_bytes(rot, nq)
        assert need + table <= got <= need + table + 4096 and got < 4 * nq * R
        rot.relation_trig = P  # the caller's table: none in the workspace
        assert lib.kge_rank_relations_workspace_bytes(rot, nq) == need
    # a bad model or size: 0
    assert lib.kge_rank_relations_workspace_bytes(_model(model=5), nq) == 0
    assert lib.kge_rank_relations_workspace_bytes(small, -1) == 0


def test_header_documents_the_order_and_keeps_the_abi():
    hdr = (Path(__file__).resolve().parents[1] / "include" / "kge_hip.h").read_text()
    doc = hdr[hdr.index("RELATION PREDICTION"):hdr.index("size_t kge_rank_relations_workspace_bytes")]
    order = [doc.index(w) for w in ("the model (as every entry)", "null queries /", "nq < 0 (KGE_ERR_ARG)",
                                    "not both NULL or both set (KGE_ERR_ARG)", "nq == 0 returns KGE_OK", "KGE_ERR_DIM",
                                    "KGE_ERR_WORKSPACE")]
    assert order == sorted(order)
    assert "no mode argument" in doc and "pRotatE" in doc
    assert re.search(r'#define KGE_ABI_VERSION "0\.5"', hdr) and _lib.ABI_VERSION == "0.5"
