"""The status every bad kge_rank_candidates call returns, one row per host-side
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
SHORT = "short"  # one byte under kge_rank_candidates_workspace_bytes
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


WIDE = dict(model=0, entity_dim=20000, relation_dim=20000)  # rows read in place: q vectors in the workspace
VALID = dict(m={}, mode=2, queries=P, nq=4, cand=P, ncand=10, ranks=P, ties=P, ws=P, ws_bytes=AMPLE, err=P,
             stream=NULL)

# (overrides of the valid call, status), in the order the checks run
CASES = [
    # 1. the model, as every entry
    (dict(m=dict(null=True)), ARG),
    (dict(m=dict(struct_size=C.sizeof(_lib.ModelDesc) - 8)), ABI),
    (dict(m=dict(model=5)), MODEL),
    (dict(m=dict(relation_dim=16)), SHAPE),
    (dict(m=dict(model=5), mode=0), MODEL),              # the model before the mode
    # 2. the mode
    (dict(mode=0), MODE),                                # KGE_SINGLE
    (dict(mode=3), MODE),
    (dict(mode=0, queries=NULL), MODE),                  # the mode before the pointers
    (dict(mode=0, ncand=0), MODE),
    # 3. pointers and sizes
    (dict(queries=NULL), ARG),
    (dict(cand=NULL), ARG),
    (dict(ranks=NULL), ARG),
    (dict(err=NULL), ARG),
    (dict(nq=-1), ARG),
    (dict(ncand=0), ARG),
    (dict(ncand=-5), ARG),
    (dict(queries=NULL, nq=0), ARG),                     # the pointers before the empty call
    (dict(ncand=0, nq=0), ARG),
    (dict(nq=GRID, ncand=0), ARG),                       # the sizes before the grid
    # 4. the empty call
    (dict(nq=0), OK),
    (dict(nq=0, ws=NULL, ws_bytes=0), OK),               # ... before the workspace
    # 5. the grid
    (dict(nq=GRID), DIM),
    (dict(nq=GRID // 2, ncand=65 * 1024), DIM),          # 2^30 queries × 65 chunks of at most 1024 candidates
    (dict(nq=GRID, ws=NULL, ws_bytes=0), DIM),           # the grid before the workspace
    # 6. the workspace
    (dict(ws_bytes=SHORT), WORKSPACE),
    (dict(ws=NULL), WORKSPACE),
    (dict(m=WIDE, ws_bytes=SHORT), WORKSPACE),
    (dict(nq=70001, ncand=3, ws_bytes=SHORT), WORKSPACE),  # past the other ranking calls' 65,535 queries: no KGE_ERR_DIM
    (dict(ties=NULL, ws_bytes=SHORT), WORKSPACE),        # ties_out is optional
]


def _call(over):
    a = dict(VALID)
    a.update(over)
    m = _model(**a["m"])
    lib = _lib.load()
    if a["ws_bytes"] == SHORT:
        need = lib.kge_rank_candidates_workspace_bytes(m, a["nq"], a["ncand"])
        assert need > 0
        a["ws_bytes"] = need - 1
    return lib.kge_rank_candidates(m, a["mode"], a["queries"], a["nq"], a["cand"], a["ncand"], a["ranks"], a["ties"],
                                   a["ws"], a["ws_bytes"], a["err"], a["stream"])


@pytest.mark.parametrize("over,status", CASES, ids=[f"{i:02d}" for i in range(len(CASES))])
def test_status(over, status):
    assert _call(over) == status


def test_workspace_never_holds_a_score_matrix():
    """[nq, ncand] fp32 would be 4·nq·ncand bytes; the workspace is two int32
    counters per query, plus the q vectors only when rows are read in place."""
    lib = _lib.load()
    m = _model(model=0, entity_dim=64, relation_dim=64, nentity=1 << 20, nrelation=3)
    nq = 65536
    need = lib.kge_rank_candidates_workspace_bytes(m, nq, 500)
    assert 8 * nq <= need <= 8 * nq + 4096
    assert lib.kge_rank_candidates_workspace_bytes(m, nq, 100000) == need  # does not grow with the lists
    wide = lib.kge_rank_candidates_workspace_bytes(_model(**WIDE), 16, 500)
    assert 16 * 20000 * 4 <= wide <= 16 * 20000 * 4 + 8192
    # a bad model or size: 0
    assert lib.kge_rank_candidates_workspace_bytes(_model(model=5), nq, 500) == 0
    assert lib.kge_rank_candidates_workspace_bytes(m, -1, 500) == 0
    assert lib.kge_rank_candidates_workspace_bytes(m, nq, 0) == 0


def test_header_documents_the_order_and_keeps_the_abi():
    hdr = (Path(__file__).resolve().parents[1] / "include" / "kge_hip.h").read_text()
    doc = hdr[hdr.index("PER-QUERY CANDIDATE LISTS"):hdr.index("size_t kge_rank_candidates_workspace_bytes")]
    order = [doc.index(w) for w in ("the model (as every entry)", "KGE_ERR_MODE", "KGE_ERR_ARG", "nq == 0 returns KGE_OK",
                                    "KGE_ERR_DIM", "KGE_ERR_WORKSPACE")]
    assert order == sorted(order)
    assert re.search(r'#define KGE_ABI_VERSION "0\.5"', hdr) and _lib.ABI_VERSION == "0.5"
