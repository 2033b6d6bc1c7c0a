"""The status every bad kge_topk call returns, one row per host-side check in
the order the checks run (no device work: each row returns before any launch;
the pointers are host addresses the library never dereferences).  Where two
checks could both fire, the row shows which wins.
"""
import ctypes as C

import pytest

from knowledgegraphembedding_amd import _lib

OK, MODEL, MODE, SHAPE, ARG, WORKSPACE, DIM, ABI = range(8)

_RAW = C.create_string_buffer(8192 + 128)
_BASE = (C.addressof(_RAW) + 127) & ~127
ENT, REL, MOD, P = _BASE, _BASE + 1024, _BASE + 2048, _BASE + 3072
AMPLE = 1 << 40
SHORT = "short"  # one byte under kge_topk_workspace_bytes
NULL = None
TABLE = _lib.RANK_FILTER_TABLE


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


TRANSE6 = dict(model=0, entity_dim=6, relation_dim=6)        # K % 4 != 0: the wave scan only
ODD_TABLE = dict(entity_embedding=ENT + 4)                    # not 16-byte aligned: the wave scan only
WIDE = dict(model=0, entity_dim=4096, relation_dim=4096)      # rows over 2048 floats
VALID = dict(m={}, mode=2, queries=P, nq=4, filt_off=P, filt_ids=P, k=10, ids=P, scores=P, path=0, parts=0, ws=P,
             ws_bytes=AMPLE, err=P, stream=NULL)

# (overrides of the valid call, status), in the order the checks run
CASES = [
    # the model, as every entry
    (dict(m=dict(null=True)), ARG),
    (dict(m=dict(struct_size=C.sizeof(_lib.ModelDesc) - 8)), ABI),
    (dict(m=dict(model=5)), MODEL),
    (dict(m=dict(relation_dim=16)), SHAPE),
    (dict(m=dict(model=5), mode=0), MODEL),              # the model before the mode
    # mode
    (dict(mode=0), MODE),
    (dict(mode=3), MODE),
    (dict(mode=0, queries=NULL), MODE),                  # the mode before the pointers
    # pointers, sizes, path
    (dict(queries=NULL), ARG),
    (dict(ids=NULL), ARG),
    (dict(scores=NULL), ARG),
    (dict(err=NULL), ARG),
    (dict(nq=-1), ARG),
    (dict(parts=-1), ARG),
    (dict(path=1), ARG),                                 # no MFMA top-k
    (dict(path=4), ARG),
    (dict(path=5), ARG),
    (dict(path=0x100), ARG),                             # a ranking flag that means nothing here
    (dict(path=1, k=0), ARG),                            # the path before k
    (dict(queries=NULL, nq=0), ARG),                     # the pointers before the empty call
    # the empty call
    (dict(nq=0), OK),
    (dict(nq=0, k=0, ws=NULL, ws_bytes=0), OK),          # ... before k and the workspace
    # k, then nq
    (dict(k=0), DIM),
    (dict(k=129), DIM),
    (dict(k=-3), DIM),
    (dict(nq=65536), DIM),
    (dict(k=0, m=TRANSE6, path=2), DIM),                 # k before the path's fit
    (dict(nq=65536, ws_bytes=SHORT), DIM),               # nq before the workspace
    (dict(m=WIDE), DIM),                                 # wide rows are not served
    # the path's fit
    (dict(m=TRANSE6, path=2), ARG),
    (dict(m=ODD_TABLE, path=2), ARG),
    (dict(m=TRANSE6, path=2, ws_bytes=SHORT), ARG),      # the fit before the workspace
    # the workspace
    (dict(ws_bytes=SHORT), WORKSPACE),
    (dict(ws=NULL), WORKSPACE),
    (dict(m=TRANSE6, path=3, ws_bytes=SHORT), WORKSPACE),
    (dict(parts=16, ws_bytes=SHORT), WORKSPACE),
    (dict(k=128, nq=65535, ws_bytes=SHORT), WORKSPACE),
]


def _call(over):
    a = dict(VALID)
    a.update(over)
    m = _model(**a["m"])
    lib = _lib.load()
    if a["ws_bytes"] == SHORT:
        need = lib.kge_topk_workspace_bytes(m, a["nq"], a["k"], a["parts"])
        assert need > 0
        a["ws_bytes"] = need - 1
    return lib.kge_topk(m, a["mode"], a["queries"], a["nq"], a["filt_off"], a["filt_ids"], a["k"], a["ids"],
                        a["scores"], a["path"], a["parts"], a["ws"], a["ws_bytes"], a["err"], a["stream"])


@pytest.mark.parametrize("over,status", CASES, ids=[f"{i:02d}" for i in range(len(CASES))])
def test_status(over, status):
    assert _call(over) == status


def test_workspace_never_holds_a_score_matrix():
    """[nq, E] fp32 would be 4·nq·E bytes; the workspace is q, the bitmap
    (nq·E / 8) and the [nq, parts, k] lists."""
    lib = _lib.load()
    m = _model(model=0, entity_dim=64, relation_dim=64, nentity=1 << 20, nrelation=3)
    nq, k = 4096, 10
    need = lib.kge_topk_workspace_bytes(m, nq, k, 0)
    assert 0 < need < 4 * nq * (1 << 20) // 8
    # more parts, longer lists: the size grows with parts · k only
    more = lib.kge_topk_workspace_bytes(m, nq, 128, 16)
    assert need < more <= need + nq * 16 * 128 * 8 + 4096


def test_header_and_binding_agree():
    assert lib_max_k() == 128


def lib_max_k():
    from knowledgegraphembedding_amd import ops
    import re
    from pathlib import Path
    hdr = (Path(__file__).resolve().parents[1] / "include" / "kge_hip.h").read_text()
    v = int(re.search(r"#define KGE_TOPK_MAX_K (\d+)", hdr).group(1))
    assert ops.TOPK_MAX_K == v
    return v
