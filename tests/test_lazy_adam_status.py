"""The status every bad kge_train_step_lazy call returns, one row per host-side
check in the order the checks run (no device work: each row returns before any
launch; the pointers are host addresses the library never dereferences).  The
lazy step goes through the training family's checks (tests/test_capi_status.py)
with its own refusals — regulariser, wide rows — behind the optimizer
descriptor's and before the alignment, weight, modulus and workspace checks;
where two checks could both fire, the row shows which wins.
"""
import ctypes as C

import pytest

from knowledgegraphembedding_amd import _lib

OK, MODEL, MODE, SHAPE, ARG, WORKSPACE, DIM, ABI = range(8)

_RAW = C.create_string_buffer(8192 + 128)
_BASE = (C.addressof(_RAW) + 127) & ~127
ENT, REL, MOD, P, P2 = _BASE, _BASE + 1024, _BASE + 2048, _BASE + 3072, _BASE + 4096
ODD = P + 4          # 4-byte but not 16-byte aligned
AMPLE = 1 << 40
SHORT = "short"      # one byte under kge_train_lazy_workspace_bytes
DENSE = "dense"      # exactly kge_train_workspace_bytes: enough for the dense step only
NULL = None


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


PROTATE = dict(model=4, entity_dim=16, relation_dim=16)
BAD_ABI = dict(struct_size=C.sizeof(_lib.ModelDesc) - 8)
WIDE = dict(entity_dim=8192, relation_dim=4096)  # RotatE rows whose halves hold 4096 floats: kge_wide.inc's geometry
WIDE_T = dict(model=0, entity_dim=4096, relation_dim=4096)  # a 4096-float TransE row: the same


def _adam(**over):
    a = _lib.AdamDesc()
    for t, p in ((a.entity, ENT), (a.relation, REL)):
        t.param, t.exp_avg, t.exp_avg_sq, t.step_size, t.bias_correction2_sqrt = p, P, P2, 1e-3, 1.0
    a.beta1, a.beta2, a.eps, a.write_grad = 0.9, 0.999, 1e-8, 1
    for k, v in over.items():
        t, _, f = k.partition("_")
        setattr(getattr(a, t), f, v)
    return a


PARAMS = ("m", "mode", "pos", "neg", "batch", "nneg", "sub_w", "wsum", "uni_weight", "uni_batch", "adversarial",
          "adv_T", "reg", "adam", "ge", "gr", "gm", "losses", "ws", "ws_bytes", "err", "stream")
VALID = dict(m={}, mode=2, pos=P, neg=P, batch=4, nneg=8, sub_w=P, wsum=NULL, uni_weight=0, uni_batch=0,
             adversarial=1, adv_T=1.0, reg=0.0, adam={}, ge=P, gr=P2, gm=P, losses=P, ws=P, ws_bytes=AMPLE, err=P,
             stream=NULL)

# (overrides of the valid call, status), in the order the checks run
CASES = [
    # the entry's own check, before the model
    (dict(adam=NULL), ARG),
    (dict(adam=NULL, m=dict(model=7)), ARG),
    # the model, as every entry
    (dict(m=dict(null=True)), ARG),
    (dict(m=BAD_ABI), ABI),
    (dict(m=dict(model=7)), MODEL),
    (dict(m=BAD_ABI, mode=0, reg=0.1), ABI),
    # mode
    (dict(mode=0), MODE),
    (dict(mode=3), MODE),
    (dict(mode=0, reg=0.1), MODE),                           # the mode before the regulariser
    (dict(mode=0, m=WIDE), MODE),                            # ... and before the row width
    # outputs and batch: no entity gradient exists, so none is asked for
    (dict(ge=NULL, ws_bytes=SHORT), WORKSPACE),              # NULL grad_entity passes every check up to the workspace
    (dict(ge=ODD, ws_bytes=SHORT), WORKSPACE),               # ... and is not held to an alignment
    (dict(gr=NULL), ARG),
    (dict(losses=NULL), ARG),
    (dict(pos=NULL), ARG),
    (dict(neg=NULL), ARG),
    (dict(err=NULL), ARG),
    (dict(batch=0), ARG),
    (dict(nneg=0), ARG),
    (dict(gr=NULL, m=WIDE), ARG),                            # an output before the row width
    # the optimizer's descriptor: the entity tensor missing, or not the model's own
    (dict(adam=dict(entity_param=0)), ARG),
    (dict(adam=dict(entity_exp_avg=0)), ARG),
    (dict(adam=dict(entity_exp_avg_sq=0)), ARG),
    (dict(adam=dict(entity_param=P)), ARG),
    (dict(adam=dict(relation_exp_avg=0)), ARG),
    (dict(adam=dict(entity_exp_avg=0), m=WIDE), ARG),        # the descriptor before the row width
    # the lazy step's own refusals: regulariser, then wide rows
    (dict(reg=0.1), ARG),
    (dict(reg=-1e-9), ARG),
    (dict(reg=0.1, m=WIDE), ARG),                            # the regulariser before the row width
    (dict(reg=0.1, ws_bytes=SHORT), ARG),                    # ... and before the workspace
    (dict(m=WIDE), DIM),
    (dict(m=WIDE_T), DIM),
    (dict(m=dict(entity_dim=4096, relation_dim=2048), ws_bytes=SHORT), WORKSPACE),  # 2048-float halves are served
    (dict(m=WIDE, ws_bytes=0), DIM),                         # the row width before the workspace
    (dict(m=WIDE, gr=ODD), DIM),                             # ... and before the alignment
    (dict(m=WIDE, sub_w=NULL), DIM),                         # ... and before the weights
    # alignment, weights, modulus
    (dict(gr=ODD), ARG),
    (dict(adam=dict(entity_exp_avg=ODD)), ARG),
    (dict(sub_w=NULL), ARG),
    (dict(sub_w=NULL, uni_weight=1, ws_bytes=SHORT), WORKSPACE),
    (dict(m=PROTATE, gm=NULL), ARG),
    (dict(gm=NULL, ws_bytes=SHORT), WORKSPACE),              # only pRotatE has a modulus
    # the workspace, sized by kge_train_lazy_workspace_bytes; then the negatives' range
    (dict(ws=NULL), WORKSPACE),
    (dict(ws_bytes=0), WORKSPACE),
    (dict(ws_bytes=SHORT), WORKSPACE),
    (dict(ws_bytes=DENSE), WORKSPACE),                       # the dense step's size does not hold the row list
    (dict(nneg=8193, ws_bytes=SHORT), WORKSPACE),
    (dict(nneg=8193), DIM),
    (dict(m=PROTATE, ws_bytes=SHORT), WORKSPACE),
]


def _call(lib, over):
    v = dict(VALID)
    assert set(over) <= set(v), over
    v.update(over)
    v["m"] = _model(**v["m"])
    if isinstance(v["adam"], dict):
        v["adam"] = _adam(**v["adam"])
    if v["ws_bytes"] == SHORT:
        v["ws_bytes"] = lib.kge_train_lazy_workspace_bytes(C.byref(v["m"]), v["batch"], v["nneg"]) - 1
        assert v["ws_bytes"] > 0
    elif v["ws_bytes"] == DENSE:
        v["ws_bytes"] = lib.kge_train_workspace_bytes(C.byref(v["m"]), v["batch"], v["nneg"])
    args = [C.byref(v[k]) if isinstance(v[k], C.Structure) else v[k] for k in PARAMS]
    return lib.kge_train_step_lazy(*args)


_IDS = [f"{'-'.join(o) or 'valid'}-{s}" for o, s in CASES]
_IDS = [f"{i}#{_IDS[:k].count(i)}" if _IDS.count(i) > 1 else i for k, i in enumerate(_IDS)]


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_status(case):
    over, status = case
    lib = _lib.load()
    st = _call(lib, over)
    assert st < _lib.ERR_HIP_BASE, f"{over}: reached a launch (status {st})"
    assert st == status, f"{over}: {lib.kge_status_string(st).decode()}"


def test_signature_and_statuses_covered():
    assert len(PARAMS) == len(_lib.SIGNATURES["kge_train_step_lazy"][1])
    assert _lib.SIGNATURES["kge_train_step_lazy"] == _lib.SIGNATURES["kge_train_step"]
    assert {s for _, s in CASES} >= {MODEL, MODE, ARG, WORKSPACE, DIM, ABI}


@pytest.mark.parametrize("shape", [dict(), dict(nentity=2_000_000, entity_dim=400, relation_dim=200),
                                   dict(model=0, entity_dim=63, relation_dim=63, nentity=3000), PROTATE])
@pytest.mark.parametrize("batch,nneg", [(1, 1), (16, 8), (1024, 256)])
def test_lazy_workspace_covers_the_dense_one(shape, batch, nneg):
    lib = _lib.load()
    m = _model(**shape)
    dense = lib.kge_train_workspace_bytes(C.byref(m), batch, nneg)
    lazy = lib.kge_train_lazy_workspace_bytes(C.byref(m), batch, nneg)
    assert lazy >= dense > 0
    # what the lazy step adds is the row list — at most min(E, B·n + 2B) ids — and O(E)-free scratch:
    # nothing proportional to nentity × entity_dim
    places = min(m.nentity, batch * nneg + 2 * batch)
    assert lazy - dense >= 4 * places
    assert lazy - dense < 4 * places + (1 << 20)
