"""The status every bad kge_train_step_adagrad call returns, one row per host-side
check in the order the checks run (no device work: each row returns before any
launch; the pointers are host addresses the library never dereferences).  The
order is kge_train_step_lazy's (tests/test_lazy_adam_status.py) with the Adagrad
descriptor's checks where the Adam descriptor's stand; where two checks could
both fire, the row shows which wins.  Also kge_adagrad_step's argument errors,
the workspace query and the ABI version, which this feature leaves at "0.5".
"""
import ctypes as C
import re
from pathlib import Path

import pytest

from knowledgegraphembedding_amd import _lib

OK, MODEL, MODE, SHAPE, ARG, WORKSPACE, DIM, ABI = range(8)

_RAW = C.create_string_buffer(8192 + 128)
_BASE = (C.addressof(_RAW) + 127) & ~127
ENT, REL, MOD, P, P2 = _BASE, _BASE + 1024, _BASE + 2048, _BASE + 3072, _BASE + 4096
ODD = P + 4          # 4-byte but not 16-byte aligned
AMPLE = 1 << 40
SHORT = "short"      # one byte under kge_train_adagrad_workspace_bytes
DENSE = "dense"      # exactly kge_train_workspace_bytes: enough for the dense step only
NULL = None
NAN, INF = float("nan"), float("inf")


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
WIDE = dict(entity_dim=8192, relation_dim=4096)  # RotatE rows whose halves hold 4096 floats
WIDE_T = dict(model=0, entity_dim=4096, relation_dim=4096)
UNALIGNED_TABLE = dict(entity_embedding=ENT + 4)  # single-float slots: nothing needs more than float alignment


def _opt(**over):
    """A valid descriptor; overrides are desc fields (lr=...) or tensor_field (entity_state_sum=...)."""
    a = _lib.AdagradDesc()
    for t, p in ((a.entity, ENT), (a.relation, REL)):
        t.param, t.state_sum = p, P
    a.lr, a.eps, a.entity_rowwise, a.write_grad = 1e-2, 1e-10, 0, 1
    for k, v in over.items():
        t, _, f = k.partition("_")
        if t in ("entity", "relation", "modulus") and f in ("param", "state_sum"):
            setattr(getattr(a, t), f, v)
        else:
            setattr(a, k, v)
    return a


PARAMS = ("m", "mode", "pos", "neg", "batch", "nneg", "sub_w", "wsum", "uni_weight", "uni_batch", "adversarial",
          "adv_T", "reg", "opt", "ge", "gr", "gm", "losses", "ws", "ws_bytes", "err", "stream")
VALID = dict(m={}, mode=2, pos=P, neg=P, batch=4, nneg=8, sub_w=P, wsum=NULL, uni_weight=0, uni_batch=0,
             adversarial=1, adv_T=1.0, reg=0.0, opt={}, ge=P, gr=P2, gm=P, losses=P, ws=P, ws_bytes=AMPLE, err=P,
             stream=NULL)
BAD_DESC_ABI = dict(struct_size=C.sizeof(_lib.AdagradDesc) - 4)

# (overrides of the valid call, status), in the order the checks run
CASES = [
    # the entry's own check, before the model
    (dict(opt=NULL), ARG),
    (dict(opt=NULL, m=dict(model=7)), ARG),
    # the model, as every entry
    (dict(m=dict(null=True)), ARG),
    (dict(m=BAD_ABI), ABI),
    (dict(m=dict(model=7)), MODEL),
    (dict(m=dict(model=7), opt=BAD_DESC_ABI), MODEL),         # the model before the descriptor
    # mode
    (dict(mode=0), MODE),
    (dict(mode=3), MODE),
    (dict(mode=0, opt=BAD_DESC_ABI), MODE),                   # the mode before the descriptor
    (dict(mode=0, reg=0.1), MODE),
    # outputs and batch: no entity gradient exists, so none is asked for
    (dict(ge=NULL, ws_bytes=SHORT), WORKSPACE),               # NULL grad_entity passes every check up to the workspace
    (dict(ge=ODD, ws_bytes=SHORT), WORKSPACE),                # ... and is not held to an alignment
    (dict(gr=NULL), ARG),
    (dict(losses=NULL), ARG),
    (dict(pos=NULL), ARG),
    (dict(neg=NULL), ARG),
    (dict(err=NULL), ARG),
    (dict(batch=0), ARG),
    (dict(nneg=0), ARG),
    (dict(gr=NULL, opt=BAD_DESC_ABI), ARG),                   # an output before the descriptor
    # the descriptor: its size first
    (dict(opt=BAD_DESC_ABI), ABI),
    (dict(opt=dict(struct_size=0)), ABI),
    (dict(opt=dict(struct_size=0, entity_param=0, eps=0.0)), ABI),   # the size before the descriptor's fields
    # ... then a tensor missing or not the model's own
    (dict(opt=dict(entity_param=0)), ARG),
    (dict(opt=dict(entity_state_sum=0)), ARG),
    (dict(opt=dict(relation_param=0)), ARG),
    (dict(opt=dict(relation_state_sum=0)), ARG),
    (dict(opt=dict(entity_param=P)), ARG),
    (dict(opt=dict(relation_param=P)), ARG),
    (dict(m=PROTATE, opt=dict(modulus_param=P, modulus_state_sum=P)), ARG),   # not the model's modulus
    (dict(m=PROTATE, opt=dict(modulus_param=MOD)), ARG),                       # its state missing
    (dict(m=PROTATE, opt=dict(modulus_param=MOD, modulus_state_sum=P), ws_bytes=SHORT), WORKSPACE),
    (dict(m=PROTATE, ws_bytes=SHORT), WORKSPACE),             # modulus.param NULL leaves the modulus alone
    # ... then eps, lr, the kind
    (dict(opt=dict(eps=0.0)), ARG),
    (dict(opt=dict(eps=-1e-10)), ARG),
    (dict(opt=dict(eps=NAN)), ARG),
    (dict(opt=dict(lr=-1e-3)), ARG),
    (dict(opt=dict(lr=NAN)), ARG),
    (dict(opt=dict(lr=INF)), ARG),
    (dict(opt=dict(lr=0.0), ws_bytes=SHORT), WORKSPACE),      # lr = 0 is served
    (dict(opt=dict(entity_rowwise=2)), ARG),
    (dict(opt=dict(entity_rowwise=-1)), ARG),
    (dict(opt=dict(entity_rowwise=1), ws_bytes=SHORT), WORKSPACE),
    (dict(opt=dict(eps=0.0), m=WIDE), ARG),                   # the descriptor before the row width
    # the lazy step's refusals: regulariser, then wide rows
    (dict(reg=0.1), ARG),
    (dict(reg=-1e-9), ARG),
    (dict(reg=0.1, m=WIDE), ARG),                             # the regulariser before the row width
    (dict(reg=0.1, ws_bytes=SHORT), ARG),                     # ... and before the workspace
    (dict(m=WIDE), DIM),
    (dict(m=WIDE_T), DIM),
    (dict(m=WIDE, opt=dict(entity_rowwise=1)), DIM),
    (dict(m=dict(entity_dim=4096, relation_dim=2048), ws_bytes=SHORT), WORKSPACE),  # 2048-float halves are served
    (dict(m=WIDE, ws_bytes=0), DIM),                          # the row width before the workspace
    (dict(m=WIDE, gr=ODD), DIM),                              # ... and before the alignment
    (dict(m=WIDE, sub_w=NULL), DIM),                          # ... and before the weights
    # alignment (16-byte slots): the gradient stream and the streamed state
    (dict(gr=ODD), ARG),
    (dict(opt=dict(entity_state_sum=ODD)), ARG),
    (dict(opt=dict(relation_state_sum=ODD)), ARG),
    (dict(opt=dict(entity_state_sum=ODD, entity_rowwise=1), ws_bytes=SHORT), WORKSPACE),  # [nentity]: float alignment
    (dict(opt=dict(relation_state_sum=ODD, entity_rowwise=1)), ARG),             # the relation state is streamed still
    (dict(m=UNALIGNED_TABLE, opt=dict(entity_param=ENT + 4, entity_state_sum=ODD), gr=ODD, ws_bytes=SHORT), WORKSPACE),
    # weights, modulus
    (dict(sub_w=NULL), ARG),
    (dict(sub_w=NULL, uni_weight=1, ws_bytes=SHORT), WORKSPACE),
    (dict(m=PROTATE, gm=NULL), ARG),
    (dict(gm=NULL, ws_bytes=SHORT), WORKSPACE),               # only pRotatE has a modulus
    # the workspace, sized by kge_train_adagrad_workspace_bytes; then the negatives' range
    (dict(ws=NULL), WORKSPACE),
    (dict(ws_bytes=0), WORKSPACE),
    (dict(ws_bytes=SHORT), WORKSPACE),
    (dict(ws_bytes=DENSE), WORKSPACE),                        # the dense step's size does not hold the row list
    (dict(nneg=8193, ws_bytes=SHORT), WORKSPACE),
    (dict(nneg=8193), DIM),
]


def _call(lib, over):
    v = dict(VALID)
    assert set(over) <= set(v), over
    v.update(over)
    v["m"] = _model(**v["m"])
    if isinstance(v["opt"], dict):
        v["opt"] = _opt(**v["opt"])
    if v["ws_bytes"] == SHORT:
        v["ws_bytes"] = lib.kge_train_adagrad_workspace_bytes(C.byref(v["m"]), v["batch"], v["nneg"]) - 1
        assert v["ws_bytes"] > 0
    elif v["ws_bytes"] == DENSE:
        v["ws_bytes"] = lib.kge_train_workspace_bytes(C.byref(v["m"]), v["batch"], v["nneg"])
    args = [C.byref(v[k]) if isinstance(v[k], C.Structure) else v[k] for k in PARAMS]
    return lib.kge_train_step_adagrad(*args)


def _ids(cases):
    ids = []
    for o, s in cases:
        parts = [k if not isinstance(v, dict) else k + "." + ".".join(v) for k, v in o.items()]
        ids.append(f"{'-'.join(parts) or 'valid'}-{s}")
    return [f"{i}#{ids[:k].count(i)}" if ids.count(i) > 1 else i for k, i in enumerate(ids)]


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_status(case):
    over, status = case
    lib = _lib.load()
    st = _call(lib, over)
    assert st < _lib.ERR_HIP_BASE, f"{over}: reached a launch (status {st})"
    assert st == status, f"{over}: {lib.kge_status_string(st).decode()}"


def test_signature_and_statuses_covered():
    sig, lazy = _lib.SIGNATURES["kge_train_step_adagrad"], _lib.SIGNATURES["kge_train_step_lazy"]
    assert len(PARAMS) == len(sig[1])
    k = PARAMS.index("opt")
    assert sig[0] == lazy[0] and sig[1][:k] == lazy[1][:k] and sig[1][k + 1:] == lazy[1][k + 1:]
    assert sig[1][k] == C.POINTER(_lib.AdagradDesc)
    assert {s for _, s in CASES} >= {MODEL, MODE, ARG, WORKSPACE, DIM, ABI}


def test_descriptor_layout():
    """struct kge_adagrad_desc as include/kge_hip.h declares it (LP64)."""
    d = _lib.AdagradDesc
    assert [(f, getattr(d, f).offset) for f in ("entity", "relation", "modulus", "lr", "eps", "entity_rowwise",
                                                "write_grad", "struct_size")] == \
        [("entity", 0), ("relation", 16), ("modulus", 32), ("lr", 48), ("eps", 52), ("entity_rowwise", 56),
         ("write_grad", 60), ("struct_size", 64)]
    assert C.sizeof(d) == 72 and _lib.AdagradDesc().struct_size == 72


@pytest.mark.parametrize("shape", [dict(), dict(nentity=2_000_000, entity_dim=400, relation_dim=200),
                                   dict(model=0, entity_dim=63, relation_dim=63, nentity=3000), PROTATE])
@pytest.mark.parametrize("batch,nneg", [(1, 1), (16, 8), (1024, 256)])
def test_workspace_is_the_lazy_steps(shape, batch, nneg):
    lib = _lib.load()
    m = _model(**shape)
    assert lib.kge_train_adagrad_workspace_bytes(C.byref(m), batch, nneg) == \
        lib.kge_train_lazy_workspace_bytes(C.byref(m), batch, nneg) > 0


# (overrides, status) of kge_adagrad_step(param, grad, state_sum, numel, lr, eps, stream), in the checks' order
STEP_VALID = dict(param=P, grad=P2, state_sum=ENT, numel=8, lr=1e-2, eps=1e-10, stream=NULL)
STEP_CASES = [
    (dict(param=NULL), ARG),
    (dict(grad=NULL), ARG),
    (dict(state_sum=NULL), ARG),
    (dict(numel=-1), ARG),
    (dict(param=NULL, numel=0), ARG),         # a NULL array before the empty update
    (dict(eps=0.0), ARG),
    (dict(eps=NAN), ARG),
    (dict(lr=-1.0), ARG),
    (dict(lr=INF), ARG),
    (dict(eps=0.0, numel=0), ARG),            # the rule's parameters before the empty update
    (dict(numel=0), OK),
    (dict(numel=0, param=ODD), OK),           # ... which is not held to an alignment
    (dict(param=ODD), ARG),
    (dict(grad=ODD), ARG),
    (dict(state_sum=ODD), ARG),
]


@pytest.mark.parametrize("case", STEP_CASES, ids=_ids(STEP_CASES))
def test_adagrad_step_status(case):
    over, status = case
    v = dict(STEP_VALID)
    v.update(over)
    st = _lib.load().kge_adagrad_step(*[v[k] for k in STEP_VALID])
    assert st == status


def test_abi_version_is_unchanged():
    header = (Path(__file__).resolve().parents[1] / "include" / "kge_hip.h").read_text()
    assert re.search(r'#define\s+KGE_ABI_VERSION\s+"0\.5"', header)
    assert _lib.ABI_VERSION == "0.5" and _lib.load().kge_version().decode().split()[1] == "0.5"
    for name in ("kge_train_adagrad_workspace_bytes", "kge_train_step_adagrad", "kge_adagrad_step"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES
