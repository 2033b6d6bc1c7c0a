"""The status every bad call returns, pinned per host-side check and in the
order the checks run (no device work: each row returns before any launch).

One row per argument check of the train family (train_impl behind its ten
entries), kge_score_backward, kge_ship_step and the ranking entries
(rank_impl); where two checks could both fire, a row shows which wins.  The
pointers are host addresses the library never dereferences before a launch.
"""
import ctypes as C

import pytest

from knowledgegraphembedding_amd import _lib

OK, MODEL, MODE, SHAPE, ARG, WORKSPACE, DIM, ABI = range(8)

_RAW = C.create_string_buffer(8192 + 128)
_BASE = (C.addressof(_RAW) + 127) & ~127
ENT, REL, MOD, P, P2 = _BASE, _BASE + 1024, _BASE + 2048, _BASE + 3072, _BASE + 4096
ODD = P + 4          # 4-byte but not 16-byte aligned
AMPLE = 1 << 40      # workspace_bytes no shape here needs
SHORT = "short"      # workspace_bytes one byte under what the call needs
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


ROTATE = {}
PROTATE = dict(model=4, entity_dim=16, relation_dim=16)
TRANSE6 = dict(model=0, entity_dim=6, relation_dim=6)  # single-float slots: no 16-byte alignment rule
BAD_ABI = dict(struct_size=C.sizeof(_lib.ModelDesc) - 8)


def _adam(**over):
    a = _lib.AdamDesc()
    for t, p in ((a.entity, ENT), (a.relation, REL)):
        t.param, t.exp_avg, t.exp_avg_sq, t.step_size, t.bias_correction2_sqrt = p, P, P2, 1e-3, 1.0
    a.beta1, a.beta2, a.eps, a.write_grad = 0.9, 0.999, 1e-8, 1
    for k, v in over.items():
        t, _, f = k.partition("_")
        setattr(getattr(a, t), f, v)
    return a


def _ship(**over):
    s = _lib.ShipDesc()
    f = dict(world=2, rank=0, own_begin=0, own_end=5, pos=P, neg=P, batch=4, nneg=8, subsampling_weight=P,
             weight_sum=P, uni_weight=0, adversarial=1, uni_batch=0, adversarial_temperature=1.0, regularization=0.0,
             q=P, qp=P, part=P, parts=P, scores=P, g=P, dq=P, pq=P, pstats=P, ent_contrib=P, rel_contrib=P,
             row_stats=P)
    f.update(over)
    for k, v in f.items():
        setattr(s, k, v)
    return s


# a valid call of each entry, by parameter name (the order is the header's)
_BATCH = [("pos", P), ("neg", P), ("batch", 4), ("nneg", 8)]
_WEIGHTS = [("sub_w", P), ("wsum", NULL), ("uni_weight", 0), ("uni_batch", 0)]
_ADV = [("adversarial", 1), ("adv_T", 1.0)]
_GRADS = [("ge", P), ("gr", P2), ("gm", P), ("losses", P)]
_WS = [("ws", P), ("ws_bytes", AMPLE), ("err", P), ("stream", NULL)]
_WEIGHTS_X = [("sub_w", P), ("wsum", P), ("uni_weight", 0), ("uni_batch", 0)]  # exchange stages: the caller's sum
_FROM_ROWS = ([("m", ROTATE), ("mode", 2)] + _BATCH + _WEIGHTS_X
              + [("reg", 0.0), ("g_in", P), ("dq_in", P), ("stats", P), ("adam", NULL)] + _GRADS + _WS)
_RANGE = [("e_begin", 0), ("e_end", 10)]
ENTRIES = {
    "kge_train_step_grads": [("m", ROTATE), ("mode", 2)] + _BATCH + _WEIGHTS + _ADV + [("reg", 0.0)] + _GRADS + _WS,
    "kge_train_step_grads_phased": ([("m", ROTATE), ("mode", 2)] + _BATCH + _WEIGHTS + _ADV + [("reg", 0.0)] + _GRADS
                                    + _WS + [("phases", 7)] + _RANGE),
    "kge_train_step": ([("m", ROTATE), ("mode", 2)] + _BATCH + _WEIGHTS + _ADV + [("reg", 0.0), ("adam", {})] + _GRADS
                       + _WS),
    "kge_train_rows_slice": ([("m", ROTATE), ("mode", 2)] + _BATCH + _WEIGHTS_X + _ADV
                             + [("g_out", P), ("dq_out", P), ("stats_out", P)] + _WS),
    "kge_train_step_from_rows": _FROM_ROWS,
    "kge_train_step_from_rows_csr": _FROM_ROWS,
    "kge_train_step_from_rows_range": _FROM_ROWS + _RANGE + [("csr_ready", 0), ("reg_relations", 1)],
    "kge_train_step_from_rows_phased": _FROM_ROWS + [("phases", 7)] + _RANGE + [("csr_ready", 0), ("reg_relations", 1)],
    "kge_train_csr": [("m", ROTATE), ("mode", 2)] + _BATCH + _WS,
    "kge_train_csr_range": [("m", ROTATE), ("mode", 2)] + _BATCH + _RANGE + _WS,
    "kge_score_backward": ([("m", ROTATE), ("mode", 2)] + _BATCH + [("grad_scores", P), ("ge", P), ("gr", P2), ("gm", P)]
                           + _WS),
    "kge_ship_step": ([("m", ROTATE), ("mode", 2), ("sh", {}), ("stage", 5), ("adam", NULL)] + _GRADS + _WS),
    "kge_rank_filtered": ([("m", ROTATE), ("mode", 2), ("queries", P), ("nq", 4), ("filt_off", P), ("filt_ids", P),
                           ("ranks", P), ("ties", P)] + _WS),
    "kge_rank_filtered_ex": ([("m", ROTATE), ("mode", 2), ("queries", P), ("nq", 4), ("filt_off", P), ("filt_ids", P),
                              ("ranks", P), ("ties", P), ("listed", NULL), ("path", 0)] + _WS),
    "kge_rank_filtered_both": ([("m", ROTATE), ("queries", P), ("nq", 4), ("filt_off", P), ("filt_ids", P),
                                ("filt_off_tail", P), ("filt_ids_tail", P), ("ranks", P), ("ties", P),
                                ("listed", NULL), ("path", 0)] + _WS),
    "kge_rank_sin_args": [("m", PROTATE), ("mode", 2), ("nq", 4), ("item_off", P), ("args", P)] + _WS,
    "kge_rank_finish_sin": ([("m", PROTATE), ("mode", 2), ("nq", 4), ("item_off", P), ("sins", P), ("ranks", P),
                             ("ties", P), ("listed", NULL)] + _WS),
}
LIST = _lib.RANK_STAGE_LIST
E_GRADS, E_PHASED, E_STEP, E_SLICE = ("kge_train_step_grads", "kge_train_step_grads_phased", "kge_train_step",
                                      "kge_train_rows_slice")
E_FROM, E_FROM_CSR, E_FROM_RANGE, E_FROM_PHASED = ("kge_train_step_from_rows", "kge_train_step_from_rows_csr",
                                                   "kge_train_step_from_rows_range", "kge_train_step_from_rows_phased")
E_CSR, E_CSR_RANGE, E_BWD, E_SHIP = "kge_train_csr", "kge_train_csr_range", "kge_score_backward", "kge_ship_step"
E_RANK, E_EX, E_BOTH, E_ARGS, E_FIN = ("kge_rank_filtered", "kge_rank_filtered_ex", "kge_rank_filtered_both",
                                       "kge_rank_sin_args", "kge_rank_finish_sin")
# a RotatE row of 4096 floats with 8192 negatives: the row pass's LDS passes 64 KiB
BIG_ROW = dict(entity_dim=4096, relation_dim=2048)

# (entry, overrides of the valid call, status), in the order the checks run
CASES = [
    # ---- train_impl: the model
    (E_GRADS, dict(m=dict(null=True)), ARG),
    (E_GRADS, dict(m=BAD_ABI), ABI),
    (E_GRADS, dict(m=dict(model=7)), MODEL),
    (E_GRADS, dict(m=dict(model=7), mode=0), MODEL),           # the model before the mode
    (E_GRADS, dict(m=dict(model=7, struct_size=0)), ABI),      # the layout before the model
    (E_GRADS, dict(m=dict(entity_embedding=0)), ARG),
    (E_GRADS, dict(m=dict(relation_embedding=0)), ARG),
    (E_GRADS, dict(m=dict(nentity=0)), ARG),
    (E_GRADS, dict(m=dict(nrelation=0)), ARG),
    (E_GRADS, dict(m=dict(nentity=1 << 31)), DIM),
    (E_GRADS, dict(m=dict(nrelation=1 << 30)), DIM),
    (E_GRADS, dict(m=dict(relation_dim=16)), SHAPE),
    (E_GRADS, dict(m=dict(relation_dim=16), mode=0), SHAPE),   # the shape before the mode
    (E_GRADS, dict(m=dict(model=2, entity_dim=6, relation_dim=6), mode=0), MODE),
    (E_GRADS, dict(m=dict(model=2, entity_dim=7, relation_dim=7)), SHAPE),
    (E_GRADS, dict(m=dict(PROTATE, modulus=0)), ARG),
    # ---- train_impl: mode, then the buffers each exchange stage needs
    (E_GRADS, dict(mode=0), MODE),
    (E_GRADS, dict(mode=3), MODE),
    (E_GRADS, dict(mode=0, ge=NULL), MODE),
    (E_GRADS, dict(ge=NULL), ARG),
    (E_GRADS, dict(gr=NULL), ARG),
    (E_GRADS, dict(losses=NULL), ARG),
    (E_GRADS, dict(ge=NULL, ws_bytes=SHORT), ARG),             # an argument before the workspace
    (E_SLICE, dict(g_out=NULL), ARG),
    (E_SLICE, dict(dq_out=NULL), ARG),
    (E_SLICE, dict(stats_out=NULL), ARG),
    (E_SLICE, dict(mode=0, g_out=NULL), MODE),
    (E_FROM, dict(g_in=NULL), ARG),
    (E_FROM, dict(dq_in=NULL), ARG),
    (E_FROM, dict(stats=NULL), ARG),
    (E_FROM, dict(ge=NULL), ARG),
    (E_FROM, dict(losses=NULL), ARG),
    (E_FROM_CSR, dict(g_in=NULL), ARG),
    (E_FROM_CSR, dict(gr=NULL), ARG),
    (E_GRADS, dict(pos=NULL), ARG),
    (E_GRADS, dict(neg=NULL), ARG),
    (E_GRADS, dict(err=NULL), ARG),
    (E_GRADS, dict(batch=0), ARG),
    (E_GRADS, dict(nneg=0), ARG),
    (E_CSR, dict(pos=NULL), ARG),                              # (the CSR alone needs no gradient buffers)
    (E_CSR, dict(batch=0), ARG),
    (E_CSR, dict(mode=0), MODE),
    (E_SLICE, dict(nneg=0), ARG),
    # ---- train_impl: the fused Adam's descriptor
    (E_STEP, dict(adam=NULL), ARG),
    (E_STEP, dict(adam=NULL, m=dict(model=7)), ARG),           # the entry's own check before the model
    (E_STEP, dict(m=dict(model=7)), MODEL),
    (E_STEP, dict(adam=dict(entity_exp_avg=0)), ARG),
    (E_STEP, dict(adam=dict(entity_exp_avg_sq=0)), ARG),
    (E_STEP, dict(adam=dict(relation_param=0)), ARG),
    (E_STEP, dict(adam=dict(relation_exp_avg=0)), ARG),
    (E_STEP, dict(adam=dict(entity_param=P)), ARG),            # not the model's own table
    (E_STEP, dict(adam=dict(relation_param=P)), ARG),
    (E_STEP, dict(m=PROTATE, adam=dict(modulus_param=P)), ARG),
    (E_FROM, dict(adam=dict(entity_exp_avg=0)), ARG),
    # ---- train_impl: 16-byte streams with float4 slots
    (E_GRADS, dict(ge=ODD), ARG),
    (E_GRADS, dict(gr=ODD), ARG),
    (E_GRADS, dict(m=TRANSE6, ge=ODD, gr=ODD, ws_bytes=SHORT), WORKSPACE),  # single-float slots take any alignment
    (E_STEP, dict(adam=dict(entity_exp_avg=ODD)), ARG),
    (E_STEP, dict(adam=dict(relation_exp_avg_sq=ODD)), ARG),
    # ---- train_impl: weights, modulus gradient, the caller's weight sum
    (E_GRADS, dict(sub_w=NULL), ARG),
    (E_GRADS, dict(sub_w=NULL, uni_weight=1, ws_bytes=SHORT), WORKSPACE),
    (E_GRADS, dict(m=PROTATE, gm=NULL), ARG),
    (E_GRADS, dict(gm=NULL, ws_bytes=SHORT), WORKSPACE),       # only pRotatE has a modulus
    (E_SLICE, dict(m=PROTATE, ws_bytes=SHORT), WORKSPACE),     # the rows-only stage writes no modulus gradient
    (E_FROM, dict(m=PROTATE, gm=NULL), ARG),
    (E_FROM, dict(wsum=NULL), ARG),
    (E_SLICE, dict(wsum=NULL), ARG),
    (E_FROM, dict(wsum=NULL, uni_weight=1, ws_bytes=SHORT), WORKSPACE),
    (E_GRADS, dict(wsum=NULL, ws_bytes=SHORT), WORKSPACE),     # the single call sums the weights itself
    # ---- train_impl: workspace, then the sizes, phases and entity range
    (E_GRADS, dict(ws=NULL), WORKSPACE),
    (E_GRADS, dict(ws_bytes=SHORT), WORKSPACE),
    (E_GRADS, dict(ws_bytes=0), WORKSPACE),
    (E_GRADS, dict(nneg=8193, ws_bytes=SHORT), WORKSPACE),     # the workspace before the negatives' range
    (E_GRADS, dict(nneg=8193), DIM),
    (E_CSR, dict(ws_bytes=SHORT), WORKSPACE),
    (E_CSR, dict(nneg=8193), DIM),
    (E_FROM_CSR, dict(ws_bytes=SHORT), WORKSPACE),
    (E_STEP, dict(ws_bytes=SHORT), WORKSPACE),
    (E_PHASED, dict(nneg=8193, phases=0), DIM),                # the negatives' range before the phases
    (E_PHASED, dict(phases=0), ARG),
    (E_PHASED, dict(phases=8), ARG),
    (E_PHASED, dict(phases=0, ws_bytes=SHORT), WORKSPACE),
    (E_PHASED, dict(e_begin=-1), ARG),
    (E_PHASED, dict(e_begin=6, e_end=5), ARG),
    (E_PHASED, dict(e_end=11), ARG),
    (E_PHASED, dict(e_end=11, ws_bytes=SHORT), WORKSPACE),
    (E_PHASED, dict(e_end=11, nneg=8193), DIM),
    # ---- the range entries check their range first, before the model
    (E_FROM_RANGE, dict(e_begin=-1), ARG),
    (E_FROM_RANGE, dict(e_begin=6, e_end=5), ARG),
    (E_FROM_RANGE, dict(e_end=11), ARG),
    (E_FROM_RANGE, dict(e_end=11, m=BAD_ABI), ARG),
    (E_FROM_RANGE, dict(m=BAD_ABI), ABI),
    (E_FROM_RANGE, dict(m=dict(null=True)), ARG),
    (E_FROM_RANGE, dict(m=dict(null=True), e_end=0), ARG),
    (E_FROM_RANGE, dict(ws_bytes=SHORT), WORKSPACE),
    (E_FROM_PHASED, dict(phases=0), ARG),
    (E_FROM_PHASED, dict(phases=8, m=BAD_ABI), ARG),
    (E_FROM_PHASED, dict(e_end=11, mode=0), ARG),
    (E_FROM_PHASED, dict(mode=0), MODE),
    (E_FROM_PHASED, dict(g_in=NULL), ARG),
    (E_FROM_PHASED, dict(ws_bytes=SHORT), WORKSPACE),
    (E_CSR_RANGE, dict(m=dict(null=True)), ARG),
    (E_CSR_RANGE, dict(e_begin=-1), ARG),
    (E_CSR_RANGE, dict(e_end=11, m=dict(model=7)), ARG),
    (E_CSR_RANGE, dict(m=dict(model=7)), MODEL),
    (E_CSR_RANGE, dict(ws_bytes=SHORT), WORKSPACE),
    # ---- run_grad: the row pass's LDS, before anything is queued
    (E_GRADS, dict(m=BIG_ROW, nneg=8192), DIM),
    (E_STEP, dict(m=BIG_ROW, nneg=8192), DIM),
    (E_SLICE, dict(m=BIG_ROW, nneg=8192), DIM),
    # ---- kge_score_backward
    (E_BWD, dict(m=dict(null=True)), ARG),
    (E_BWD, dict(m=BAD_ABI), ABI),
    (E_BWD, dict(mode=9), MODE),
    (E_BWD, dict(mode=9, ws_bytes=SHORT), MODE),
    (E_BWD, dict(pos=NULL), ARG),
    (E_BWD, dict(grad_scores=NULL), ARG),
    (E_BWD, dict(ge=NULL), ARG),
    (E_BWD, dict(gr=NULL), ARG),
    (E_BWD, dict(err=NULL), ARG),
    (E_BWD, dict(batch=0), ARG),
    (E_BWD, dict(nneg=0), ARG),
    (E_BWD, dict(ge=ODD), ARG),
    (E_BWD, dict(gr=ODD), ARG),
    (E_BWD, dict(m=TRANSE6, ge=ODD, ws_bytes=SHORT), WORKSPACE),
    (E_BWD, dict(mode=0, nneg=2), ARG),                        # 'single' scores one candidate per row
    (E_BWD, dict(mode=0, nneg=2, ws_bytes=SHORT), ARG),
    (E_BWD, dict(neg=NULL), ARG),
    (E_BWD, dict(mode=0, nneg=1, neg=NULL, ws_bytes=SHORT), WORKSPACE),  # 'single' reads no negatives
    (E_BWD, dict(ws=NULL), WORKSPACE),
    (E_BWD, dict(ws_bytes=SHORT), WORKSPACE),
    (E_BWD, dict(m=PROTATE, gm=NULL, ws_bytes=SHORT), WORKSPACE),  # the modulus gradient is optional here
    # ---- kge_ship_step
    (E_SHIP, dict(m=dict(null=True)), ARG),
    (E_SHIP, dict(m=dict(model=7), mode=0), MODEL),
    (E_SHIP, dict(mode=0), MODE),
    (E_SHIP, dict(mode=0, sh=NULL), MODE),
    (E_SHIP, dict(sh=NULL), ARG),
    (E_SHIP, dict(stage=0), ARG),
    (E_SHIP, dict(stage=6), ARG),
    (E_SHIP, dict(err=NULL), ARG),
    (E_SHIP, dict(sh=dict(pos=0)), ARG),
    (E_SHIP, dict(sh=dict(neg=0)), ARG),
    (E_SHIP, dict(sh=dict(batch=0)), ARG),
    (E_SHIP, dict(sh=dict(nneg=0)), ARG),
    (E_SHIP, dict(sh=dict(nneg=8193)), ARG),                   # (an argument error here, not KGE_ERR_DIM)
    (E_SHIP, dict(sh=dict(nneg=8193), ws_bytes=SHORT), ARG),
    (E_SHIP, dict(sh=dict(world=0)), ARG),
    (E_SHIP, dict(sh=dict(world=4097)), ARG),
    (E_SHIP, dict(sh=dict(rank=-1)), ARG),
    (E_SHIP, dict(sh=dict(rank=2)), ARG),
    (E_SHIP, dict(sh=dict(own_begin=-1)), ARG),
    (E_SHIP, dict(sh=dict(own_begin=6)), ARG),
    (E_SHIP, dict(sh=dict(own_end=11)), ARG),
    (E_SHIP, dict(sh=dict(subsampling_weight=0)), ARG),
    (E_SHIP, dict(sh=dict(weight_sum=0)), ARG),
    (E_SHIP, dict(sh=dict(subsampling_weight=0, weight_sum=0, uni_weight=1), ws_bytes=SHORT), WORKSPACE),
    *[(E_SHIP, dict(sh={f: 0}), ARG) for f in ("q", "part", "parts", "scores", "g", "dq", "pstats", "ent_contrib",
                                                "rel_contrib", "row_stats")],
    (E_SHIP, dict(mode=1, sh=dict(qp=0)), ARG),                # head-batch ships the positive's q too
    (E_SHIP, dict(mode=1, sh=dict(pq=0)), ARG),
    (E_SHIP, dict(sh=dict(qp=0, pq=0), ws_bytes=SHORT), WORKSPACE),
    (E_SHIP, dict(stage=4, gr=NULL), ARG),
    (E_SHIP, dict(stage=5, gr=NULL), ARG),
    (E_SHIP, dict(stage=3, gr=NULL, ws_bytes=SHORT), WORKSPACE),
    (E_SHIP, dict(stage=5, ge=NULL), ARG),
    (E_SHIP, dict(stage=5, losses=NULL), ARG),
    (E_SHIP, dict(stage=5, m=PROTATE, gm=NULL), ARG),
    (E_SHIP, dict(stage=4, ge=NULL, losses=NULL, ws_bytes=SHORT), WORKSPACE),
    (E_SHIP, dict(stage=4, m=PROTATE, gm=NULL, ws_bytes=SHORT), WORKSPACE),
    (E_SHIP, dict(adam=dict(entity_exp_avg=0)), ARG),
    (E_SHIP, dict(adam=dict(entity_param=P)), ARG),
    (E_SHIP, dict(adam=dict(relation_param=0, relation_exp_avg=0), ws_bytes=SHORT), WORKSPACE),  # entity table only
    (E_SHIP, dict(gr=ODD), ARG),
    (E_SHIP, dict(adam=dict(entity_exp_avg_sq=ODD)), ARG),
    (E_SHIP, dict(ws=NULL), WORKSPACE),
    (E_SHIP, dict(ws_bytes=SHORT), WORKSPACE),
    *[(E_SHIP, dict(stage=k, ws_bytes=SHORT), WORKSPACE) for k in (1, 2, 3, 4)],
    # ---- rank_impl
    (E_EX, dict(m=dict(null=True)), ARG),
    (E_EX, dict(m=BAD_ABI), ABI),
    (E_EX, dict(m=dict(relation_dim=16), mode=0), SHAPE),
    (E_EX, dict(mode=0), MODE),
    (E_EX, dict(mode=0, err=NULL), MODE),
    (E_RANK, dict(mode=3), MODE),
    (E_EX, dict(err=NULL), ARG),
    (E_EX, dict(nq=-1), ARG),
    (E_BOTH, dict(err=NULL), ARG),
    (E_BOTH, dict(filt_off_tail=NULL), ARG),
    (E_EX, dict(queries=NULL), ARG),
    (E_EX, dict(filt_off=NULL), ARG),
    (E_RANK, dict(queries=NULL), ARG),
    (E_BOTH, dict(queries=NULL), ARG),
    (E_EX, dict(ranks=NULL), ARG),
    (E_RANK, dict(ranks=NULL), ARG),
    (E_BOTH, dict(ranks=NULL), ARG),
    (E_FIN, dict(ranks=NULL), ARG),
    (E_EX, dict(m=PROTATE, path=LIST, listed=NULL), ARG),
    (E_EX, dict(m=PROTATE, path=LIST, listed=P, ranks=NULL, ws_bytes=SHORT), WORKSPACE),  # the list stage writes no ranks
    (E_ARGS, dict(item_off=NULL), ARG),
    (E_ARGS, dict(args=NULL), ARG),
    (E_FIN, dict(item_off=NULL), ARG),
    (E_FIN, dict(sins=NULL), ARG),
    (E_EX, dict(path=LIST, listed=P), MODEL),                  # the three-call form is pRotatE's
    (E_ARGS, dict(m=ROTATE), MODEL),
    (E_FIN, dict(m=ROTATE), MODEL),
    (E_ARGS, dict(m=ROTATE, item_off=NULL), ARG),              # the stage's buffers before its model
    (E_FIN, dict(m=ROTATE, sins=NULL), ARG),
    (E_ARGS, dict(m=ROTATE, ws_bytes=SHORT), MODEL),
    (E_EX, dict(path=5), ARG),
    (E_EX, dict(path=-1), ARG),
    (E_EX, dict(path=5, nq=0), ARG),                           # the path before the empty call
    (E_EX, dict(nq=0, ws=NULL), OK),                           # an empty call: nothing to check further, no launch
    (E_BOTH, dict(nq=0, ws_bytes=0), OK),
    (E_EX, dict(nq=0, ranks=NULL), ARG),
    (E_EX, dict(nq=65536), DIM),
    (E_EX, dict(nq=65536, path=1), DIM),                       # the query count before the path's fit
    (E_EX, dict(nq=65536, ws=NULL), DIM),
    (E_EX, dict(path=1), ARG),                                 # the split-bf16 tile is DistMult's and ComplEx's
    (E_EX, dict(path=4), ARG),
    (E_EX, dict(m=TRANSE6, path=2), ARG),                      # the register tile needs K % 4 == 0
    (E_EX, dict(path=1, ws_bytes=SHORT), ARG),
    (E_EX, dict(m=dict(relation_trig=ODD)), ARG),
    (E_EX, dict(m=dict(relation_trig=ODD), ws_bytes=SHORT), ARG),
    (E_BOTH, dict(m=dict(relation_trig=ODD)), ARG),
    (E_EX, dict(ws=NULL), WORKSPACE),
    (E_EX, dict(ws_bytes=SHORT), WORKSPACE),
    (E_RANK, dict(ws_bytes=SHORT), WORKSPACE),
    (E_BOTH, dict(ws_bytes=SHORT), WORKSPACE),                 # (sized for both directions' queries)
    (E_ARGS, dict(ws_bytes=SHORT), WORKSPACE),
    (E_FIN, dict(ws_bytes=SHORT), WORKSPACE),
    (E_BOTH, dict(path=LIST), ARG),                            # the three-call form is per direction
    (E_BOTH, dict(path=LIST, m=BAD_ABI), ARG),
    (E_BOTH, dict(m=BAD_ABI), ABI),
]


def _short(lib, entry, v):
    m = C.byref(v["m"])
    if entry.startswith("kge_rank"):
        return lib.kge_rank_workspace_bytes(m, v["nq"] * (2 if entry == E_BOTH else 1)) - 1
    if entry == E_SHIP:
        return lib.kge_train_workspace_bytes(m, v["sh"].batch, v["sh"].nneg) - 1
    return lib.kge_train_workspace_bytes(m, v["batch"], v["nneg"]) - 1


def _call(lib, entry, over):
    v = dict(ENTRIES[entry])
    assert set(over) <= set(v), (entry, over)
    v.update(over)
    keep = []  # the descriptors stay alive over the call
    v["m"] = _model(**v["m"])
    if isinstance(v.get("adam"), dict):
        v["adam"] = _adam(**v["adam"])
    if isinstance(v.get("sh"), dict):
        v["sh"] = _ship(**v["sh"])
    if v["ws_bytes"] == SHORT:
        v["ws_bytes"] = _short(lib, entry, v)
        assert v["ws_bytes"] > 0
    args = []
    for name, _ in ENTRIES[entry]:
        x = v[name]
        if isinstance(x, C.Structure):
            keep.append(x)
            x = C.byref(x)
        args.append(x)
    return getattr(lib, entry)(*args)


def _id(case):
    entry, over, status = case
    return f"{entry[4:]}-{'-'.join(over) or 'valid'}-{status}"


_IDS = [_id(c) for c in CASES]
_IDS = [f"{i}#{_IDS[:k].count(i)}" if _IDS.count(i) > 1 else i for k, i in enumerate(_IDS)]


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_status(case):
    entry, over, status = case
    st = _call(_lib.load(), entry, over)
    assert st < _lib.ERR_HIP_BASE, f"{entry} {over}: reached a launch (status {st})"
    assert st == status, f"{entry} {over}: {_lib.load().kge_status_string(st).decode()}"


def test_every_train_entry_and_status_appears():
    train = {e for e in ENTRIES if e.startswith("kge_train")}
    assert len(train) == 10 and train <= {c[0] for c in CASES}
    assert set(ENTRIES) <= set(_lib.SIGNATURES)
    assert {c[2] for c in CASES} == {OK, MODEL, MODE, SHAPE, ARG, WORKSPACE, DIM, ABI}
    for entry, params in ENTRIES.items():
        assert len(params) == len(_lib.SIGNATURES[entry][1]), entry
