"""The per-call host switches that select another stream schedule "with the
same bits" (kge_capi.hip: KGE_CSR_SERIAL, KGE_RANK_SIDE), flipped between
calls in one process: every output is equal bit for bit."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from knowledgegraphembedding_amd import KGEAdam, synth
from test_gpu_parity import DEV, build_model

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("reg", [0.0, 1e-4])
@pytest.mark.parametrize("mode", ["head-batch", "tail-batch"])
def test_csr_serial_bitwise_equals_side_stream(mode, reg, monkeypatch):
    """KGE_CSR_SERIAL=1 builds the occurrence CSR on the caller's stream before
    the row pass instead of beside it: one train_step_grads and one fused-Adam
    train_step from identical starting state give the same losses, gradients,
    updated tables and moments."""
    E, R, d, B, n = 300, 7, 32, 16, 8
    pos, neg, w = synth.kge_batch(23, B, n, E, R)
    P, N, W = torch.from_numpy(pos).to(DEV), torch.from_numpy(neg).to(DEV), torch.from_numpy(w).to(DEV)
    args = Namespace(negative_adversarial_sampling=True, adversarial_temperature=0.5, uni_weight=False,
                     regularization=reg)
    runs = []
    for serial in ("0", "1"):
        monkeypatch.setenv("KGE_CSR_SERIAL", serial)
        m, *_ = build_model("RotatE", E, R, d, 12.0, 31)
        opt = KGEAdam([p for p in m.parameters() if p.requires_grad], lr=3e-3)
        out = {"grads losses": m.compute_train_grads(P, N, W, mode, args).cpu().clone(),
               "grads entity": m.entity_embedding.grad.detach().cpu().clone(),
               "grads relation": m.relation_embedding.grad.detach().cpu().clone()}
        out["step losses"] = m.compute_train_grads(P, N, W, mode, args, optimizer=opt).cpu().clone()
        opt.step()
        for name, p in (("entity", m.entity_embedding), ("relation", m.relation_embedding)):
            st = opt.state[p]
            for what, t in (("table", p), ("grad", p.grad), ("exp_avg", st["exp_avg"]),
                            ("exp_avg_sq", st["exp_avg_sq"])):
                out[f"step {name} {what}"] = t.detach().cpu().clone()
        runs.append(out)
    assert runs[0].keys() == runs[1].keys()
    assert torch.isfinite(runs[0]["step losses"][:4]).all() and runs[0]["step losses"][4] == 0
    assert runs[0]["grads entity"].abs().max() > 0 and runs[0]["step entity exp_avg_sq"].abs().max() > 0
    for key in runs[0]:
        assert torch.equal(runs[0][key], runs[1][key]), key


@pytest.mark.parametrize("name", ["DistMult", "pRotatE"])  # the split-bf16 tile; the phase table
def test_rank_side_stream_equals_one_stream(name, monkeypatch):
    """KGE_RANK_SIDE=1 runs the entity table's statistics / split / phase table
    on the side stream beside the queries' stages: rank_queries_both and a
    single-direction call give the same ranks and tie counts."""
    E, R, d, nq = 300, 7, 32, 20
    m, *_ = build_model(name, E, R, d, 12.0, 9)
    pos, _, _ = synth.kge_batch(4, nq, 2, E, R)
    triples = pos.tolist()
    runs = []
    for side in ("0", "1"):
        monkeypatch.setenv("KGE_RANK_SIDE", side)
        (rh, th), (rt, tt) = m.rank_queries_both(triples, triples)
        r1, t1 = m.rank_queries(triples, triples, "head-batch")
        runs.append([np.asarray(x).copy() for x in (rh, th, rt, tt, r1, t1)])
    for x in runs[0][::2]:
        assert x.shape == (nq,) and (x >= 0).all() and (x <= E).all()
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
