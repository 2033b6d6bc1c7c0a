"""kge_train_step_adagrad (both kinds) and kge_adagrad_step on exactly sized,
guard-banded device buffers (tests/arena.py), the workspace poisoned and of
exactly the queried size: no guard byte may change, untouched rows keep their
bytes, and the result has the bits of the same call on ordinary tensors."""
import ctypes as C

import numpy as np
import pytest
import torch

import adagrad_cases as A
import lazy_adam_cases as L
from arena import arena, arena_of
from knowledgegraphembedding_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
E, R, B, N = 300, 5, 6, 7


def _stream():
    return ops._stream(DEV)


def _batch(seed):
    rng = np.random.default_rng(seed)
    pool = np.arange(10, E - 10)  # rows 0..9 and E-10..E-1 stay untouched: the tables' first and last bytes
    pos = np.stack([rng.choice(pool, B), rng.integers(0, R, B), rng.choice(pool, B)], 1).astype(np.int64)
    neg = rng.choice(pool, (B, N)).astype(np.int64)
    w = rng.uniform(0.2, 1.0, B).astype(np.float32)
    return pos, neg, w


def _step(guarded, name, d, rowwise, mode):
    """One kge_train_step_adagrad call from a non-zero state; returns the tables and states (host)
    and, when guarded, checks every band."""
    src = L.make_model(name, E, R, d, DEV)
    params = [p.detach() for p in L.params_of(src)]
    g, rng = src._host_scalars()
    gen = torch.Generator().manual_seed(9)
    shapes = [(E,) if (rowwise and k == 0) else tuple(p.shape) for k, p in enumerate(params)]
    states = [torch.rand(s, generator=gen) * 0.01 for s in shapes]
    pos, neg, w = _batch(3)
    held = []

    def buf(t, dtype=None):
        t = t if isinstance(t, torch.Tensor) else torch.from_numpy(t)
        if not guarded:
            return t.to(DEV).clone()
        held.append(arena_of(t.cpu(), DEV))
        return held[-1].view

    def out(shape, dtype=torch.float32):
        if not guarded:
            t = torch.empty(shape, dtype=dtype, device=DEV)
            t.view(torch.uint8).fill_(0xFF)
            return t
        held.append(arena(shape, dtype, DEV))
        return held[-1].view

    tabs = [buf(p) for p in params]
    sums = [buf(s) for s in states]
    tpos, tneg, tw = buf(pos), buf(neg), buf(w)
    gr = out(tuple(params[1].shape))
    gm = out((1, 1)) if len(params) == 3 else None
    losses = out((5,))
    err = buf(torch.zeros(1, dtype=torch.int32))
    desc = ops.make_desc(name, tabs[0], tabs[1], g, rng, tabs[2] if len(tabs) == 3 else None)
    need = _lib.load().kge_train_adagrad_workspace_bytes(C.byref(desc), B, N)
    ws = out((need,), torch.uint8)  # (guarded: 0xFF everywhere, exactly `need` bytes)
    ad = _lib.AdagradDesc()
    ad.lr, ad.eps, ad.entity_rowwise, ad.write_grad = A.LR, A.EPS, int(rowwise), 1
    for t, p, s in zip((ad.entity, ad.relation, ad.modulus), tabs, sums):
        t.param, t.state_sum = p.data_ptr(), s.data_ptr()
    before = [t.cpu().clone() for t in tabs + sums]
    st = _lib.load().kge_train_step_adagrad(
        C.byref(desc), _lib.MODE_IDS[mode], tpos.data_ptr(), tneg.data_ptr(), B, N, tw.data_ptr(), None, 0, 0, 1, 0.5,
        0.0, C.byref(ad), None, gr.data_ptr(), ops._ptr(gm), losses.data_ptr(), ws.data_ptr(), need, err.data_ptr(),
        _stream())
    assert st == 0, _lib.load().kge_status_string(st).decode()
    torch.cuda.synchronize(DEV)
    assert int(err.item()) == 0
    for a in held:
        a.check()
    res = dict(entity=tabs[0].cpu(), relation=tabs[1].cpu(), entity_sum=sums[0].cpu(), relation_sum=sums[1].cpu(),
               grad_relation=gr.cpu(), losses=losses[:4].cpu())
    if gm is not None:
        res.update(modulus=tabs[2].cpu(), modulus_sum=sums[2].cpu(), grad_modulus=gm.cpu())
    # inputs stay as given; untouched entity rows keep their bytes, touched rows' state grew
    assert torch.equal(tpos.cpu(), torch.from_numpy(pos)) and torch.equal(tneg.cpu(), torch.from_numpy(neg))
    touched = L.touched_ids(torch.from_numpy(pos), torch.from_numpy(neg), E)
    un = torch.ones(E, dtype=torch.bool)
    un[touched] = False
    assert L.same_bits(res["entity"][un], before[0][un]) and L.same_bits(res["entity_sum"][un], before[len(tabs)][un])
    assert (res["entity_sum"][touched] >= before[len(tabs)][touched]).all() and torch.isfinite(res["losses"]).all()
    assert not L.same_bits(res["entity"][touched], before[0][touched])
    return res


@pytest.mark.parametrize("rowwise", [False, True], ids=["elementwise", "rowwise"])
@pytest.mark.parametrize("name,d,mode", [("RotatE", 64, "head-batch"), ("pRotatE", 24, "tail-batch"),
                                         ("TransE", 63, "head-batch"), ("RotatE", 520, "tail-batch")])
def test_train_step_adagrad(name, d, mode, rowwise):
    """d = 64: one slice; 24: a partly filled wave; 63: single-float slots; 520: 4 column slices
    element-wise (S = 130 slots), the row-per-wave pass with NS = 4 row-wise."""
    got, plain = _step(True, name, d, rowwise, mode), _step(False, name, d, rowwise, mode)
    assert got.keys() == plain.keys()
    for k in got:
        assert L.same_bits(got[k], plain[k]), f"{name} d={d} {mode} rowwise={rowwise}: {k}"


@pytest.mark.parametrize("n", [4 * 1031 + 3, 8, 4])
def test_adagrad_step(n):
    rng = np.random.default_rng(n)
    p, g, s = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    s = np.abs(s)
    ap, ag, asum = (arena_of(x, DEV) for x in (p, g, s))
    st = _lib.load().kge_adagrad_step(ap.ptr(), ag.ptr(), asum.ptr(), n, A.LR, A.EPS, _stream())
    assert st == 0
    torch.cuda.synchronize(DEV)
    for a in (ap, ag, asum):
        a.check()
    ag.unchanged(g)
    p1, s1 = A.adagrad_elem_ref(p, g, s)
    ap.unchanged(p1)
    asum.unchanged(s1)
