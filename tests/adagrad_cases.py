"""The fused Adagrad step's rules restated in numpy fp32, and the GPU tests' runs
(test_adagrad_*.py).  Batches and model builders are the lazy Adam tests'
(tests/lazy_adam_cases.py).

The rule (include/kge_hip.h, kge_train_step_adagrad), one fp32 rounding per
operation:
    element-wise   s' = s + g*g;  std = sqrt(s') + eps;  p' = p + (-lr)*(g/std)
    row-wise       G' = G + (sum_k g_k*g_k)/Le;  std = sqrt(G') + eps;  p_k' = p_k + (-lr)*(g_k/std)
A zero gradient changes nothing, so the rule applied to every row of the dense
gradient is what the fused step, which touches only the batch's rows, computes.

Bounds of the comparisons against torch.optim.Adagrad (derived, not fitted):
each formula ends in one add (at most 2 roundings of |p'|: the product's and the
add's); the chain sum -> sqrt -> +eps -> quotient -> product carries about 10
roundings to first order, 16 are allowed:
    |dp|   <= 2^-22 |p'| + 2^-20 lr |g| / std
    |dsum| <= 2^-22 s'
"""
import numpy as np
import torch

import lazy_adam_cases as L

LR, EPS = 3e-2, 1e-10
f32 = np.float32


# ---------------------------------------------------------------- the rules
def adagrad_elem_ref(p, g, s, lr=LR, eps=EPS):
    """Element-wise rule on fp32 arrays of one shape; returns (p', s').  numpy
    evaluates each fp32 operation with one rounding and fuses nothing."""
    p, g, s = (np.asarray(x, dtype=f32) for x in (p, g, s))
    s1 = s + g * g
    std = np.sqrt(s1) + f32(eps)
    return p + (-f32(lr)) * (g / std), s1


def adagrad_move_ref(p, g, G1, lr=LR, eps=EPS):
    """The row-wise rule's parameter update given the new state G' [rows]."""
    p, g, G1 = (np.asarray(x, dtype=f32) for x in (p, g, G1))
    std = np.sqrt(G1) + f32(eps)
    return p + (-f32(lr)) * (g / std[:, None])


def adagrad_row_ref(p, g, G, lr=LR, eps=EPS):
    """Row-wise rule on [rows, Le] fp32 tables and the [rows] state, the row sum
    taken left to right in fp32 (one admissible order; the device's is lane-local
    then a tree, so its G' is compared through rowsum_bound, not bit for bit)."""
    g = np.asarray(g, dtype=f32)
    acc = np.zeros(g.shape[0], dtype=f32)
    for k in range(g.shape[1]):
        acc = acc + g[:, k] * g[:, k]
    G1 = np.asarray(G, dtype=f32) + acc / f32(g.shape[1])
    return adagrad_move_ref(p, g, G1, lr, eps), G1


def adagrad_row_f64(p, g, G, lr=LR, eps=EPS):
    """The row-wise rule in double precision from the same fp32 inputs; returns (p', G')."""
    p, g, G = (np.asarray(x, dtype=np.float64) for x in (p, g, G))
    G1 = G + (g * g).sum(1) / g.shape[1]
    std = np.sqrt(G1) + float(f32(eps))
    return p + (-float(f32(lr))) * (g / std[:, None]), G1


def rowsum_bound(G1_f64, Le):
    """|G'_fp32 - G'_double| <= (Le + 4) 2^-24 G': Le rounded squares and adds of
    non-negative terms (each partial sum <= the total), the division, the
    accumulation onto G."""
    return (Le + 4) * 2.0 ** -24 * G1_f64


def p_bound(p1, g, std, lr=LR):
    return 2.0 ** -22 * np.abs(p1) + 2.0 ** -20 * float(lr) * np.abs(g) / std


def sum_bound(s1):
    return 2.0 ** -22 * s1


def torch_adagrad_step(p, g, s, lr=LR, eps=EPS):
    """One torch.optim.Adagrad step on the CPU from the given fp32 p / sum; returns (p', sum') as numpy."""
    par = torch.nn.Parameter(torch.from_numpy(np.array(p, dtype=f32)))
    opt = torch.optim.Adagrad([par], lr=lr, eps=eps)
    opt.state[par]["sum"] = torch.from_numpy(np.array(s, dtype=f32))
    par.grad = torch.from_numpy(np.array(g, dtype=f32))
    opt.step()
    return par.detach().numpy(), opt.state[par]["sum"].numpy()


# -------------------------------------------------------------------- runs
def make_opt(m, rowwise=False, lr=LR, eps=EPS):
    from knowledgegraphembedding_amd import KGEAdagrad
    return KGEAdagrad(L.params_of(m), lr=lr, eps=eps, rowwise_entity=rowwise)


def snapshot(m, opt, losses):
    out = {"losses": torch.stack([x[:4] for x in losses])}
    for k, p in zip(("entity", "relation", "modulus"), L.params_of(m)):
        out[k] = p.detach().clone()
        out[k + ".sum"] = opt.state[p]["sum"].clone()
    return out


def run_steps(m, opt, batches, dev, modes=L.MODES3, after_step=None):
    """Fused Adagrad steps on the batches; after_step(k, m, opt) sees every step's result."""
    losses = []
    for k, ((pos, neg, w), mode) in enumerate(zip(batches, modes)):
        out = m.compute_train_grads(pos.to(dev), neg.to(dev), w.to(dev), mode, L.train_args(), optimizer=opt)
        opt.step()
        losses.append(out.detach().clone().to(dev))
        if after_step is not None:
            after_step(k, m, opt)
    return snapshot(m, opt, losses)


def _np(t):
    return t.detach().cpu().numpy()


def dense_reference_steps(m, batches, dev, modes=L.MODES3, rowwise_state=None):
    """The composed reference on the twin model `m`: per step, dense gradients from
    compute_train_grads(optimizer=None), then the numpy element-wise rule on EVERY row of
    every table (the dense update).  Yields, per step, a snapshot-shaped dict of torch
    tensors on `dev` plus "grad.entity" (the step's dense entity gradient) and
    "entity.before".  rowwise_state: a callable k -> the device's own G' [E] of step k
    (numpy); the entity table is then moved by the row-wise rule with that state."""
    params = L.params_of(m)
    keys = ("entity", "relation", "modulus")[:len(params)]
    sums = {k: np.zeros(tuple(p.shape), dtype=f32) for k, p in zip(keys, params)}
    losses = []
    for step, ((pos, neg, w), mode) in enumerate(zip(batches, modes)):
        out = m.compute_train_grads(pos.to(dev), neg.to(dev), w.to(dev), mode, L.train_args())
        losses.append(out.detach().clone())
        snap = {"entity.before": params[0].detach().clone(), "grad.entity": params[0].grad.detach().clone()}
        for k, p in zip(keys, params):
            g = _np(p.grad)
            if k == "entity" and rowwise_state is not None:
                G1 = rowwise_state(step)
                p1, sums[k] = adagrad_move_ref(_np(p), g, G1), G1
            else:
                p1, sums[k] = adagrad_elem_ref(_np(p), g, sums[k])
            with torch.no_grad():
                p.copy_(torch.from_numpy(p1).to(dev))
            p.grad = None
            snap[k] = p.detach().clone()
            snap[k + ".sum"] = torch.from_numpy(sums[k].copy()).to(dev)
        snap["losses"] = torch.stack([x[:4] for x in losses])
        yield snap


def same_keys_same_bits(got, ref, what):
    for k in got:
        assert L.same_bits(got[k], ref[k]), f"{what}: {k} differs in " \
            f"{int((L.bits(got[k]) != L.bits(ref[k])).sum())} of {ref[k].numel()} elements"
