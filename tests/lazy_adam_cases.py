"""Builders shared by the lazy-entity-Adam tests (test_lazy_adam_*.py).

The lazy rule (include/kge_hip.h, kge_train_step_lazy): a step updates the
entity rows its batch touches with the dense step's own per-element Adam and
the optimizer's GLOBAL step count, and neither reads nor writes any other row.

  lazy_adam_ref   the rule restated in plain torch (fp32, CPU or GPU)
  touched_ids     the rows a batch touches
  staleness_batches / exact_rows_batches / single_row_batch   the GPU tests' batches
  make_model, train_args, run_steps, composed_reference       the GPU runs
"""
import math
from argparse import Namespace

import numpy as np
import torch

LR, BETAS, EPS = 3e-3, (0.9, 0.999), 1e-8
MODEL_DIMS = {"TransE": (False, False), "DistMult": (False, False), "ComplEx": (True, True),
              "RotatE": (True, False), "pRotatE": (False, False)}
NAMES = tuple(MODEL_DIMS)
MODES3 = ("head-batch", "tail-batch", "head-batch")  # the modes of a 3-step run: both, alternating


# ------------------------------------------------------------- the rule
def lazy_adam_ref(param, grads_per_step, touched_per_step, lr=LR, betas=BETAS, eps=EPS):
    """The lazy rule on one [rows, width] fp32 table from zero moments.
    grads_per_step[k]: dense [rows, width] gradient of step k + 1 (only the
    touched rows are read); touched_per_step[k]: int64 ids of its touched rows.
    Per element the arithmetic of the library's Adam: the first moment as a
    lerp, eps added to sqrt(v) / sqrt(1 - beta2^t), step_size and that square
    root computed in double from the global step t and rounded to fp32.
    Returns (param, exp_avg, exp_avg_sq)."""
    b1, b2 = betas
    p = param.detach().clone()
    m = torch.zeros_like(p)
    v = torch.zeros_like(p)
    f32 = lambda x: torch.tensor(x, dtype=torch.float32, device=p.device)  # noqa: E731
    for k, (g, ids) in enumerate(zip(grads_per_step, touched_per_step)):
        t = k + 1
        step_size, bc2s = f32(lr / (1 - b1 ** t)), f32(math.sqrt(1 - b2 ** t))
        ids = ids.to(p.device)
        pr, gr, mr, vr = p[ids], g.to(p.device)[ids], m[ids], v[ids]
        mr = mr + f32(1.0 - b1) * (gr - mr)
        vr = vr * f32(b2) + f32(1.0 - b2) * (gr * gr)
        denom = vr.sqrt() / bc2s + f32(eps)
        pr = pr + (-step_size) * (mr / denom)
        p[ids], m[ids], v[ids] = pr, mr, vr
    return p, m, v


def touched_ids(pos, neg, E):
    """Ascending ids of the entity rows a batch touches: its in-range positive
    heads, positive tails and negatives."""
    ids = torch.cat([pos[:, 0].reshape(-1), pos[:, 2].reshape(-1), neg.reshape(-1)]).to(torch.int64)
    return torch.unique(ids[(ids >= 0) & (ids < E)])


# -------------------------------------------------------------- batches
def _weights(rng, B):
    return torch.from_numpy(rng.uniform(0.2, 1.0, B).astype(np.float32))


def staleness_batches(E, R, B=16, n=8, seed=7):
    """Three batches (pos, neg, w); `marked` entities — 0 and E - 1 among them —
    are touched at steps 1 and 3 and at no place of step 2.  Returns
    (batches, marked ids)."""
    rng = np.random.default_rng(seed)
    marked = np.array([0, E - 1, 7, E // 2 + 1, E - 500], dtype=np.int64)
    assert n >= len(marked) and E > 1000
    pool = np.setdiff1d(np.arange(100, E - 100), marked)
    out = []
    for step in range(3):
        pos = np.stack([rng.choice(pool, B), rng.integers(0, R, B), rng.choice(pool, B)], 1).astype(np.int64)
        neg = rng.choice(pool, (B, n)).astype(np.int64)
        if step != 1:
            neg[step, :len(marked)] = marked
            pos[B - 1, 0 if step == 0 else 2] = marked[2]  # a marked row as a positive head, then as a tail
        out.append((torch.from_numpy(pos), torch.from_numpy(neg), _weights(rng, B)))
    assert not np.isin(marked, np.concatenate([out[1][0][:, [0, 2]].numpy().ravel(), out[1][1].numpy().ravel()])).any()
    return out, torch.from_numpy(marked)


def exact_rows_batches(E, R, nrows, B=16, n=8, seed=11):
    """Three batches that each touch exactly `nrows` distinct rows (other rows
    every step), so the entity launch's last block is partly filled as asked."""
    rng = np.random.default_rng(seed)
    slots = B * n + 2 * B
    assert 1 <= nrows <= min(slots, E)
    out = []
    for _ in range(3):
        ids = rng.choice(E, nrows, replace=False)
        flat = np.concatenate([ids, rng.choice(ids, slots - nrows)])
        rng.shuffle(flat)
        pos = np.stack([flat[:B], rng.integers(0, R, B), flat[B:2 * B]], 1).astype(np.int64)
        neg = flat[2 * B:].reshape(B, n).astype(np.int64)
        out.append((torch.from_numpy(pos), torch.from_numpy(neg), _weights(rng, B)))
        assert len(touched_ids(out[-1][0], out[-1][1], E)) == nrows
    return out


def single_row_batches(E, R, seed=13):
    """B = 1, n = 1, head = tail = the negative: one touched row per step."""
    rng = np.random.default_rng(seed)
    out = []
    for e in (E - 1, 0, E // 3):
        pos = torch.tensor([[e, int(rng.integers(0, R)), e]], dtype=torch.int64)
        out.append((pos, torch.tensor([[e]], dtype=torch.int64), _weights(rng, 1)))
    return out


# ----------------------------------------------------------------- runs
def train_args():
    return Namespace(negative_adversarial_sampling=True, adversarial_temperature=0.5, uni_weight=False,
                     regularization=0.0)


def unaligned(t):
    """A contiguous copy of t one float past a 16-byte boundary (as tests/test_slot_matrix_gpu.py builds it)."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def make_model(name, E, R, d, dev, seed=5, gamma=12.0, off16=False):
    """A KGEModel with its own seeded init; off16: the entity table one float past a 16-byte boundary."""
    from knowledgegraphembedding_amd import KGEModel
    de, dr = MODEL_DIMS[name]
    torch.manual_seed(seed)
    m = KGEModel(name, E, R, d, gamma, de, dr).to(dev)
    if off16:
        m.entity_embedding.data = unaligned(m.entity_embedding.data)
    return m


def params_of(m):
    return [m.entity_embedding, m.relation_embedding] + ([m.modulus] if m.model_name == "pRotatE" else [])


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def snapshot(m, opt, losses):
    """Everything the tests compare as raw bits: tables, moments, the steps' losses."""
    out = {"losses": torch.stack([x[:4] for x in losses])}
    for k, p in zip(("entity", "relation", "modulus"), params_of(m)):
        out[k] = p.detach().clone()
        out[k + ".m"] = opt.state[p]["exp_avg"].clone()
        out[k + ".v"] = opt.state[p]["exp_avg_sq"].clone()
    return out


def assert_same(got, ref, what):
    assert got.keys() == ref.keys()
    for k in ref:
        assert same_bits(got[k], ref[k]), f"{what}: {k} differs in " \
            f"{int((bits(got[k]) != bits(ref[k])).sum())} of {ref[k].numel()} elements"


def run_steps(m, opt, batches, dev, modes=MODES3):
    """Fused train steps of `opt` (KGEAdam: dense, KGELazyAdam: lazy) on the
    batches; returns the snapshot.  The device error flag is left to the caller."""
    losses = []
    for (pos, neg, w), mode in zip(batches, modes):
        out = m.compute_train_grads(pos.to(dev), neg.to(dev), w.to(dev), mode, train_args(), optimizer=opt)
        opt.step()
        losses.append(out.detach().clone().to(dev))
    return snapshot(m, opt, losses)


def composed_reference(m, batches, dev, modes=MODES3):
    """The lazy run composed from parts tested elsewhere, on the twin model `m`:
    dense gradients from compute_train_grads(optimizer=None), the touched ids
    from the batch, ops.adam_step on the gathered touched rows scattered back,
    KGEAdam for the relation table and the modulus.  Returns (snapshot, the
    steps' dense entity gradients, the steps' touched ids)."""
    from knowledgegraphembedding_amd import KGEAdam, ops
    ent = m.entity_embedding
    rest = params_of(m)[1:]
    opt = KGEAdam(params_of(m), lr=LR, betas=BETAS, eps=EPS)  # (the entity table's state is kept by hand)
    em, ev = torch.zeros_like(ent.data), torch.zeros_like(ent.data)
    losses, grads, touched = [], [], []
    for t, ((pos, neg, w), mode) in enumerate(zip(batches, modes), 1):
        out = m.compute_train_grads(pos.to(dev), neg.to(dev), w.to(dev), mode, train_args())
        losses.append(out.detach().clone())
        ge = ent.grad.detach().clone()
        ids = touched_ids(pos, neg, ent.shape[0]).to(dev)
        rows = [x[ids].contiguous() for x in (ent.data, ge, em, ev)]
        ops.adam_step(*rows, step=t, lr=LR, beta1=BETAS[0], beta2=BETAS[1], eps=EPS)
        with torch.no_grad():
            ent.data[ids], em[ids], ev[ids] = rows[0], rows[2], rows[3]
        ent.grad = None  # KGEAdam.step() below: the relation table and the modulus only
        opt.step()
        grads.append(ge)
        touched.append(ids)
    snap = {"losses": torch.stack([x[:4] for x in losses]), "entity": ent.detach().clone(), "entity.m": em,
            "entity.v": ev}
    for k, p in zip(("relation", "modulus"), rest):
        snap[k] = p.detach().clone()
        snap[k + ".m"] = opt.state[p]["exp_avg"].clone()
        snap[k + ".v"] = opt.state[p]["exp_avg_sq"].clone()
    return snap, grads, touched


def write_dataset(root, E=40, R=3, ntrain=300, seed=2):
    """A tiny dataset in the reference's on-disk format (entities.dict, relations.dict, *.txt); returns root."""
    import os
    os.makedirs(root, exist_ok=True)
    rng = np.random.default_rng(seed)
    tr = np.stack([rng.integers(0, E, 400), rng.integers(0, R, 400), rng.integers(0, E, 400)], 1)
    with open(os.path.join(root, "entities.dict"), "w") as f:
        f.writelines(f"{i}\te{i}\n" for i in range(E))
    with open(os.path.join(root, "relations.dict"), "w") as f:
        f.writelines(f"{i}\tr{i}\n" for i in range(R))
    for name, part in (("train.txt", tr[:ntrain]), ("valid.txt", tr[ntrain:ntrain + 50]), ("test.txt", tr[ntrain + 50:])):
        with open(os.path.join(root, name), "w") as f:
            f.writelines(f"e{h}\tr{r}\te{t}\n" for h, r, t in part.tolist())
    return root
