"""KGEAdam — torch.optim.Adam's update as one fused HIP kernel per tensor;
KGELazyAdam — the same with the entity table updated only in the rows a batch
touches; KGEAdagrad — Adagrad fused into the lazy step, where updating the
touched rows alone is the dense update.

The reference optimises with a plain torch.optim.Adam(lr) (run.py:266-269,
re-created on every learning-rate decay, run.py:315-322).  KGEAdam keeps that
optimizer's hyper-parameters, per-parameter state keys ('step', 'exp_avg',
'exp_avg_sq') and state_dict layout, so checkpoints move between the two in
either direction; the dense update (every row, zero-grad rows included —
SURVEY §7 hard part vii) runs in kge_adam_step.
"""
from __future__ import annotations

import math

import torch

from . import ops


class KGEAdam(torch.optim.Optimizer):
    lazy_entity = False  # KGELazyAdam: the fused step updates touched entity rows only
    fused_setting = "betas / eps"  # what prepare_fused needs equal across the tables' groups

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False):
        if weight_decay != 0 or amsgrad:
            raise ValueError("KGEAdam implements the reference's Adam configuration only "
                             "(weight_decay=0, amsgrad=False)")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=False, maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=None)
        super().__init__(params, defaults)

        self._fused_done = set()

    def _group_of(self, p):
        for g in self.param_groups:
            for q in g['params']:
                if q is p:
                    return g
        return None

    def _advance(self, p, group):
        state = self.state[p]
        if len(state) == 0:
            state['step'] = torch.tensor(0.0)
            state['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        state['step'] += 1
        return state, int(state['step'].item())

    def prepare_fused(self, entity, relation, modulus=None, write_grad=True):
        """Adam descriptor for kge_train_step, which applies this optimizer's
        update to the tables inside the gradient passes.  Advances the step
        counters now and marks the tensors so the following step() skips them.
        Returns None (use the unfused path) if the configuration does not fit."""
        from . import _lib
        tensors = [entity, relation] + ([modulus] if modulus is not None else [])
        groups = [self._group_of(p) for p in tensors]
        if any(g is None for g in groups) or any(not p.requires_grad for p in tensors):
            return None
        if len({(g['betas'], g['eps']) for g in groups}) != 1:
            return None
        if any(not p.is_contiguous() for p in tensors):
            return None
        desc = _lib.AdamDesc()
        beta1, beta2 = groups[0]['betas']
        desc.beta1, desc.beta2, desc.eps = beta1, beta2, groups[0]['eps']
        desc.write_grad = 1 if write_grad else 0
        for p, g, field in zip(tensors, groups, ('entity', 'relation', 'modulus')):
            state, step = self._advance(p, g)
            t = getattr(desc, field)
            t.param = p.data_ptr()
            t.exp_avg = state['exp_avg'].data_ptr()
            t.exp_avg_sq = state['exp_avg_sq'].data_ptr()
            t.step_size = g['lr'] / (1 - beta1 ** step)
            t.bias_correction2_sqrt = math.sqrt(1 - beta2 ** step)
            self._fused_done.add(id(p))
        return desc

    def prepare_fused_rows(self, shard, table, row0, relation, modulus=None, write_grad=True):
        """prepare_fused for an owner of entity rows [row0, row0 + len(shard)):
        `shard` is the optimizer's parameter (a view of those rows of `table`,
        whose moments are shard-sized); the descriptor points the entity
        update at `table` and its moments `row0` rows before the shard's, so
        the kernels index them by global row (kge_train_step_from_rows_range
        touches only the owned rows).  None if the configuration does not fit."""
        from . import _lib
        if shard.data_ptr() != table.data_ptr() + row0 * table.stride(0) * table.element_size():
            return None
        desc = self.prepare_fused(shard, relation, modulus, write_grad)
        if desc is None:
            return None
        off = row0 * table.stride(0) * table.element_size()
        st = self.state[shard]
        desc.entity.param = table.data_ptr()
        desc.entity.exp_avg = st['exp_avg'].data_ptr() - off
        desc.entity.exp_avg_sq = st['exp_avg_sq'].data_ptr() - off
        return desc

    @torch.no_grad()
    def step_param(self, p, chunks=None, before_chunk=None) -> bool:
        """Apply this step's update to ONE parameter now — row range by row
        range, calling before_chunk(k) before range k (the data-parallel path
        waits there for that range's all-reduce) — and skip it in the next
        step().  Same per-element arithmetic as step()."""
        group = self._group_of(p)
        if group is None or p.grad is None or id(p) in self._fused_done:
            return False
        beta1, beta2 = group['betas']
        state, step = self._advance(p, group)
        row_bytes = p[0].numel() * p.element_size() if p.dim() > 1 else 0
        if chunks is not None and (p.dim() < 2 or row_bytes % 16 != 0 or not p.grad.is_contiguous()):
            # row ranges would break kge_adam_step's 16-byte alignment: wait for
            # every range first, then update the whole tensor at once
            if before_chunk is not None:
                for k in range(len(chunks)):
                    before_chunk(k)
            chunks, before_chunk = None, None
        if chunks is None:
            chunks = [(0, p.shape[0] if p.dim() else 1)]
        for k, (r0, r1) in enumerate(chunks):
            if before_chunk is not None:
                before_chunk(k)
            sl = (slice(r0, r1),) if p.dim() else ()
            ops.adam_step(p.data[sl], p.grad[sl], state['exp_avg'][sl], state['exp_avg_sq'][sl], step=step,
                          lr=group['lr'], beta1=beta1, beta2=beta2, eps=group['eps'])
        self._fused_done.add(id(p))
        return True

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        done, self._fused_done = self._fused_done, set()
        for group in self.param_groups:
            beta1, beta2 = group['betas']
            for p in group['params']:
                if p.grad is None or id(p) in done:
                    continue
                state, step = self._advance(p, group)
                grad = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                ops.adam_step(p.data, grad, state['exp_avg'], state['exp_avg_sq'], step=step,
                              lr=group['lr'], beta1=beta1, beta2=beta2, eps=group['eps'])
        return loss


class KGELazyAdam(KGEAdam):
    """KGEAdam whose ENTITY table is updated lazily: a fused train step
    (kge_train_step_lazy) applies Adam only to the entity rows its batch
    touches — a positive head or tail, or a negative — and neither reads nor
    writes any other row's parameter or moments.  A touched row gets exactly
    the dense step's update, with the bias corrections of the optimizer's
    global step count (there is no per-row count); the relation table and the
    pRotatE modulus keep the dense update.  This is "lazy Adam" with
    KGEAdam's own per-element formula, not torch.optim.SparseAdam's.

    Hyper-parameters, state keys and state_dict layout are KGEAdam's, so
    checkpoints move between the dense and the lazy optimizer in both
    directions.  The lazy step exists only fused into the gradient passes of a
    single process: KGEModel.train_step raises ValueError for a row partition,
    a data-parallel group, model.fuse_optimizer = False or a regulariser.  No
    dense entity gradient exists, so entity_embedding.grad stays None and
    step() has nothing left to do for that table."""

    lazy_entity = True
    lazy_name = "KGELazyAdam (lazy entity Adam)"  # as KGEModel's refusals name it


class KGEAdagrad(torch.optim.Optimizer):
    """Adagrad fused into the lazy train step (kge_train_step_adagrad).

    The rule (include/kge_hip.h), per element in fp32:
        sum += g*g;  p += (-lr) * (g / (sqrt(sum) + eps))
    is torch.optim.Adagrad's with lr_decay = 0, weight_decay = 0 and
    initial_accumulator_value = 0 — the only configuration served.  A zero
    gradient changes neither `sum` nor `p`, so the fused step, which touches
    only the entity rows of its batch, equals the dense update on every row at
    every step: there is no staleness as with KGELazyAdam, and the state is
    one table instead of two.

    rowwise_entity=True keeps ONE float per entity row instead (state 4*E
    bytes): G += mean_k(g_k^2), p_k += (-lr) * (g_k / (sqrt(G) + eps)).  The
    relation table and the pRotatE modulus stay element-wise.

    State keys are 'step' and 'sum'; without rowwise_entity a state_dict loads
    into torch.optim.Adagrad and back.  Like KGELazyAdam the step exists only
    fused into the gradient passes of a single process (KGEModel.train_step
    raises ValueError for a row partition, a data-parallel group,
    model.fuse_optimizer = False or a regulariser); step() applies the dense
    element-wise rule (kge_adagrad_step) to any other parameter with a .grad."""

    lazy_entity = True
    lazy_name = "KGEAdagrad (fused lazy Adagrad)"
    fused_setting = "lr / eps"

    def __init__(self, params, lr=1e-2, eps=1e-10, rowwise_entity=False, lr_decay=0, weight_decay=0,
                 initial_accumulator_value=0):
        if lr_decay != 0 or weight_decay != 0 or initial_accumulator_value != 0:
            raise ValueError("KGEAdagrad implements lr_decay=0, weight_decay=0, initial_accumulator_value=0 only")
        if not lr >= 0.0 or math.isinf(lr):
            raise ValueError(f"Invalid learning rate: {lr}")
        if not eps > 0.0:
            raise ValueError(f"Invalid epsilon value: {eps} (must be > 0: with eps = 0 an untouched all-zero row "
                             "would be NaN under the dense rule)")
        defaults = dict(lr=lr, lr_decay=0, eps=eps, weight_decay=0, initial_accumulator_value=0, foreach=None,
                        maximize=False, differentiable=False, fused=None)
        super().__init__(params, defaults)
        self.rowwise_entity = bool(rowwise_entity)
        self._fused_done = set()
        self._rowwise = set()  # ids of the parameters whose 'sum' is one float per row

    _group_of = KGEAdam._group_of

    def _advance(self, p, rowwise=False):
        state = self.state[p]
        if len(state) == 0:
            state['step'] = torch.tensor(0.0)
            if rowwise:
                state['sum'] = torch.zeros(p.shape[0], dtype=p.dtype, device=p.device)
            else:
                state['sum'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        state['step'] += 1
        return state

    def prepare_fused(self, entity, relation, modulus=None, write_grad=True):
        """Adagrad descriptor for kge_train_step_adagrad.  Advances the step
        counters now and marks the tensors so the following step() skips them.
        Returns None if the configuration does not fit."""
        from . import _lib
        tensors = [entity, relation] + ([modulus] if modulus is not None else [])
        groups = [self._group_of(p) for p in tensors]
        if any(g is None for g in groups) or any(not p.requires_grad for p in tensors):
            return None
        if len({(g['lr'], g['eps']) for g in groups}) != 1:  # the descriptor carries one lr and one eps
            return None
        if any(not p.is_contiguous() for p in tensors):
            return None
        desc = _lib.AdagradDesc()
        desc.lr, desc.eps = groups[0]['lr'], groups[0]['eps']
        desc.entity_rowwise = 1 if self.rowwise_entity else 0
        desc.write_grad = 1 if write_grad else 0
        for p, field in zip(tensors, ('entity', 'relation', 'modulus')):
            rowwise = self.rowwise_entity and field == 'entity'
            state = self._advance(p, rowwise)
            if state['sum'].shape != ((p.shape[0],) if rowwise else p.shape) or not state['sum'].is_contiguous():
                raise ValueError(f"KGEAdagrad: the {field} table's 'sum' state has shape {tuple(state['sum'].shape)}; "
                                 f"rowwise_entity={self.rowwise_entity} needs "
                                 f"{(p.shape[0],) if rowwise else tuple(p.shape)}")
            if rowwise:
                self._rowwise.add(id(p))
            t = getattr(desc, field)
            t.param = p.data_ptr()
            t.state_sum = state['sum'].data_ptr()
            self._fused_done.add(id(p))
        return desc

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        done, self._fused_done = self._fused_done, set()
        for group in self.param_groups:
            for p in group['params']:
                if p.grad is None or id(p) in done:
                    continue
                if id(p) in self._rowwise or ('sum' in self.state[p] and self.state[p]['sum'].shape != p.shape):
                    raise ValueError("KGEAdagrad: a row-wise entity table has no dense step (its .grad must stay None; "
                                     "the update exists only fused into the train step)")
                state = self._advance(p)
                grad = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                ops.adagrad_step(p.data, grad, state['sum'], lr=group['lr'], eps=group['eps'])
        return loss
