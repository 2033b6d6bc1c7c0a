"""Query shipping (kge_ship_step) in one process: the shard patterns, the two
wide-negative cases and a driver that plays every rank in turn.

No GPU is needed to import this module; run_ship needs one.

Shard patterns: cut points over test_slot_matrix_ref's E = 40, shard k owns
[cuts[k], cuts[k + 1]).  The C ABI takes any [own_begin, own_end); partition.py
only ever makes equal shards with the empty ones last, so W3 and W4 go beyond
what the host mirror exercises.

    W1  (0, 40)             one shard owning everything
    W2  (0, 20, 40)         the trained-regime (D) geometry: positives below 20, random
                            negatives from 20 on, so the dominant negative sits alone in shard 0
    W3  (0, 33, 39, 40)     a shard of one row; a shard holding most of the table
    W4  (0, 5, 5, 23, 40)   an empty shard in the middle; uneven shards

run_ship(inp, tr, cuts) runs one full step for world = len(cuts) - 1 emulated
ranks on one stream, through _lib.load().kge_ship_step directly (ops.ship_step's
workspace carries slack).  Stage order and collectives are those of
EntityRowPartition._ship_step:

    Q on every rank       q (head-batch: q | qp) summed over the ranks
    ROWS                  part stacked into parts [world, B, 4]
    MERGE                 dq | pstats (head-batch: | pq) summed
    CHAIN                 grad_relation summed
    ENTITY

Each sum is an fp32 torch sum accumulated in rank order 0, 1, …, its result
copied back into every rank's buffer.

Per emulated rank every device pointer is the view of its own tests/arena.py
arena of exactly the documented size: the eleven kge_ship_desc buffers, pos, neg,
w, weight_sum, grad_relation, grad_modulus, losses [5], err_flag, and a workspace
of exactly kge_train_workspace_bytes(m, B, n) bytes that is left poisoned.  The
entity table, grad_entity and the fused Adam's entity moments of a rank are each
a FULL [E, Le] arena filled with 0xFF with only rows [lo, hi) copied in, and the
descriptor's pointer is the arena's row 0 (partition.py offsets a shard-sized
allocation by -lo rows instead): a read of a row the rank does not own yields
NaN, which the value checks see; it stays inside memory the test owns; and a
write to such a row shows when the rows outside [lo, hi) are compared with the
fill.  The relation table and the modulus are replicated per rank.

After every stage of every rank, behind a stream sync: the status is KGE_OK,
err_flag is 0, and in every arena of that rank both bands hold their fill, every
read-only buffer is byte for byte what was put in and the rows outside [lo, hi)
of the table, grad_entity and the moments hold the fill.  (A byte once written
stays written: the last stage's pass over all ranks is also the proof for the
stages before it; the earlier passes say which stage did it.)
"""
import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from arena import FLOAT_FILL, arena, arena_of
from test_slot_matrix_ref import B, E, Case

PATTERNS = {"W1": (0, 40), "W2": (0, 20, 40), "W3": (0, 33, 39, 40), "W4": (0, 5, 5, 23, 40)}
assert all(c[0] == 0 and c[-1] == E and list(c) == sorted(c) for c in PATTERNS.values())

# merge's j loop strides (n > 256) and, under W4, a shard owns more than 64 and fewer than 256
# of a row's negatives; both must meet rho_case <= RHO_CAP (test_ship_stages_ref)
WIDE_N = [Case("B", "RotatE", 64, n=300), Case("B", "TransE", 9, n=257)]

STAGES = ("Q", "ROWS", "MERGE", "CHAIN", "ENTITY")
BETAS, EPS, LR = (0.9, 0.999), 1e-8, 3e-3
F32, I64, I32, U8 = torch.float32, torch.int64, torch.int32, torch.uint8


def shards(cuts):
    return list(zip(cuts[:-1], cuts[1:]))


def shard_of(cuts, ids):
    """The shard that owns each id (empty shards own nothing); -1 for an id outside [0, E)."""
    ids = np.asarray(ids)
    out = np.full(ids.shape, -1, dtype=np.int64)
    for k, (lo, hi) in enumerate(shards(cuts)):
        out[(ids >= lo) & (ids < hi)] = k
    return out


def split_rows(pos, cuts):
    """Per row: whether h and t live in different shards."""
    return shard_of(cuts, pos[:, 0]) != shard_of(cuts, pos[:, 2])


def starved_rows(neg, cuts):
    """Per row: whether some NON-EMPTY shard owns none of the row's negatives (that shard's
    partial softmax state for the row is the -inf one)."""
    own = shard_of(cuts, neg)
    return np.array([any(hi > lo and not (own[i] == k).any() for k, (lo, hi) in enumerate(shards(cuts)))
                     for i in range(neg.shape[0])])


# ------------------------------------------------------------------ the driver
@dataclass
class Fused:
    """The fused Adam of a run: initial moments of the whole table ([E, Le] host arrays; a rank
    gets its rows) and of pRotatE's modulus."""
    write_grad: int
    m0: np.ndarray
    v0: np.ndarray
    mod_m0: Optional[np.ndarray] = None
    mod_v0: Optional[np.ndarray] = None
    step: int = 3


@dataclass
class RankOut:
    lo: int
    hi: int
    grad_entity: torch.Tensor            # the full [E, Le] arena's interior (rows outside [lo, hi): fill)
    grad_relation: torch.Tensor          # after the rank-order sum
    grad_modulus: Optional[torch.Tensor]
    losses: torch.Tensor
    row_stats: torch.Tensor              # after CHAIN
    g_merge: torch.Tensor                # g after MERGE
    table: torch.Tensor                  # the full [E, Le] table arena's interior after the step
    modulus: Optional[torch.Tensor]
    moments: dict = field(default_factory=dict)   # "entity.m", "entity.v", "modulus.m", "modulus.v"
    err: int = 0


class _Rank:
    """The buffers of one emulated rank and the record of what may change in them."""

    def __init__(self, dev, lo, hi):
        self.dev, self.lo, self.hi = dev, lo, hi
        self.arenas = {}
        self.free = {}     # name -> (first, last) byte range of the interior a call may write
        self.plain = []    # tensors that are no arenas (unaligned tables): values only
        self.snap = {}

    def put(self, name, src, *, ro=True):
        a = self.arenas[name] = arena_of(src if isinstance(src, torch.Tensor) else torch.from_numpy(np.array(src)),
                                         self.dev, name=name)
        self.free[name] = (0, 0) if ro else (0, a.nbytes)
        return a.view

    def out(self, name, shape, dtype=F32):
        a = self.arenas[name] = arena(shape, dtype, self.dev, name=name)
        self.free[name] = (0, a.nbytes)
        return a.view

    def rows(self, name, full, *, ro, copy=True):
        """A full [E, Le] arena at its fill with rows [lo, hi) of `full` copied in (copy = False:
        left at the fill too); writable (ro = False) in those rows only."""
        a = self.arenas[name] = arena(tuple(full.shape), F32, self.dev, name=name)
        if copy and self.hi > self.lo:
            a.view[self.lo:self.hi].copy_(torch.from_numpy(np.array(full[self.lo:self.hi])))
        rb = full.shape[1] * 4
        self.free[name] = (0, 0) if ro else (self.lo * rb, self.hi * rb)
        return a.view

    def seal(self):
        """Every arena as it stands is what must still be there, outside its writable bytes."""
        self.snap = {k: a.backing.clone() for k, a in self.arenas.items()}

    def dirty(self):
        """A device scalar: the bytes that differ from the sealed state outside the writable ranges."""
        tot = torch.zeros((), dtype=I64, device=self.dev)
        for k, a in self.arenas.items():
            f0, f1 = self.free[k]
            s, b = self.snap[k], a.backing
            tot += (b[:a.start + f0] != s[:a.start + f0]).sum() + (b[a.start + f1:] != s[a.start + f1:]).sum()
        return tot

    def explain(self, what):
        """The precise failure behind dirty() != 0, through the arenas' own checks."""
        for k, a in self.arenas.items():
            a.check()
            f0, f1 = self.free[k]
            got = a.bytes.cpu()
            want = self.snap[k][a.start:a.end].cpu()
            bad = torch.cat([(got[:f0] != want[:f0]).nonzero(), (got[f1:] != want[f1:]).nonzero() + f1])
            if bad.numel():
                first = int(bad[0, 0])
                row = f" (row {first // (a.view.shape[1] * 4)})" if a.view.dim() == 2 else ""
                raise AssertionError(f"{what}: arena {k} of the rank owning [{self.lo}, {self.hi}): {bad.shape[0]} "
                                     f"interior byte(s) changed that the call must not write, first at byte "
                                     f"{first}{row}")
        raise AssertionError(f"{what}: guarded bytes changed")  # (dirty() saw what the passes above did not)


def run_ship(inp, tr, cuts, *, fused=None, place=None, pos=None, neg=None, err_ok=False, dev=None):
    """One query-shipping step of inp (test_slot_matrix_ref.Inputs) under tr (its Train) for the
    shards of `cuts`; returns [RankOut] in rank order.  fused: a Fused, or None for adam == NULL.
    place(t): a device tensor holding host tensor t, used for the entity and relation tables in
    place of arenas (the unaligned cases: values only).  pos / neg replace the case's ids (the
    index-error cases), err_ok lets err_flag be non-zero after a stage."""
    from knowledgegraphembedding_amd import _lib, ops
    lib = _lib.load()
    dev = dev or torch.device("cuda", 0)
    case = inp.case
    mode, head = tr.mode, tr.mode == "head-batch"
    pos = inp.pos if pos is None else pos
    neg = inp.neg[mode] if neg is None else neg
    n = neg.shape[1]
    Le, Lr = inp.ent.shape[1], inp.rel.shape[1]
    world = len(cuts) - 1
    stream = ops._stream(dev)

    wsum_t = torch.empty(1, dtype=F32, device=dev)
    w_t = torch.from_numpy(inp.w).to(dev)
    st = lib.kge_weight_sum(w_t.data_ptr(), B, wsum_t.data_ptr(), stream)
    assert st == 0, f"kge_weight_sum: status {st}"
    wsum = wsum_t.cpu()

    ranks, calls = [], []
    for r, (lo, hi) in enumerate(shards(cuts)):
        k = _Rank(dev, lo, hi)
        if place is None:
            ent = k.rows("entity", inp.ent, ro=fused is None)
            rel = k.put("relation", inp.rel)
        else:
            full = torch.full(inp.ent.shape, math.nan, dtype=F32)
            full[lo:hi] = torch.from_numpy(inp.ent[lo:hi])
            ent, rel = place(full), place(torch.from_numpy(inp.rel))
            k.plain += [ent, rel]
        mod = None if inp.mod is None else k.put("modulus", inp.mod, ro=fused is None)
        desc = ops.make_desc(case.name, ent, rel, inp.g32, inp.erange, mod)
        assert desc.nentity == E
        v = dict(pos=k.put("pos", pos), neg=k.put("neg", neg), w=k.put("subsampling_weight", inp.w),
                 wsum=k.put("weight_sum", wsum), err=k.put("err_flag", torch.zeros(1, dtype=I32), ro=False),
                 q=k.out("q", (B, Le)), qp=k.out("qp", (B, Le)), part=k.out("part", (B, 4)),
                 parts=k.out("parts", (world, B, 4)), scores=k.out("scores", (B, n)), g=k.out("g", (B, n)),
                 dq=k.out("dq", (B, Le)), pq=k.out("pq", (B, Le)), pstats=k.out("pstats", (B, 4)),
                 ent_contrib=k.out("ent_contrib", (2 * B, Le)), rel_contrib=k.out("rel_contrib", (B, Lr)),
                 row_stats=k.out("row_stats", (B, 4)), gr=k.out("grad_relation", inp.rel.shape),
                 gm=None if mod is None else k.out("grad_modulus", (1, 1)), losses=k.out("losses", 5),
                 ent=ent, rel=rel, mod=mod)
        # grad_entity: a full table at its fill, written (if at all) in the owned rows only
        v["ge"] = k.rows("grad_entity", inp.ent, ro=False, copy=False)
        need = lib.kge_train_workspace_bytes(desc, B, n)
        k.out("workspace", int(need), U8)
        adam = None
        if fused is not None:
            adam = _lib.AdamDesc()
            adam.beta1, adam.beta2, adam.eps, adam.write_grad = BETAS[0], BETAS[1], EPS, int(fused.write_grad)
            v["em"] = k.rows("entity.exp_avg", fused.m0, ro=False)
            v["ev"] = k.rows("entity.exp_avg_sq", fused.v0, ro=False)
            tensors = [(adam.entity, ent, v["em"], v["ev"])]
            if mod is not None:
                v["mm"] = k.put("modulus.exp_avg", fused.mod_m0, ro=False)
                v["mv"] = k.put("modulus.exp_avg_sq", fused.mod_v0, ro=False)
                tensors.append((adam.modulus, mod, v["mm"], v["mv"]))
            for t, p, m_, v_ in tensors:
                t.param, t.exp_avg, t.exp_avg_sq = p.data_ptr(), m_.data_ptr(), v_.data_ptr()
                t.step_size = LR / (1 - BETAS[0] ** fused.step)
                t.bias_correction2_sqrt = math.sqrt(1 - BETAS[1] ** fused.step)
        sd = _lib.ShipDesc()
        sd.world, sd.rank, sd.own_begin, sd.own_end = world, r, lo, hi
        sd.pos, sd.neg, sd.batch, sd.nneg = v["pos"].data_ptr(), v["neg"].data_ptr(), B, n
        sd.subsampling_weight, sd.weight_sum = v["w"].data_ptr(), v["wsum"].data_ptr()
        sd.uni_weight, sd.adversarial, sd.uni_batch = int(tr.uni_weight), int(tr.adversarial), B
        sd.adversarial_temperature, sd.regularization = float(tr.temperature), float(tr.regularization)
        for f in ("q", "qp", "part", "parts", "scores", "g", "dq", "pq", "pstats", "ent_contrib", "rel_contrib",
                  "row_stats"):
            setattr(sd, f, v[f].data_ptr())
        k.seal()
        k.v = v
        ranks.append(k)
        ws = k.arenas["workspace"]
        calls.append((desc, sd, adam, (v["ge"].data_ptr(), v["gr"].data_ptr(), ops._ptr(v["gm"]),
                                       v["losses"].data_ptr(), ws.ptr(), ws.nbytes, v["err"].data_ptr(), stream)))

    def stage(s):
        for r, (k, (desc, sd, adam, rest)) in enumerate(zip(ranks, calls)):
            what = f"{case.id} {mode} rank {r} of {world} [{k.lo}, {k.hi}) stage {STAGES[s - 1]}"
            st = lib.kge_ship_step(desc, _lib.MODE_IDS[mode], C.byref(sd), s, None if adam is None else C.byref(adam),
                                   *rest)
            torch.cuda.synchronize(dev)
            assert st == 0, f"{what}: status {st} ({lib.kge_status_string(st).decode()})"
            flag = int(k.v["err"].item())
            assert err_ok or flag == 0, f"{what}: err_flag {flag}"
            for o in (ranks if s == _lib.SHIP_ENTITY and r == world - 1 else [k]):
                if int(o.dirty().item()):
                    o.explain(what)

    def all_sum(*names):
        for nm in names:
            tot = ranks[0].v[nm].clone()
            for k in ranks[1:]:
                tot += k.v[nm]
            for k in ranks:
                k.v[nm].copy_(tot)

    stage(_lib.SHIP_Q)
    all_sum(*(("q", "qp") if head else ("q",)))
    stage(_lib.SHIP_ROWS)
    parts = torch.stack([k.v["part"] for k in ranks])
    for k in ranks:
        k.v["parts"].copy_(parts)
    stage(_lib.SHIP_MERGE)
    g_merge = [k.v["g"].cpu() for k in ranks]
    all_sum(*(("dq", "pstats", "pq") if head else ("dq", "pstats")))
    stage(_lib.SHIP_CHAIN)
    row_stats = [k.v["row_stats"].cpu() for k in ranks]
    all_sum("gr")
    stage(_lib.SHIP_ENTITY)

    out = []
    for r, k in enumerate(ranks):
        v = k.v
        cpu = lambda t: None if t is None else t.detach().cpu().clone()  # noqa: E731
        o = RankOut(k.lo, k.hi, cpu(v["ge"]), cpu(v["gr"]), cpu(v["gm"]), cpu(v["losses"]), row_stats[r], g_merge[r],
                    cpu(v["ent"]), cpu(v["mod"]), err=int(v["err"].item()))
        for key, nm in (("em", "entity.m"), ("ev", "entity.v"), ("mm", "modulus.m"), ("mv", "modulus.v")):
            if key in v:
                o.moments[nm] = cpu(v[key])
        out.append(o)
    return out


def is_fill(t):
    """Every byte of the float32 tensor t is FLOAT_FILL."""
    return bool((t.contiguous().view(torch.uint8) == FLOAT_FILL).all())
