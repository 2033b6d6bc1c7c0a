"""Top-k link prediction on the device (kge_topk through ops.topk,
KGEModel.predict and torch.ops.kge.topk) against oracle.kge_oracle.forward in
float64 over all entities: checks (a)-(d) of topk_cases.check_result, the
bitwise invariances (parts, query batching, repetition), ties, filters,
padding and the index error.  E = 1003 (not a multiple of 64), K = 32.
"""
import numpy as np
import pytest
import torch

import topk_cases as T
from knowledgegraphembedding_amd import KGEModel, ops
from knowledgegraphembedding_amd.filters import FilterIndex

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PATHS = ("tile", "scan")


class Case:
    """One model's tables on the device and its descriptor."""

    def __init__(self, name, nentity=T.E, d=T.D, ties=False, misalign=False):
        ent, rel, mod = T.tables(name, nentity=nentity, d=d, ties=ties)
        self.name, self.np = name, (ent, rel, mod)
        if misalign:  # the table one float past a 16-byte boundary
            buf = torch.empty(ent.size + 1, dtype=torch.float32, device=DEV)
            self.ent = buf[1:].view(ent.shape)
            self.ent.copy_(torch.from_numpy(ent.copy()))
            assert self.ent.data_ptr() % 16 == 4
        else:
            self.ent = torch.from_numpy(ent.copy()).to(DEV)
        self.rel = torch.from_numpy(rel.copy()).to(DEV)
        self.mod = None if mod is None else torch.from_numpy(mod.copy()).to(DEV)
        self.desc = ops.make_desc(name, self.ent, self.rel, T.GAMMA, T.erange_of(d), self.mod)

    def topk(self, mode, q, k, **kw):
        ids, sc = ops.topk(self.desc, mode, torch.from_numpy(np.array(q, dtype=np.int64)), k, DEV, **kw)
        return ids.cpu().numpy(), sc.cpu().numpy()


_CASES = {}


def case(name, **kw):
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _CASES:
        _CASES[key] = Case(name, **kw)
    return _CASES[key]


def err_flag():
    return int(ops.state(DEV).err.item())


def dev_filter(mode):
    off, ids = T.csr_of(T.mask_of(mode))
    return torch.from_numpy(off).to(DEV), torch.from_numpy(ids).to(DEV)


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


# ---------------------------------------------------------------- the cases
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("name", T.NAMES)
def test_against_oracle(name, mode, path):
    c, q, s64 = case(name), T.queries(), T.s64_of(name, mode)
    none = np.zeros(s64.shape, dtype=bool)
    for k in T.KS:
        r = c.topk(mode, q, k, path=path)
        T.check_result(*r, s64, none, k, exact=k <= 10, what=f"{name} {mode} {path} k={k}")
        r = c.topk(mode, q, k, path=path, filt=dev_filter(mode))
        T.check_result(*r, s64, T.mask_of(mode), k, exact=k <= 10, what=f"{name} {mode} {path} k={k} filtered")
        one = c.topk(mode, q[:1], k, path=path)  # nq = 1
        T.check_result(*one, s64[:1], none[:1], k, exact=k <= 10, what=f"{name} {mode} {path} k={k} nq=1")
    assert err_flag() == 0


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("name", T.NAMES)
def test_scan_only_rows(name, mode):
    """Rows only the wave scan takes: hidden_dim 30 (K % 4 != 0) and a table
    one float past a 16-byte boundary; path "auto" picks the scan, "tile" is
    refused."""
    q = T.queries()
    for kw, d in ((dict(d=30), 30), (dict(misalign=True), T.D)):
        c = case(name, **kw)
        s64 = T.oracle_scores(name, *c.np, q, mode, d=d)
        none = np.zeros(s64.shape, dtype=bool)
        for k in (10, 128):
            r = c.topk(mode, q, k)
            T.check_result(*r, s64, none, k, exact=k <= 10, what=f"{name} {mode} {kw} k={k}")
            assert same(r, c.topk(mode, q, k, path="scan"))
        with pytest.raises(Exception, match="status 4"):
            c.topk(mode, q, 10, path="tile")
    assert err_flag() == 0


# ------------------------------------------------------------- invariances
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", T.NAMES)
def test_invariance(name, path):
    """Bitwise the same ids and scores whatever `parts`, however the queries
    are batched, and on repetition."""
    c, q = case(name), T.queries()
    for mode in T.MODES:
        for k in (10, 128):
            base = c.topk(mode, q, k, path=path, parts=1)
            for parts in (2, 16, 0):
                assert same(base, c.topk(mode, q, k, path=path, parts=parts)), (mode, k, parts)
            assert same(base, c.topk(mode, q, k, path=path, parts=1)), "two identical calls differ"
            a, b = c.topk(mode, q[:64], k, path=path), c.topk(mode, q[64:], k, path=path)
            assert same(base, (np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]))), "blocks of 64 + 66"
        k = 10
        base = c.topk(mode, q, k, path=path)
        ones = [c.topk(mode, q[i:i + 1], k, path=path) for i in range(len(q))]
        assert same(base, (np.concatenate([o[0] for o in ones]), np.concatenate([o[1] for o in ones]))), \
            "one query at a time"


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", T.NAMES)
def test_ties(name, path):
    """Five identical rows in different tiles (and parts): wherever the first
    is returned, the five come consecutively, in ascending id, with bit-equal
    scores."""
    c, q, k = case(name, ties=True), T.queries(), 128
    s64 = T.s64_of(name, "tail-batch", ties=True)
    none = np.zeros(s64.shape, dtype=bool)
    seen = 0
    for parts in (1, 2, 16):
        ids, sc = c.topk("tail-batch", q, k, path=path, parts=parts)
        T.check_result(ids, sc, s64, none, k, exact=False, what=f"{name} ties parts={parts}")
        for i in range(len(q)):
            at = np.nonzero(ids[i] == T.TIE_ROWS[0])[0]
            if len(at) == 0:
                assert not np.isin(ids[i], T.TIE_ROWS).any()
                continue
            p = int(at[0])
            n = min(5, k - p)
            assert ids[i, p:p + n].tolist() == list(T.TIE_ROWS[:n]), (name, path, parts, i)
            assert len(set(sc[i, p:p + n].view(np.uint32).tolist())) == 1
            seen += n == 5
    assert seen >= 3, "no query returned the tied rows: the case checks nothing"


# ------------------------------------------------------------------ filters
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ("TransE", "RotatE", "pRotatE"))
def test_filter_forms_agree(name, path):
    """Per-query lists and the whole filter index give identical results,
    with anything in the predicted column."""
    c = case(name)
    index = FilterIndex(T.true_triples(), T.E, T.R)
    for mode in T.MODES:
        q = T.queries().copy()
        q[:, 0 if mode == "head-batch" else 2] = -1
        tab = index.device_table(mode, DEV)
        assert tab is not None
        a = c.topk(mode, q, 64, path=path, filt=dev_filter(mode))
        b = c.topk(mode, q, 64, path=path, filt=tab, filter_table=True)
        assert same(a, b)
        assert not np.take_along_axis(T.mask_of(mode), a[0], 1).any()
    assert err_flag() == 0


@pytest.mark.parametrize("path", PATHS)
def test_filter_is_per_query(path):
    """An entity listed for query 0 but not for the identical query 1 still
    appears for query 1."""
    c, k = case("TransE"), 10
    q = np.repeat(T.queries()[:1], 2, axis=0)
    plain = c.topk("tail-batch", q, k, path=path)
    assert same((plain[0][:1], plain[1][:1]), (plain[0][1:], plain[1][1:]))
    listed = np.sort(plain[0][0, :5])
    off = torch.tensor([0, 5, 5], dtype=torch.int64)
    ids, sc = c.topk("tail-batch", q, k, path=path, filt=(off, torch.from_numpy(listed)))
    assert not np.isin(ids[0], listed).any()
    assert np.array_equal(ids[1], plain[0][1]) and np.array_equal(sc[1], plain[1][1])
    assert np.array_equal(ids[0, :5], plain[0][0, 5:])  # the rest moves up


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ("DistMult", "RotatE"))
def test_padding(name, path):
    """Fewer than k candidates: E = 100 with k = 128, and a list that leaves 3."""
    c = case(name, nentity=100)
    q = T.queries(8, 100)
    for mode in T.MODES:
        s64 = T.oracle_scores(name, *c.np, q, mode)
        none = np.zeros(s64.shape, dtype=bool)
        ids, sc = c.topk(mode, q, 128, path=path)
        T.check_result(ids, sc, s64, none, 128, exact=False, what=f"{name} E=100")
        assert (ids[:, 100:] == -1).all() and np.isneginf(sc[:, 100:]).all() and (ids[:, :100] >= 0).all()
        mask = np.ones(s64.shape, dtype=bool)
        for i in range(len(q)):
            mask[i, [(7 * i) % 100, (7 * i + 31) % 100, 99 - i]] = False
        off, lst = T.csr_of(mask)
        for k in (1, 10):
            ids, sc = c.topk(mode, q, k, path=path, filt=(torch.from_numpy(off), torch.from_numpy(lst)))
            T.check_result(ids, sc, s64, mask, k, exact=False, what=f"{name} three left k={k}")
            assert ((ids >= 0).sum(1) == min(k, 3)).all()


# -------------------------------------------------------------- index error
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("mode", T.MODES)
def test_index_error(mode, path):
    c, k = case("ComplEx"), 10
    q = T.queries().copy()
    clean = c.topk(mode, q, k, path=path, filt=dev_filter(mode))
    assert err_flag() == 0
    pred = 0 if mode == "head-batch" else 2
    for v in (-1, T.E + 5):  # the predicted column is neither read nor checked
        q2 = q.copy()
        q2[:, pred] = v
        assert same(clean, c.topk(mode, q2, k, path=path, filt=dev_filter(mode)))
        assert err_flag() == 0
    bad = q.copy()
    bad[77, 1] = T.R
    ids, sc = c.topk(mode, bad, k, path=path, filt=dev_filter(mode))
    assert err_flag() & 1
    with pytest.raises(IndexError):
        ops.raise_on_device_error(DEV)
    assert err_flag() == 0
    assert (ids[77] == -1).all() and np.isnan(sc[77]).all()
    keep = np.arange(len(q)) != 77
    assert same((ids[keep], sc[keep]), (clean[0][keep], clean[1][keep]))


# ------------------------------------------------- the Python and torch layers
def _model(name):
    de, dr = T.DOUBLE[name]
    m = KGEModel(name, T.E, T.R, T.D, T.GAMMA, de == 2, dr == 2)
    ent, rel, _ = T.tables(name)
    with torch.no_grad():
        m.entity_embedding.copy_(torch.from_numpy(ent.copy()))
        m.relation_embedding.copy_(torch.from_numpy(rel.copy()))
    return m.to(DEV)


@pytest.mark.parametrize("name", ("TransE", "pRotatE"))
def test_predict(name):
    m, q = _model(name), T.queries()
    for mode in T.MODES:
        want = case(name).topk(mode, q, 10, filt=dev_filter(mode))
        a = m.predict(q, mode, k=10, all_true_triples=T.true_triples())
        b = m.predict(q, mode, k=10, all_true_triples=FilterIndex(T.true_triples(), T.E, T.R))
        assert same(a, want) and same(b, want)
        assert same(m.predict(q, mode), case(name).topk(mode, q, 10))  # k = 10, no filter
    with pytest.raises(ValueError, match="mode single not supported"):
        m.predict(q, "single")
    for k in (0, 129):
        with pytest.raises(ValueError):
            m.predict(q, "tail-batch", k=k)
    bad = q.copy()
    bad[3, 1] = T.R
    with pytest.raises(IndexError):
        m.predict(bad, "tail-batch")
    assert err_flag() == 0


@pytest.mark.parametrize("name", ("DistMult", "RotatE", "pRotatE"))
def test_torch_op(name):
    from knowledgegraphembedding_amd import _lib, torch_ops
    torch_ops.load()
    c, q = case(name), torch.from_numpy(T.queries().copy()).to(DEV)
    for mode in T.MODES:
        off, ids = dev_filter(mode)
        for k, path in ((10, "auto"), (128, "scan")):
            want = c.topk(mode, T.queries(), k, path=path, filt=(off, ids))
            got = torch.ops.kge.topk(c.ent, c.rel, c.mod, q, off, ids, _lib.MODE_IDS[mode], _lib.MODEL_IDS[name],
                                     T.GAMMA, T.erange_of(T.D), k, ops.TOPK_PATHS[path])
            assert same((got[0].cpu().numpy(), got[1].cpu().numpy()), want)
        want = c.topk(mode, T.queries(), 10)
        got = torch.ops.kge.topk(c.ent, c.rel, c.mod, q, None, None, _lib.MODE_IDS[mode], _lib.MODEL_IDS[name],
                                 T.GAMMA, T.erange_of(T.D), 10)
        assert same((got[0].cpu().numpy(), got[1].cpu().numpy()), want)
    with pytest.raises(ValueError):
        torch.ops.kge.topk(c.ent, c.rel, c.mod, q, None, None, 0, _lib.MODEL_IDS[name], T.GAMMA, 0.4, 10)
    with pytest.raises(ValueError):
        torch.ops.kge.topk(c.ent, c.rel, c.mod, q, None, None, 2, _lib.MODEL_IDS[name], T.GAMMA, 0.4, 129)


def test_torch_op_meta():
    """The Meta kernel gives [nq, k] long and float without touching a device."""
    from knowledgegraphembedding_amd import torch_ops
    torch_ops.load()
    ent = torch.empty(T.E, 32, device="meta")
    rel = torch.empty(T.R, 32, device="meta")
    q = torch.empty(17, 3, dtype=torch.int64, device="meta")
    ids, sc = torch.ops.kge.topk(ent, rel, None, q, None, None, 2, 0, 12.0, 0.4, 7)
    assert ids.shape == (17, 7) and ids.dtype == torch.int64 and ids.device.type == "meta"
    assert sc.shape == (17, 7) and sc.dtype == torch.float32
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        e, r = torch.empty(T.E, 32, device="cuda"), torch.empty(T.R, 32, device="cuda")
        qq = torch.empty(5, 3, dtype=torch.int64, device="cuda")
        ids, sc = torch.ops.kge.topk(e, r, None, qq, None, None, 1, 1, 12.0, 0.4, 128)
        assert ids.shape == (5, 128) and sc.shape == (5, 128) and sc.dtype == torch.float32
