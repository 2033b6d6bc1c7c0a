"""torch.ops.kge.rank_relations: registered from the C++ library with CUDA, Meta
and CPU kernels; the Meta kernel's shapes and dtypes (CPU); on the device, the
same ranks, ties and scores as ops.rank_relations."""
import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from knowledgegraphembedding_amd.torch_ops import MODEL_IDS  # (loads libkge_torch.so)

ROTATE = MODEL_IDS["RotatE"]


def test_registered():
    for key in ("CUDA", "Meta", "CPU"):
        assert torch._C._dispatch_has_kernel_for_dispatch_key("kge::rank_relations", key), key
    schema = str(torch.ops.kge.rank_relations.default._schema)
    assert schema.startswith("kge::rank_relations(") and "Tensor? filt_off, Tensor? filt_ids" in schema
    assert "Tensor? relation_trig=None" in schema and "bool with_scores=False" in schema
    assert "int mode," not in schema and "int model," in schema  # there is no mode argument
    assert schema.endswith("-> (Tensor, Tensor, Tensor)")


def test_meta_shapes_and_dtypes():
    with FakeTensorMode():
        ent, rel = torch.empty(100, 32), torch.empty(7, 16)
        q = torch.empty(8, 3, dtype=torch.int64)
        r, t, s = torch.ops.kge.rank_relations(ent, rel, None, q, None, None, ROTATE, 12.0, 0.875)
        assert r.shape == (8,) and r.dtype == torch.int64
        assert t.shape == (8,) and t.dtype == torch.int32
        assert s.shape == (0, 7) and s.dtype == torch.float32
        off, ids = torch.empty(9, dtype=torch.int64), torch.empty(20, dtype=torch.int64)
        r, t, s = torch.ops.kge.rank_relations(ent, rel, None, q, off, ids, ROTATE, 12.0, 0.875, torch.empty(7, 2, 16),
                                               True)
        assert r.shape == (8,) and t.shape == (8,) and s.shape == (8, 7) and s.dtype == torch.float32
    ent, rel = torch.empty(100, 32, device="meta"), torch.empty(7, 16, device="meta")
    q = torch.empty(0, 3, dtype=torch.int64, device="meta")
    r, t, s = torch.ops.kge.rank_relations(ent, rel, None, q, None, None, ROTATE, 12.0, 0.875, None, True)
    assert r.shape == (0,) and r.device.type == "meta" and t.dtype == torch.int32 and s.shape == (0, 7)


def test_reference_errors_and_no_cpu_path():
    ent, rel = torch.zeros(10, 8), torch.zeros(3, 4)
    q = torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="model 7 not supported"):
        torch.ops.kge.rank_relations(ent, rel, None, q, None, None, 7, 12.0, 0.5)
    with pytest.raises(ValueError, match="model 7 not supported"):
        torch.ops.kge.rank_relations(ent.to("meta"), rel.to("meta"), None, q.to("meta"), None, None, 7, 12.0, 0.5)
    with pytest.raises(RuntimeError, match="ROCm"):
        torch.ops.kge.rank_relations(ent, rel, None, q, None, None, ROTATE, 12.0, 0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("name,d", [("RotatE", 20), ("DistMult", 40), ("pRotatE", 40)])
def test_equals_ops(name, d):
    import rank_relations_cases as K
    from knowledgegraphembedding_amd import ops
    from test_rank_relations_gpu import DEV, make

    case = next(c for c in K.BASE if (c.name, c.d) == (name, d))
    m = make(case)
    q = torch.from_numpy(K.queries(case).copy()).to(DEV)
    off, ids = (torch.from_numpy(x.copy()).to(DEV) for x in K.filt(case))
    trig = m._rank_rotation(DEV)
    _, erange = m._host_scalars()
    tables = (m.entity_embedding.detach(), m.relation_embedding.detach(),
              m.modulus.detach() if name == "pRotatE" else None)
    for filt in (None, (off, ids)):
        want = ops.rank_relations(m.desc(), q, DEV, filt=filt, relation_trig=trig, scores=True)
        f = filt or (None, None)
        got = torch.ops.kge.rank_relations(*tables, q, f[0], f[1], MODEL_IDS[name], K.GAMMA, erange, trig, True)
        assert got[0].dtype == torch.int64 and got[1].dtype == torch.int32 and got[2].dtype == torch.float32
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert torch.equal(got[2].view(torch.int32), want[2].view(torch.int32))
        # against the oracle, pRotatE too (its inputs excuse no query: test_rank_relations_ref.py)
        ref = K.reference(case, filt is not None)
        assert np.array_equal(got[0].cpu().numpy(), ref[0]) and np.array_equal(got[1].cpu().numpy(), ref[1])
        assert np.array_equal(got[2].cpu().numpy().view(np.int32), K.scores(case).view(np.int32))
        bare = torch.ops.kge.rank_relations(*tables, q, f[0], f[1], MODEL_IDS[name], K.GAMMA, erange, trig)
        assert torch.equal(bare[0], want[0]) and torch.equal(bare[1], want[1]) and bare[2].shape == (0, case.R)
    with pytest.raises(ValueError):
        torch.ops.kge.rank_relations(*tables, q, off, None, MODEL_IDS[name], K.GAMMA, erange, trig)
    with pytest.raises(ValueError):
        torch.ops.kge.rank_relations(*tables, q, off[:-1], ids, MODEL_IDS[name], K.GAMMA, erange, trig)
    ops.raise_on_device_error(DEV)
