"""CPU-only checks of lpformer_amd.sources: the pair / id checks, the chunk helpers, the per-object cache, the numpy row
gather and the host-side branches of the source resolver."""
import gc

import numpy as np
import pytest
import torch

from lpformer_amd import _lib, graph, sources
from tests.golden_util import Fixture
from tests.test_host_logic import _model_for


def test_as_pairs_layouts():
    e = torch.arange(10).reshape(5, 2)
    assert torch.equal(sources.as_pairs(e), e.t())
    assert torch.equal(sources.as_pairs(e.t()), e.t())
    sq = torch.tensor([[0, 1], [2, 3]])
    assert torch.equal(sources.as_pairs(sq), sq)                       # [2, 2] reads as [2, P]
    assert sources.as_pairs(torch.zeros(0, 2, dtype=torch.int64)).shape == (2, 0)
    assert torch.equal(sources.as_pairs([[0, 1], [2, 3], [4, 5]]), torch.tensor([[0, 2, 4], [1, 3, 5]]))
    for bad in (torch.arange(4), torch.zeros(3, 3, dtype=torch.int64)):
        with pytest.raises(ValueError):
            sources.as_pairs(bad)


@pytest.mark.parametrize("exc", [ValueError, TypeError])
@pytest.mark.parametrize("dtype", [torch.float32, torch.complex64, torch.bool])
def test_ids_reject_non_integer_dtypes_with_the_callers_type(exc, dtype):
    with pytest.raises(exc):
        sources.as_pairs(torch.zeros(2, 3, dtype=dtype), exc=exc)
    with pytest.raises(exc):
        sources.node_ids(torch.zeros(3, dtype=dtype), "nodes", exc)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_integer_ids_pass_without_a_copy(dtype):
    e = torch.zeros(4, 2, dtype=dtype)
    assert sources.as_pairs(e).data_ptr() == e.data_ptr() == sources.as_pairs(e.t()).data_ptr()
    v = torch.zeros(4, dtype=dtype)
    assert sources.node_ids(v, "nodes") is v


def test_clamp_chunk():
    for bad in (0, -1):
        with pytest.raises(ValueError):
            sources.clamp_chunk(bad)
    assert sources.clamp_chunk(1) == 1
    assert sources.clamp_chunk(1 << 40) == (1 << 31) - 2


def test_chunks_cover_the_pairs_once_in_order():
    c = 7
    for P in (0, 1, c, c + 1, 3 * c):
        got = list(sources.chunks(P, c))
        assert all(1 <= m <= c for _, m in got)
        assert [i for lo, m in got for i in range(lo, lo + m)] == list(range(P))


def test_csr_rows_against_a_loop():
    rowptr = np.array([0, 2, 2, 5, 6, 6, 9], np.int64)                 # 6 nodes; rows 1 and 4 are empty
    for nodes in ([2, 0, 2, 1, 5], [4], []):
        nodes = np.array(nodes, np.int64)
        flat, pos = sources.csr_rows(rowptr, nodes)
        want = [(e, i) for i, u in enumerate(nodes) for e in range(rowptr[u], rowptr[u + 1])]
        assert flat.dtype == pos.dtype == np.int64
        assert list(zip(flat.tolist(), pos.tolist())) == want


def test_per_object_cache():
    class Obj:
        def __eq__(self, other):
            return True
        __hash__ = None
    cache, made = {}, []

    def make():
        made.append(object())
        return made[-1]
    a, b = Obj(), Obj()
    va = sources.per_object(cache, a, make)
    assert sources.per_object(cache, a, make) is va and len(made) == 1
    assert sources.per_object(cache, b, make) is not va and len(made) == 2    # equal, but another object
    assert len(cache) == 2
    del a
    gc.collect()
    assert len(cache) == 1 and sources.per_object(cache, b, make) is made[1]


def _tiny(n_ppr=3, val=True):
    return (graph.CSR(np.array([0, 1, 2, 2], np.int64), np.array([1, 0], np.int32), None, 3),
            graph.CSR(np.arange(n_ppr + 1, dtype=np.int64), np.arange(n_ppr, dtype=np.int32),
                      np.ones(n_ppr, np.float32) if val else None, n_ppr))


def test_resolve_rejects_bad_sources():
    like = torch.zeros(2, 3, dtype=torch.int64)
    adj, ppr = _tiny()
    for bad in ("a graph", np.eye(3), (adj, ppr)):                     # (a tuple is a source with pieces=True only)
        with pytest.raises(TypeError):
            sources.resolve(bad, False, like, who="t")
    for bad in ((adj, "ppr"), (adj,), (adj, ppr, None, None)):
        with pytest.raises(TypeError):
            sources.resolve(bad, False, like, who="t", pieces=True)
    with pytest.raises(ValueError):
        sources.resolve(_tiny(n_ppr=4), False, like, who="t", pieces=True, host_ok=True)
    with pytest.raises(ValueError):
        sources.resolve(_tiny(val=False), False, like, who="t", pieces=True, host_ok=True)
    on_cpu = adj.to_device("cpu")
    with pytest.raises(_lib.LpfError, match="^t:"):
        sources.resolve(on_cpu, False, like, who="t", host_ok=True)


def test_resolve_host_path(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    like = torch.zeros(2, 3, dtype=torch.int64)
    adj, ppr = _tiny()
    x = torch.zeros(3, 4)
    assert sources.resolve(adj, False, like, who="t", host_ok=True) == (None, adj, None, None)
    got = sources.resolve((adj, ppr, x), False, like, who="t", pieces=True, host_ok=True)
    assert got[0] is None and got[1] is adj and got[2] is ppr and got[3] is x
    got = sources.resolve([adj, ppr], False, like, who="t", pieces=True, host_ok=True)
    assert got[0] is None and got[1] is adj and got[2] is ppr and got[3] is None
    with pytest.raises(_lib.LpfError, match="^t needs"):
        sources.resolve(adj, False, like, who="t")


def test_cpu_model_error_names_the_caller():
    model = _model_for(Fixture("lp_all_d64"))
    like = torch.zeros(2, 3, dtype=torch.int64)
    for call in (lambda: sources.model_graphs(model, False, "some_entry"),
                 lambda: sources.resolve(model, False, like, who="some_entry", host_ok=True)):
        with pytest.raises(_lib.LpfError) as err:
            call()
        assert str(err.value).startswith("some_entry")
