"""CPU-only checks of ``graph.Structure``: the tables derived from a ``DeviceCSR``'s structure are made once and shared,
by construction, by every graph on that structure (``DeviceCSR.with_values``) -- and of ``graph.as_coo_on``."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from lpformer_amd import graph, mask_delta, ops, train

N = 301                     # no multiple of 16
HUBS = {7: 200, 150: 140}   # above LPF_SPMM_LONG_ROW = 128 and above the fused layer's hub threshold of 64


def _arrays():
    """A directed graph: two hub rows, rows 20 .. 39 and the last one empty, the others 0 .. 6 entries; fp32 values."""
    rng = np.random.default_rng(0)
    deg = rng.integers(0, 7, N)
    deg[20:40] = 0
    deg[N - 1] = 0
    for r, d in HUBS.items():
        deg[r] = d
    col = np.concatenate([np.sort(rng.choice(N, d, replace=False)) for d in deg]).astype(np.int32)
    rowptr = np.zeros(N + 1, np.int64)
    np.cumsum(deg, out=rowptr[1:])
    return torch.from_numpy(rowptr), torch.from_numpy(col), torch.from_numpy(rng.random(col.size, dtype=np.float32))


def _pair():
    rowptr, col, val = _arrays()
    a = graph.DeviceCSR(rowptr, col, val, N)
    return a, a.with_values(torch.from_numpy(np.random.default_rng(1).random(col.numel(), dtype=np.float32)))


def test_with_values_shares_every_derived_table_by_identity():
    a, b = _pair()
    assert b.rowptr is a.rowptr and b.col is a.col and b.val is not a.val and b.structure is a.structure
    assert ops.long_rows(a).tolist() == sorted(HUBS) and ops.long_rows(b) is ops.long_rows(a)
    assert ops.long_rows(a, 100, 200).tolist() == [50] and ops.long_rows(b, 100, 200) is ops.long_rows(a, 100, 200)
    for pad in (False, True):
        assert b.structure.row_order(0, N, pad) is a.structure.row_order(0, N, pad)
    assert a.structure.row_order(0, N, False) is not a.structure.row_order(0, N, True)
    keys = a.structure.edge_keys()
    assert b.structure.edge_keys() is keys and torch.equal(keys, mask_delta.edge_keys(a.rowptr, a.col, N))
    assert keys.dtype == torch.int64 and bool((keys[1:] > keys[:-1]).all())
    assert "structure" not in repr(a) and "raw_val" not in repr(a)


def test_row_order_is_computed_once_per_block_and_padding(monkeypatch):
    """Through ``a``, then ``b``, then the evaluation-style caller (``LinkTransformer._layer_fused``: keyword
    ``pad_hubs``, the precision flag) and the training-style one (``train._fused_layer``: the whole graph, no flag)."""
    a, b = _pair()
    calls = []
    real = graph.fused_row_order
    monkeypatch.setattr(graph, "fused_row_order", lambda *args, **kw: calls.append((args[1:], kw)) or real(*args, **kw))
    for g in (a, b):
        g.structure.row_order(0, N, True)
        g.structure.row_order(16, 160, False)
        first = g.structure.row_order(0, N, pad_hubs=False)      # evaluation, fp32
        assert g.structure.row_order(0, N) is first              # training
    assert sorted(c[0] for c in calls) == [(0, N), (0, N), (16, 160)] and len(a.structure._row_order) == 3
    assert sorted(c[1]["pad_hubs"] for c in calls) == [False, False, True]
    order, hubs, parts = first
    assert sorted(hubs[:, 0].tolist()) == sorted(HUBS) and order.numel() % 16 == 0 and parts.shape[0] == 2


def test_transposed_structure_is_shared_and_values_follow_the_permutation():
    a, b = _pair()
    at, bt = train._transpose_csr(a), train._transpose_csr(b)
    assert train._transpose_csr(a) is at and train._transpose_csr(b) is bt and bt is not at      # kept per graph object
    assert bt.rowptr is at.rowptr and bt.col is at.col and bt.structure is at.structure is a.structure.transposed()[0]
    fresh = train._transpose_csr(graph.DeviceCSR(b.rowptr.clone(), b.col.clone(), b.val.clone(), N))
    assert torch.equal(bt.val, fresh.val) and torch.equal(bt.col, fresh.col) and torch.equal(bt.rowptr, fresh.rowptr)
    want = sp.csr_matrix((b.val.numpy(), b.col.numpy(), b.rowptr.numpy()), shape=(N, N)).T.tocsr()
    want.sort_indices()
    assert np.array_equal(want.indptr, bt.rowptr.numpy()) and np.array_equal(want.indices, bt.col.numpy())
    assert np.array_equal(want.data, bt.val.numpy())
    # the transposed graphs share THEIR row order and hub list too (column 7 .. of a: whatever rows are long there)
    assert bt.structure.row_order(0, N) is at.structure.row_order(0, N)
    assert ops.long_rows(bt) is ops.long_rows(at)
    assert ops.long_rows(at, 0, 16) is ops.long_rows(bt, 0, 16)


def test_a_graph_built_fresh_from_the_same_arrays_shares_nothing():
    a, _ = _pair()
    c = graph.DeviceCSR(a.rowptr, a.col, a.val, N)
    assert c.structure is not a.structure
    assert ops.long_rows(c) is not ops.long_rows(a) and torch.equal(ops.long_rows(c), ops.long_rows(a))
    assert c.structure.row_order(0, N) is not a.structure.row_order(0, N)
    assert c.structure.edge_keys() is not a.structure.edge_keys()
    assert train._transpose_csr(c).rowptr is not train._transpose_csr(a).rowptr


def test_gcn_norm_result_declares_its_raw_weights():
    a, b = _pair()
    assert a.raw_val is None and b.raw_val is None
    g = a.with_values(b.val, raw_val=a.val)
    assert g.raw_val is a.val and g.structure is a.structure and g.host is None


class _Coo:
    """A ``torch_sparse.SparseTensor`` look-alike."""

    def __init__(self, row, col, val, n):
        self._coo, self._n = (row, col, val), n

    def coo(self):
        return self._coo

    def sparse_sizes(self):
        return (self._n, self._n)


def test_as_coo_on():
    rowptr, col, val = _arrays()
    rows = torch.repeat_interleave(torch.arange(N), rowptr[1:] - rowptr[:-1])
    cpu, other = torch.device("cpu"), torch.device("meta")       # (meta: a device the containers below do NOT live on)
    # a look-alike ON the target device: as_coo_device's answer, the container's own tensors by identity
    on = _Coo(rows, col.long(), val, N)
    got, dev = graph.as_coo_on(on, cpu), graph.as_coo_device(on, cpu)
    assert got[0] is dev[0] is rows and got[1] is dev[1] is on.coo()[1] and got[3] == dev[3] == N
    assert torch.equal(got[2], val) and graph.as_coo_on(_Coo(rows, col.long(), None, N), cpu)[2] is None
    # ... and OFF it: as_coo_device has no answer, the arrays of as_coo_numpy go to the target device
    assert graph.as_coo_device(on, other) is None
    got, host = graph.as_coo_on(on, other), graph.as_coo_numpy(on)
    assert all(g.device == other and g.shape == h.shape and g.dtype == torch.from_numpy(h).dtype
               for g, h in zip(got[:3], host[:3])) and got[3] == host[3] == N
    # a torch sparse COO tensor on the target device: the device path (coalesced)
    t = torch.sparse_coo_tensor(torch.stack([rows, col.long()]).flip(1), val.flip(0), (N, N))
    for g, d in zip(graph.as_coo_on(t, cpu)[:3], graph.as_coo_device(t, cpu)[:3]):
        assert torch.equal(g, d)
    assert torch.equal(graph.as_coo_on(t, cpu)[0], rows) and graph.as_coo_on(t, cpu)[3] == N
    # host containers: the values of as_coo_numpy, as tensors
    for obj in (graph.CSR(rowptr.numpy(), col.numpy(), val.numpy(), N), graph.CSR(rowptr.numpy(), col.numpy(), None, N),
                sp.coo_matrix((val.numpy(), (rows.numpy(), col.numpy())), shape=(N, N))):
        assert graph.as_coo_device(obj, cpu) is None
        got, host = graph.as_coo_on(obj, cpu), graph.as_coo_numpy(obj)
        assert got[3] == host[3] == N and (got[2] is None) == (host[2] is None)
        for g, h in zip(got[:3], host[:3]):
            assert h is None or (g.dtype == torch.from_numpy(h).dtype and np.array_equal(g.numpy(), h))
        assert graph.as_coo_on(obj, cpu, values=False)[2] is None
    for bad in (object(), torch.zeros(3, 3), [[0, 1], [1, 0]]):
        with pytest.raises(TypeError):
            graph.as_coo_on(bad, cpu)
