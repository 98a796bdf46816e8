"""CPU-only checks of the launch helpers in lpformer_amd/ops.py that need no launch: the row layout lpf_gemm_f32 wants
(``pad4``, ``f32_rows``) and the hub-row list of lpf_spmm_csr_* (``long_rows``)."""
import pytest
import torch

from lpformer_amd import _lib, graph, ops


def test_pad4():
    assert [ops.pad4(k) for k in (0, 1, 4, 5)] == [0, 4, 4, 8]


def _conforms(y):
    return (y.dtype == torch.float32 and y.dim() == 2 and y.stride(1) == 1 and y.stride(0) % 4 == 0 and
            y.stride(0) >= y.shape[1] and y.data_ptr() % 16 == 0 and not y.requires_grad)


def test_f32_rows_returns_a_conforming_tensor_as_it_is():
    x = torch.randn(3, 8)
    assert _conforms(x)
    y = ops.f32_rows(x)
    assert y.data_ptr() == x.data_ptr() and y.shape == x.shape and y.stride() == x.stride()
    v = torch.randn(5, 16)[:, 4:12]          # a strided view with aligned rows conforms too
    assert ops.f32_rows(v).data_ptr() == v.data_ptr()


def _cases():
    g = torch.Generator().manual_seed(0)
    return {"float64": torch.randn(3, 8, generator=g, dtype=torch.float64),
            "three_d": torch.randn(2, 3, 8, generator=g),
            "unaligned_view": torch.randn(3, 8, generator=g)[:, 1:],
            "row_stride_6": torch.randn(3, 6, generator=g),
            "requires_grad": torch.randn(3, 8, generator=g).requires_grad_()}


@pytest.mark.parametrize("name", sorted(_cases()))
def test_f32_rows_makes_the_layout(name):
    x = _cases()[name]
    y = ops.f32_rows(x)
    assert _conforms(y), (y.dtype, y.shape, y.stride(), y.data_ptr() % 16, y.requires_grad)
    want = x.detach().reshape(-1, x.shape[-1]).float()
    assert y.shape == want.shape and torch.equal(y, want)
    rows = torch.as_strided(y, (y.shape[0], y.stride(0)), (y.stride(0), 1))   # the rows with their padding columns
    assert torch.equal(rows[:, :y.shape[1]], want)
    if name in ("unaligned_view", "row_stride_6"):     # copies: what lies behind a row's last value is zero
        assert y.stride(0) == ops.pad4(y.shape[1]) > y.shape[1]
        assert not rows[:, y.shape[1]:].any()
    if name == "requires_grad":                        # detached, not copied
        assert y.data_ptr() == x.data_ptr()


def _csr(degrees):
    rowptr = torch.zeros(len(degrees) + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.tensor(degrees), 0)
    return graph.DeviceCSR(rowptr, torch.zeros(int(rowptr[-1]), dtype=torch.int32), None, len(degrees))


DEGREES = [127, 128, 129, 5, 400]     # hub rows (more than LPF_SPMM_LONG_ROW = 128 entries): 2 and 4


def test_long_rows_whole_graph_and_blocks():
    assert _lib.CONST["LPF_SPMM_LONG_ROW"] == 128
    a = _csr(DEGREES)
    whole = ops.long_rows(a)
    assert whole.dtype == torch.int32 and whole.tolist() == [2, 4]
    assert ops.long_rows(a, 0, 3).tolist() == [2]          # a block that cuts between the two ...
    assert ops.long_rows(a, 3, 5).tolist() == [1]          # ... and the other side: row 4, relative to lo = 3
    assert ops.long_rows(a, 0, 2) is None and ops.long_rows(a, 3, 4) is None
    assert ops.long_rows(_csr([128, 0, 1])) is None


def test_long_rows_is_computed_once_per_graph_and_block():
    a = _csr(DEGREES)
    first, block, none = ops.long_rows(a), ops.long_rows(a, 3, 5), ops.long_rows(a, 0, 2)
    assert ops.long_rows(a, 0, a.n) is first               # hi=None is the whole graph: one key
    a.rowptr = a.structure.rowptr = None                   # a second look at the degrees would raise
    assert ops.long_rows(a) is first and ops.long_rows(a, 3, 5) is block
    assert ops.long_rows(a, 0, 2) is none is None          # "no hub row" is cached too
    # the graph object holds its declared fields and nothing else; of the holder's memos, one kind is filled
    assert set(a.__dict__) == {"rowptr", "col", "val", "n", "host", "structure", "raw_val"}
    assert set(vars(a.structure)) == {"rowptr", "col", "n", "_long_rows", "_row_order", "_edge_keys", "_transposed"}
    assert set(a.structure._long_rows) == {(0, a.n), (3, 5), (0, 2)}
    assert a.structure._row_order == {} and a.structure._edge_keys is None and a.structure._transposed is None


def test_long_rows_threshold_is_the_headers(monkeypatch):
    monkeypatch.setitem(_lib.CONST, "LPF_SPMM_LONG_ROW", 399)
    assert ops.long_rows(_csr(DEGREES)).tolist() == [4]
    monkeypatch.setitem(_lib.CONST, "LPF_SPMM_LONG_ROW", 126)
    assert ops.long_rows(_csr(DEGREES)).tolist() == [0, 1, 2, 4]
