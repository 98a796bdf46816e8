"""The launch helpers of lpformer_amd/ops.py on the device: what can go wrong here is argument plumbing, so every case
is tiny and most are BITWISE comparisons -- with a direct ctypes call on the same operands, or with the one fp32
operation per element that torch does too."""
import pytest
import torch

from lpformer_amd import _lib, graph, ops
from lpformer_amd.graphed import _StepRecorder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _gemm_direct(a, w, bias, addend, relu, out):
    """lpf_gemm_f32 on prepared operands, no wrapper in between."""
    m, k = a.shape
    _lib.check(_lib.hip().lpf_gemm_f32(m, w.shape[0], k, a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0),
                                       _lib.ptr(bias), _lib.ptr(addend), 0 if addend is None else addend.stride(0),
                                       out.data_ptr(), out.stride(0), _lib.FLAG_RELU if relu else 0, _stream()),
               "lpf_gemm_f32")
    return out


@pytest.mark.parametrize("m,n,k,how", [(33, 12, 20, "bias"), (5, 8, 8, "addend_relu_out"), (4100, 8, 8, "rows_kernel")])
def test_gemm_is_the_direct_call(m, n, k, how):
    a, w = ops.f32_rows(_rand(m, k, seed=1)), ops.f32_rows(_rand(n, k, seed=2))
    bias, add = _rand(n, seed=3), _rand(m, n, seed=4)
    if how == "addend_relu_out":
        buf = torch.full((m, n + 8), 7.0, device=DEV)
        got = ops.gemm(a, w, addend=add, relu=True, out=buf[:, 4:4 + n])        # a strided view, rows 16-byte aligned
        assert got.data_ptr() == buf[:, 4:].data_ptr() and got.stride(0) == n + 8
        assert (buf[:, :4] == 7.0).all() and (buf[:, 4 + n:] == 7.0).all()     # nothing written around it
        want = _gemm_direct(a, w, None, add, True, torch.empty(m, n, device=DEV))
        assert (got >= 0).all() and (got == 0).any()
    else:
        got = ops.gemm(a, w, bias)
        assert got.shape == (m, n) and got.stride(0) == ops.pad4(n)
        want = _gemm_direct(a, w, bias, None, False, torch.empty(m, n, device=DEV))
    assert torch.equal(got, want)


def test_gemm_pads_both_operands():
    """(5, 6, 7): neither k nor n is a multiple of 4 -- a, w and the result are all laid out by the wrapper."""
    m, n, k = 5, 6, 7
    a, w, bias = _rand(m, k, seed=5), _rand(n, k, seed=6), _rand(n, seed=7)
    out = ops.gemm(a, w, bias)
    ref = a.double() @ w.double().T + bias.double()
    err = (out.double() - ref).abs().max().item()
    print(f"gemm (5, 6, 7): max |out - fp64| = {err:.3e}")
    assert out.shape == (m, n) and err <= 2e-5 * max(1.0, k ** 0.5)


class _Count:
    """A recorder that only counts the launches (``_lib.recording``)."""

    def __init__(self):
        self.names = []

    def launch(self, name, fn):
        self.names.append(name)
        return fn

    def keep(self, t):
        pass

    def wait(self, a, b):
        pass


def test_gemm_edge_cases_launch_nothing():
    bias = _rand(8, seed=8)
    with _lib.recording(_Count()) as rec:
        assert ops.gemm(torch.empty(0, 8, device=DEV), _rand(8, 8), bias).shape == (0, 8)
        assert ops.gemm(_rand(5, 8), torch.empty(0, 8, device=DEV)).shape == (5, 0)
        zeros = ops.gemm(torch.empty(5, 0, device=DEV), torch.empty(8, 0, device=DEV))
        rows = ops.gemm(torch.empty(5, 0, device=DEV), torch.empty(8, 0, device=DEV), bias)
    assert rec.names == []
    assert zeros.shape == (5, 8) and not zeros.any()
    assert torch.equal(rows, bias.expand(5, 8))


def _pairs():
    return torch.tensor([[0, 3, 6, 3, 5], [1, 3, 0, 2, 6]], dtype=torch.int64, device=DEV)   # node 3 repeats; (3, 3): a == b


@pytest.mark.parametrize("which", ["product", "sum", "both"])
def test_pair_gather(which):
    x, batch = _rand(7, 8, seed=9), _pairs()
    prod = torch.full((5, 8), 7.0, device=DEV) if which != "sum" else None
    tot = torch.full((5, 8), 7.0, device=DEV) if which != "product" else None
    ops.pair_gather(x, batch, product=prod, sum=tot)
    if prod is not None:
        assert torch.equal(prod, x[batch[0]] * x[batch[1]])
    if tot is not None:
        assert torch.equal(tot, x[batch[0]] + x[batch[1]])


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("in_place", [True, False])
def test_layernorm(relu, in_place):
    x, g, b = _rand(3, 32, seed=10), _rand(32, seed=11), _rand(32, seed=12)
    ref = torch.nn.functional.layer_norm(x, (32,), g, b)
    ref = torch.relu(ref) if relu else ref
    src = x.clone()
    if in_place:
        out = ops.layernorm_(src, g, b, relu=relu)
        assert out is src
    else:
        dst = torch.full((3, 36), 7.0, device=DEV)
        out = ops.layernorm_(src, g, b, relu=relu, out=dst[:, :32])
        assert torch.equal(src, x) and (dst[:, 32:] == 7.0).all()
    err = (out - ref).abs().max().item()
    print(f"layernorm relu={relu} in_place={in_place}: max |out - torch| = {err:.3e}")
    assert err <= 2e-5


def test_spmm_is_the_direct_call():
    """A row block [lo, hi) with a hub row in it, every epilogue input given: the wrapper's launch against the same
    launch spelled out."""
    n, d, lo, hi = 40, 32, 8, 37
    g = torch.Generator().manual_seed(13)
    deg = torch.randint(0, 6, (n,), generator=g)
    deg[20] = 300                                                       # a hub row inside the block
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    nnz = int(rowptr[-1])
    a = graph.DeviceCSR(rowptr.to(DEV), torch.randint(0, n, (nnz,), generator=g).to(torch.int32).to(DEV),
                        torch.rand(nnz, generator=g).to(DEV), n)
    t, res, bias = _rand(n, d, seed=14), _rand(hi - lo, d, seed=15), _rand(d, seed=16)
    ln, fin = torch.nn.LayerNorm(d).to(DEV), torch.nn.LayerNorm(d).to(DEV)
    with torch.no_grad():
        for p, s in zip((ln.weight, ln.bias, fin.weight, fin.bias), (17, 18, 19, 20)):
            p.copy_(_rand(d, seed=s))
    got = ops.spmm(a, t, lo, hi, bias=bias, ln=ln, res=res, final_ln=fin, relu=True)
    hubs = ops.long_rows(a, lo, hi)
    assert hubs.tolist() == [20 - lo]
    want = torch.empty(hi - lo, d, device=DEV)
    _lib.check(_lib.hip().lpf_spmm_csr_f32(
        hi - lo, d, a.rowptr.data_ptr() + 8 * lo, a.col.data_ptr(), a.val.data_ptr(), t.data_ptr(), d, want.data_ptr(), d,
        bias.data_ptr(), ln.weight.data_ptr(), ln.bias.data_ptr(), res.data_ptr(), d, fin.weight.data_ptr(),
        fin.bias.data_ptr(), _lib.FLAG_RELU, hubs.data_ptr(), 1, _stream()), "lpf_spmm_csr_f32")
    assert torch.equal(got, want)
    plain = ops.spmm(a, t)                                              # the training form: whole graph, no epilogue
    want = torch.empty(n, d, device=DEV)
    _lib.check(_lib.hip().lpf_spmm_csr_f32(
        n, d, a.rowptr.data_ptr(), a.col.data_ptr(), a.val.data_ptr(), t.data_ptr(), d, want.data_ptr(), d, None, None,
        None, None, 0, None, None, 0, ops.long_rows(a).data_ptr(), 1, _stream()), "lpf_spmm_csr_f32")
    assert ops.long_rows(a).tolist() == [20] and torch.equal(plain, want)


def test_recording_sees_the_wrappers():
    """What PlannedScorer relies on: a wrapper called inside ``_lib.recording`` leaves its launch (entry point and
    arguments) and its tensors with the recorder, and calling the recorded launches again gives the same bits."""
    a, w, bias = _rand(33, 20, seed=21), _rand(12, 20, seed=22), _rand(12, seed=23)
    x, batch = _rand(7, 8, seed=24), _pairs()
    tot = torch.empty(5, 8, device=DEV)
    with _lib.recording(_StepRecorder(frozenset())) as rec:
        out = ops.gemm(a, w, bias)
        ops.pair_gather(x, batch, sum=tot)
    assert [name for name, _, _ in rec.calls] == ["lpf_gemm_f32", "lpf_pair_gather_f32"]
    kept = {t.data_ptr() for t in rec.kept}
    assert {t.data_ptr() for t in (a, w, bias, out, x, batch, tot)} <= kept
    want = (out.clone(), tot.clone())
    assert torch.equal(want[1], x[batch[0]] + x[batch[1]])
    out.zero_()
    tot.zero_()
    for name, fn, args in rec.calls:
        _lib.check(fn(*args), name)
    torch.cuda.synchronize()
    assert torch.equal(out, want[0]) and torch.equal(tot, want[1])
