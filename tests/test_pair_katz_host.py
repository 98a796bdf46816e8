"""pair_walks / pair_katz without a GPU: the numpy restatement (walks_reference, what the entry points run for a host
graph.CSR with CPU edges when no GPU is present) against scipy's A @ A row products, the Katz arithmetic, argument
validation and the C ABI registration.  The walk counts have no tolerance."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import lpformer_amd
from lpformer_amd import _lib, katz
from lpformer_amd.katz import check_range, katz_from_walks, pair_katz, pair_walks, walks_reference
from tests import pair_katz_cases as KC


def _t(pairs):
    return torch.from_numpy(np.array(pairs, dtype=np.int64))


def _host(case, pairs, **kw):
    """Through the public function where it takes the host path (no GPU present), else the restatement itself."""
    fn = walks_reference if torch.cuda.is_available() else pair_walks
    out = fn(case.csr, _t(pairs), **kw)
    assert out.dtype == torch.int64 and not out.is_cuda
    assert out.shape == (np.asarray(pairs).shape[1], kw.get("max_len", 3))
    return out.numpy()


def test_batches_cover_what_the_tests_rely_on():
    for name in ("S", "H", "C"):
        c, w = KC.case(name), KC.exact(name)                                  # (exact() asserts the share condition)
        assert c.pairs.shape[1] == 4 * KC.WALK_PAIRS + 256 + 64 + 2 * KC.RUN + (2 if name == "C" else 3) + 4
        assert (w[c.edges, 0] == 1).all()                                     # the 64 stored edges
        wi = KC.exact_ignore_direct(name)
        assert (wi[c.edges, 0] == 0).all() and (wi[w[:, 0] == 0] == w[w[:, 0] == 0]).all()
        assert (w[-4:] == 0).all()                                            # ids of -1 and n
        print(name, "shares (W_3 > 0, W_4 > W_3 > 0):", KC.shares(name), "largest:", w.max(axis=0))
    h = KC.case("H")
    deg = np.diff(h.A.indptr)
    hub, leaf, iso = h.pairs[0, -7:-4]
    assert deg[hub] == 603 and deg[leaf] == 1 and deg[iso] == 0
    np.testing.assert_array_equal(KC.exact("H")[-7:-4, :2], [[0, 603], [0, 1], [0, 0]])   # W_2(a, a) = deg(a)


@pytest.mark.parametrize("ignore_direct", [False, True])
@pytest.mark.parametrize("max_len", KC.MAX_LENS)
@pytest.mark.parametrize("name", ["S", "H", "C"])
def test_numpy_path_matches_scipy(name, max_len, ignore_direct):
    c = KC.case(name)
    ref = KC.exact_ignore_direct(name) if ignore_direct else KC.exact(name)
    got = _host(c, c.pairs, max_len=max_len, ignore_direct=ignore_direct)
    np.testing.assert_array_equal(got, ref[:, :max_len])


@pytest.mark.parametrize("name", ["S", "H", "C"])
def test_swapped_pairs_are_equal(name):
    c = KC.case(name)
    sub = c.pairs[:, ::4]                      # every part of the batch, a quarter of each
    np.testing.assert_array_equal(_host(c, sub[::-1], max_len=4), KC.exact(name)[::4])
    np.testing.assert_array_equal(_host(c, sub[::-1], max_len=4, ignore_direct=True), KC.exact_ignore_direct(name)[::4])


def test_stored_self_loops_count():
    c = KC.case("S")
    A = c.A.tolil(copy=True)
    A.setdiag(1.0)
    A = A.tocsr()
    A.sort_indices()
    csr = lpformer_amd.graph.CSR(A.indptr.astype(np.int64), A.indices.astype(np.int32), None, c.n)
    looped = KC.Case(c.n, A, csr, c.pairs, c.hub, c.edges)
    sub = c.pairs[:, ::3]
    ref = KC.scipy_walks(A, sub)
    assert (ref != KC.exact("S")[::3]).any()
    np.testing.assert_array_equal(_host(looped, sub, max_len=4), ref)
    # a == b under ignore_direct: the skipped entry is the self-loop
    same = np.array([[7, 11], [7, 11]])
    cut = KC.WithoutEdge(A)
    want = np.stack([cut.counts(7, 7), cut.counts(11, 11)])
    np.testing.assert_array_equal(_host(looped, same, max_len=4, ignore_direct=True), want)


def _numpy_katz(w, beta):
    acc = w[:, 0].astype(np.float64) * np.float64(beta ** 1)
    for l in range(1, w.shape[1]):
        acc = acc + w[:, l].astype(np.float64) * np.float64(beta ** (l + 1))
    return acc.astype(np.float32)


@pytest.mark.parametrize("beta", [0.005, 0.05, 0.37])
def test_katz_from_walks(beta):
    for name in ("S", "H", "C"):
        for L in KC.MAX_LENS:
            w = KC.exact(name)[:, :L].copy()
            got = katz_from_walks(torch.from_numpy(w), beta)
            assert got.dtype == torch.float32 and got.shape == (w.shape[0],)
            assert np.array_equal(got.numpy().view(np.uint32), _numpy_katz(w, beta).view(np.uint32))
    # the fp64 sum before the final rounding against exact rational arithmetic (beta as the float it is)
    w = KC.exact("C")
    rows = np.unique(np.concatenate([np.argsort(w[:, 3])[-50:], np.arange(0, w.shape[0], 37)]))
    acc = w[rows, 0].astype(np.float64) * (beta ** 1)
    for l in range(1, 4):
        acc = acc + w[rows, l].astype(np.float64) * (beta ** (l + 1))
    b = Fraction(beta)
    for r, got in zip(rows, acc):
        want = sum(int(w[r, l]) * b ** (l + 1) for l in range(4))
        assert abs(Fraction(float(got)) - want) <= Fraction(1, 10 ** 12) * want
    # float32 rounding of the same: within half an ulp of fp32 of the exact value
    k = katz_from_walks(torch.from_numpy(w[rows].copy()), beta).numpy()
    for r, got in zip(rows, k):
        want = float(sum(int(w[r, l]) * b ** (l + 1) for l in range(4)))
        assert abs(float(got) - want) <= 2.0 ** -23 * want


def test_host_fallback_returns_cpu_tensors():
    c = KC.case("H")
    sub = _t(c.pairs[:, ::5])
    if torch.cuda.is_available():       # the entry points answer on the device there (tests/test_gpu_pair_katz.py)
        w = walks_reference(c.csr, sub, max_len=4)
        k = katz_from_walks(w, 0.01)
    else:
        w = pair_walks(c.csr, sub, max_len=4)
        k = pair_katz(c.csr, sub, max_len=4, beta=0.01)
    assert not w.is_cuda and w.dtype == torch.int64 and not k.is_cuda and k.dtype == torch.float32
    np.testing.assert_array_equal(w.numpy(), KC.exact("H")[::5])
    assert torch.equal(k, katz_from_walks(w, 0.01))
    fn = walks_reference if torch.cuda.is_available() else pair_walks
    np.testing.assert_array_equal(fn(c.csr, sub.t().contiguous(), max_len=2).numpy(), KC.exact("H")[::5, :2])   # [P, 2]
    for empty in (torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0, 2, dtype=torch.int64)):
        assert walks_reference(c.csr, empty).shape == (0, 3)
        assert katz_from_walks(walks_reference(c.csr, empty), 0.1).shape == (0,)


def test_value_errors():
    csr = KC.case("C").csr
    ok = torch.tensor([[0, 1], [2, 3]])
    for bad in (0, 5, True, 2.0, -1, "3", None):
        with pytest.raises(ValueError):
            pair_walks(csr, ok, max_len=bad)
        with pytest.raises(ValueError):
            walks_reference(csr, ok, max_len=bad)
        with pytest.raises(ValueError):
            pair_katz(csr, ok, max_len=bad)
    for bad in (0.0, -0.5, float("nan"), float("inf"), True, "0.1", None):
        with pytest.raises(ValueError):
            pair_katz(csr, ok, beta=bad)
        with pytest.raises(ValueError):
            katz_from_walks(torch.zeros(2, 3, dtype=torch.int64), bad)
    for bad in (torch.tensor([[0.0, 1.0], [2.0, 3.0]]), torch.tensor([[True, False], [False, True]]),
                torch.zeros(3, dtype=torch.int64), torch.zeros(3, 3, dtype=torch.int64)):
        with pytest.raises(ValueError):
            pair_walks(csr, bad)
        with pytest.raises(ValueError):
            pair_katz(csr, bad)
    for kw in ({"chunk": 0}, {"groups": 0}, {"groups": 65536}, {"workspace_mb": 0}):
        with pytest.raises(ValueError):
            pair_walks(csr, ok, **kw)
    with pytest.raises(ValueError):
        katz_from_walks(torch.zeros(2, 3), 0.1)
    with pytest.raises(TypeError):
        pair_walks("not a graph", ok)


def test_range_guard():
    with pytest.raises(ValueError):
        check_range(1 << 21, 4)                                               # 2^63
    check_range((1 << 21) - 1, 4)
    check_range(1 << 21, 3)
    check_range(1 << 31, 3)                                                   # 2^62
    with pytest.raises(ValueError):
        check_range(3037000500, 3)                                            # ceil(sqrt(2^63))
    check_range(3037000499, 3)
    for deg in (0, 1, 1 << 40):
        check_range(deg, 1)
        check_range(deg, 2)


def test_abi_registration_and_exports():
    assert _lib.ABI_VERSION == 16
    assert "lpf_pair_walks" in _lib.HIP_PROTOTYPES and "lpf_pair_walks_workspace_bytes" in _lib.HIP_PROTOTYPES
    assert len(_lib.HIP_PROTOTYPES["lpf_pair_walks"]) == 13
    hip = _lib.hip()                                                          # loads without a GPU
    assert hip.lpf_abi_version() == 16
    assert hip.lpf_pair_walks_workspace_bytes(1000, 3) == 16 + 3 * 8000
    assert hip.lpf_pair_walks_workspace_bytes(0, 3) == 0
    for name in ("pair_walks", "pair_katz", "katz_from_walks", "walks_reference"):
        assert getattr(lpformer_amd, name) is getattr(katz, name) and name in lpformer_amd.__all__
    assert katz.default_groups(235_868, 32_768, 1024) == ((1024 << 20) - 16) // (8 * 235_868)
    assert katz.default_groups(1000, 5, 1024) == 5 and katz.default_groups(1 << 30, 100, 1) == 1


def test_katz_is_no_kind_of_pair_heuristics():
    from lpformer_amd.heuristics import KINDS, pair_heuristics
    assert "katz" not in KINDS
    with pytest.raises(ValueError):
        pair_heuristics(KC.case("C").csr, torch.tensor([[0, 1], [2, 3]]), kinds=("katz",))
