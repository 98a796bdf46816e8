"""pair_distance without a GPU: the numpy restatement (distance_reference, what pair_distance runs for a host graph.CSR
with CPU edges when no GPU is present) against scipy's unweighted shortest_path, the contract's corner cases, argument
validation, the C ABI registration and DIST_BINS through metrics_by_bin.  Nothing here has a tolerance."""
import numpy as np
import pytest
import torch

import lpformer_amd
from lpformer_amd import _lib, graph
from lpformer_amd import evaluate as E
from lpformer_amd.distance import DIST_BINS, distance_reference, pair_distance
from tests import pair_distance_cases as PC


def _t(pairs):
    return torch.from_numpy(np.array(pairs, dtype=np.int64))


def _host(case, pairs, **kw):
    """Through the public function where it takes the host path (no GPU present), else the restatement itself."""
    fn = distance_reference if torch.cuda.is_available() else pair_distance
    out = fn(case.csr, _t(pairs), **kw)
    assert out.dtype == torch.int32 and not out.is_cuda and out.shape == (np.asarray(pairs).shape[1],)
    return out.numpy()


def test_recipes_cover_what_the_tests_rely_on():
    s, h, c = PC.graph_s(), PC.graph_h(), PC.graph_c()
    ds, dh, dc = PC.exact("S"), PC.exact("H"), PC.exact("C")
    assert np.diff(s.A.indptr).max() == 10 and set(range(-1, 16)) <= set(ds.tolist()) and (ds == -1).sum() == 739
    deg = np.diff(h.A.indptr)
    assert deg[list(PC.HUBS)].tolist() == [603, 302, 260] and deg[list(PC.HUBS)].min() > 256
    # 64 is the farthest of the 4,096 DRAWN pairs; the graph's own largest finite distance, the eccentricity of the
    # path's far end, is 69 (the path's 60 hops to node 5 plus the body's 9 from there)
    assert (deg == 0).sum() == 262 and (dh == -1).sum() == 594 and dh.max() == 64
    far = PC.scipy_distance(h.A, np.stack([np.full(h.n, PC.PATH_LAST), np.arange(h.n)]))
    assert far.max() == 69 and far[5] == 60
    assert (deg[PC.PATH_FIRST:PC.PATH_LAST] == 2).all() and deg[PC.PATH_LAST] == 1
    assert c.n == 605 and np.diff(c.A.indptr)[1] == PC.CLIQUE - 1 and dc.min() == 1 and dc.max() == 8
    for case in (s, h, c):
        assert (case.A != case.A.T).nnz == 0 and case.A.diagonal().sum() == 0


@pytest.mark.parametrize("name", ["S", "H", "C"])
def test_numpy_path_matches_scipy(name):
    case = PC.CASES[name]()
    np.testing.assert_array_equal(_host(case, case.pairs), PC.exact(name))


@pytest.mark.parametrize("m", PC.MAX_DISTS)
@pytest.mark.parametrize("name", ["S", "H", "C"])
def test_numpy_path_max_dist_is_the_masked_exact_result(name, m):
    case = PC.CASES[name]()
    np.testing.assert_array_equal(_host(case, case.pairs, max_dist=m), PC.masked(PC.exact(name), m))


def test_numpy_path_ignore_direct():
    pairs, ref, plain = PC.ignore_direct_h()
    assert set(ref[:64].tolist()) == {-1, 2, 3, 4, 5, 6, 7} and (ref[:64] == -1).sum() == 11
    assert (plain[:64] == 1).all() and (plain[64:] != 1).all()
    case = PC.graph_h()
    got = _host(case, pairs, ignore_direct=True)
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(got[64:], plain[64:])                     # non-edges are unaffected
    np.testing.assert_array_equal(_host(case, pairs), plain)
    np.testing.assert_array_equal(_host(case, pairs[::-1], ignore_direct=True), ref)
    np.testing.assert_array_equal(_host(case, pairs, ignore_direct=True, max_dist=3), PC.masked(ref, 3))


def test_contract_cases():
    case = PC.graph_h()
    n = case.n
    iso = np.flatnonzero(np.diff(case.A.indptr) == 0)
    pairs = np.array([[7, 0, -1, n, 3, -1, iso[0], iso[1], 9, iso[2]],
                      [7, 0, 3, 3, n, -1, iso[1], 9, iso[1], iso[2]]])
    want = np.array([0, 0, -1, -1, -1, 0, -1, -1, -1, 0], np.int32)         # a == b reads 0 before anything else
    for kw in ({}, {"ignore_direct": True}, {"max_dist": 1}, {"ignore_direct": True, "max_dist": 2}):
        np.testing.assert_array_equal(_host(case, pairs, **kw), want, err_msg=str(kw))
    # P = 0 and P = 1, both layouts
    for empty in (torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0, 2, dtype=torch.int64)):
        out = pair_distance(case.csr, empty) if not torch.cuda.is_available() else distance_reference(case.csr, empty)
        assert out.dtype == torch.int32 and out.numel() == 0
    one = case.pairs[:, :1]
    np.testing.assert_array_equal(_host(case, one), PC.exact("H")[:1])
    sub = case.pairs[:, :300]
    fn = distance_reference if torch.cuda.is_available() else pair_distance
    np.testing.assert_array_equal(fn(case.csr, _t(sub.T)).numpy(), PC.exact("H")[:300])     # [P, 2]
    np.testing.assert_array_equal(fn(case.csr, _t(sub).to(torch.int32)).numpy(), PC.exact("H")[:300])


def test_stored_self_loops_change_nothing():
    case = PC.graph_s()
    A = case.A.tolil(copy=True)
    A.setdiag(1.0)
    A = A.tocsr()
    A.sort_indices()
    looped = PC.Case(case.n, A, graph.CSR(A.indptr.astype(np.int64), A.indices.astype(np.int32), None, case.n),
                     case.pairs)
    sub = case.pairs[:, :600]
    np.testing.assert_array_equal(_host(looped, sub), PC.exact("S")[:600])
    np.testing.assert_array_equal(_host(looped, sub, ignore_direct=True, max_dist=5),
                                  _host(case, sub, ignore_direct=True, max_dist=5))


def test_value_errors():
    csr = PC.graph_c().csr
    ok = torch.tensor([[0, 1], [2, 3]])
    for bad in (torch.tensor([[0.0, 1.0], [2.0, 3.0]]), torch.tensor([[True, False], [False, True]]),
                torch.zeros(3, dtype=torch.int64), torch.zeros(3, 3, dtype=torch.int64),
                torch.zeros(2, 2, 2, dtype=torch.int64)):
        with pytest.raises(ValueError):
            pair_distance(csr, bad)
    for kw in ({"chunk": 0}, {"chunk": -5}, {"max_dist": 0}, {"max_dist": -1}, {"max_dist": 2.5}, {"max_dist": True},
               {"groups": 0}, {"groups": -3}, {"workspace_mb": 0}):
        with pytest.raises(ValueError):
            pair_distance(csr, ok, **kw)
    with pytest.raises(ValueError):
        distance_reference(csr, ok, max_dist=0)
    with pytest.raises(TypeError):
        pair_distance("not a graph", ok)


def test_abi_registration_and_exports():
    assert _lib.ABI_VERSION == 16
    assert "lpf_pair_bfs" in _lib.HIP_PROTOTYPES and "lpf_pair_bfs_workspace_bytes" in _lib.HIP_PROTOTYPES
    assert len(_lib.HIP_PROTOTYPES["lpf_pair_bfs"]) == 14
    assert lpformer_amd.pair_distance is pair_distance and lpformer_amd.DIST_BINS is DIST_BINS
    assert "pair_distance" in lpformer_amd.__all__ and "DIST_BINS" in lpformer_amd.__all__
    from lpformer_amd.heuristics import KINDS
    assert KINDS == ("cn", "aa", "ra", "ppr", "feat")


def test_default_groups_fit_the_workspace():
    from lpformer_amd.distance import default_groups
    assert default_groups(235_868, 32_768, 1024) == (1024 << 20) // (8 * 235_868 + 8)
    assert default_groups(1000, 32_768, 1024) == 2048 and default_groups(1000, 5, 1024) == 5
    assert default_groups(1 << 30, 100, 1) == 1


def test_dist_bins_through_metrics_by_bin():
    dist = torch.tensor([-1, 0, 1, 5, 6, 40, 2, 3, 4], dtype=torch.int32)
    pos = torch.linspace(0.1, 0.9, dist.numel())
    neg = torch.linspace(0.0, 1.0, 50)
    got = E.metrics_by_bin(pos, neg, dist, bins=DIST_BINS, k_list=(10,))
    assert [g["bin"] for g in got] == list(DIST_BINS)
    # unreachable | same node | 1 | 2 | 3 | 4-5 | 6 or more
    assert [g["count"] for g in got] == [1, 1, 1, 1, 1, 2, 2]
    cell = {v: next(i for i, (lo, hi) in enumerate(DIST_BINS) if lo <= v < hi) for v in (-1, 0, 1, 5, 6, 40)}
    assert cell == {-1: 0, 0: 1, 1: 2, 5: 5, 6: 6, 40: 6}
    for g, want in zip(got, ([0], [1], [2], [6], [7], [3, 8], [4, 5])):      # which positives each cell holds
        assert g["Hits@10"] == pytest.approx(E.hits_at_k(pos[want], neg, 10))
