"""pair_hop_counts without a GPU: the numpy restatement (hop_counts_reference, what the entry point runs for a host
graph.CSR with CPU edges when no GPU is present) against scipy's shortest paths and the hand cases, the derived
features, argument validation and the C ABI registration.  Every comparison of counts is exact integer equality."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import lpformer_amd
from lpformer_amd import _lib, hops
from lpformer_amd.distance import distance_reference
from lpformer_amd.hops import ball_jaccard, elph_features, hop_counts_reference, pair_hop_counts
from tests import pair_hops_cases as HC
from tests import pair_katz_cases as KC


def _t(pairs):
    return torch.from_numpy(np.array(pairs, dtype=np.int64))


def _host(csr, pairs, **kw):
    """Through the public function where it takes the host path (no GPU present), else the restatement itself."""
    fn = hop_counts_reference if torch.cuda.is_available() else pair_hop_counts
    out = fn(csr, _t(pairs), **kw)
    k = kw.get("hops", 2)
    assert out.dtype == torch.int32 and not out.is_cuda and out.shape == (np.asarray(pairs).shape[1], k + 2, k + 2)
    return out.numpy()


@lru_cache(maxsize=None)
def _host_case(name, k=2, ignore_direct=False):
    """The restatement on a case's whole batch, computed once per process and handed out read-only."""
    c = KC.case(name)
    out = _host(c.csr, c.pairs, hops=k, ignore_direct=ignore_direct)
    out.setflags(write=False)
    return out


def test_reference_meets_the_conditions():
    """exact() asserts the shares, the distinct tables, the sums and the ignore_direct rule; here they are printed."""
    for name in HC.NAMES:
        t = HC.exact(name, 2)
        ti = HC.exact(name, 2, True)
        print(name, "positive shares:", HC.positive_shares(t), "distinct tables:", HC.distinct_tables(t),
              "stored entries:", int(HC.stored(name).sum()), "changed:", int((t != ti).any(axis=(1, 2)).sum()))
        assert t.shape == (KC.case(name).pairs.shape[1], 4, 4) and HC.exact(name, 1).shape[1:] == (3, 3)


@pytest.mark.parametrize("ignore_direct", [False, True])
@pytest.mark.parametrize("k", HC.HOPS)
@pytest.mark.parametrize("name", HC.NAMES)
def test_numpy_path_matches_scipy(name, k, ignore_direct):
    np.testing.assert_array_equal(_host_case(name, k, ignore_direct), HC.exact(name, k, ignore_direct))


@pytest.mark.parametrize("hand", HC.hand_cases(), ids=lambda h: h.what)
def test_numpy_path_matches_the_hand_cases(hand):
    got = _host(hand.csr, hand.pairs, hops=hand.hops, ignore_direct=hand.ignore_direct)
    np.testing.assert_array_equal(got, hand.tables)
    np.testing.assert_array_equal(_host(hand.csr, hand.pairs[::-1], hops=hand.hops, ignore_direct=hand.ignore_direct),
                                  hand.tables.transpose(0, 2, 1))
    ok = ((hand.pairs >= 0) & (hand.pairs < hand.csr.n)).all(axis=0)
    np.testing.assert_array_equal(hand.tables.sum(axis=(1, 2)), np.where(ok, hand.csr.n, 0))


@pytest.mark.parametrize("name", HC.NAMES)
def test_swapped_pairs_give_the_transpose(name):
    c = KC.case(name)
    sub = c.pairs[:, ::4]                      # every part of the batch, a quarter of each
    for ig in (False, True):
        np.testing.assert_array_equal(_host(c.csr, sub[::-1], ignore_direct=ig),
                                      HC.exact(name, 2, ig)[::4].transpose(0, 2, 1))


@pytest.mark.parametrize("name", HC.NAMES)
def test_one_hop_is_two_hops_with_the_far_classes_merged(name):
    for ig in (False, True):
        t2 = _host_case(name, 2, ig).astype(np.int64)
        merged = np.zeros((t2.shape[0], 3, 3), np.int64)
        fold = np.array([0, 1, 2, 2])
        for i in range(4):
            for j in range(4):
                merged[:, fold[i], fold[j]] += t2[:, i, j]
        np.testing.assert_array_equal(_host_case(name, 1, ig), merged)


@pytest.mark.parametrize("name", HC.NAMES)
def test_against_distance_and_common_neighbours(name):
    """T[0][j] has its single 1 at j = min(dist, k + 1) (dist -1 -> k + 1) by distance.py's host reference, with
    ignore_direct off and on; T[1][1] is the common-neighbour count for a != b (pair_heuristics has no host path: its
    CN is (A @ A)[a, b], which is W_2 of tests/pair_katz_cases.exact)."""
    c = KC.case(name)
    ok = ((c.pairs >= 0) & (c.pairs < c.n)).all(axis=0)
    for ig in (False, True):
        d = distance_reference(c.csr, _t(c.pairs), ignore_direct=ig).numpy().astype(np.int64)
        for k in HC.HOPS:
            t = _host_case(name, k, ig)
            at = np.where((d < 0) | (d > k), k + 1, d)
            want = np.zeros((c.pairs.shape[1], k + 2), np.int32)
            want[np.flatnonzero(ok), at[ok]] = 1
            np.testing.assert_array_equal(t[:, 0, :], want)
            np.testing.assert_array_equal(t[:, :, 0], want)          # by symmetry of the graph
    differ = ok & (c.pairs[0] != c.pairs[1])
    cn = KC.exact(name)[:, 1]
    for k in HC.HOPS:
        np.testing.assert_array_equal(_host_case(name, k)[differ, 1, 1], cn[differ])
    assert int(cn[differ].max()) > 0


def test_stored_self_loops_change_nothing():
    c = KC.case("S")
    A = c.A.tolil(copy=True)
    A.setdiag(1.0)
    A = A.tocsr()
    A.sort_indices()
    csr = lpformer_amd.graph.CSR(A.indptr.astype(np.int64), A.indices.astype(np.int32), None, c.n)
    sub = c.pairs[:, ::3]
    for ig in (False, True):
        np.testing.assert_array_equal(_host(csr, sub, ignore_direct=ig), HC.exact("S", 2, ig)[::3])


def test_elph_features_order_and_ball_jaccard():
    t2 = torch.tensor([[[1, 0, 0, 0],        # (a made-up table: every cell the features read has its own value)
                        [0, 11, 12, 13],
                        [0, 21, 22, 23],
                        [1, 31, 32, 33]],
                       [[0, 0, 0, 0]] * 4], dtype=torch.int32)
    f = elph_features(t2)
    assert f.shape == (2, 8) and not f.dtype.is_floating_point
    assert f[0].tolist() == [11, 12, 21, 22, 13, 23, 31, 32] and f[1].tolist() == [0] * 8
    t1 = torch.tensor([[[0, 1, 0], [1, 5, 7], [0, 9, 100]]], dtype=torch.int32)
    assert elph_features(t1).tolist() == [[5, 7, 9]]
    j = ball_jaccard(t2)
    inter = 1 + 11 + 12 + 21 + 22
    union = inter + 13 + 23 + 1 + 31 + 32
    assert j.dtype == torch.float32 and j.shape == (2,)
    assert j[0].item() == np.float32(np.float64(inter) / np.float64(union)) and j[1].item() == 0.0
    assert ball_jaccard(t1).item() == np.float32(np.float64(7) / np.float64(23))
    # on real tables: within [0, 1], 1 exactly for a == b, 0 for a bad id
    c = KC.case("H")
    jt = ball_jaccard(torch.from_numpy(HC.exact("H", 2).copy())).numpy()
    same = (c.pairs[0] == c.pairs[1]) & (c.pairs[0] >= 0) & (c.pairs[0] < c.n)
    assert (jt >= 0).all() and (jt <= 1).all() and int(same.sum()) >= 3 and (jt[same] == 1).all()
    assert (jt[-4:] == 0).all()
    for bad in (torch.zeros(3, 4, 4), torch.zeros(3, 4, dtype=torch.int32), torch.zeros(3, 5, 5, dtype=torch.int32),
                torch.zeros(3, 4, 3, dtype=torch.int32), np.zeros((3, 4, 4), np.int32)):
        with pytest.raises(ValueError):
            elph_features(bad)
        with pytest.raises(ValueError):
            ball_jaccard(bad)


def test_value_errors():
    csr = KC.case("C").csr
    ok = torch.tensor([[0, 1], [2, 3]])
    for bad in (0, 3, True, False, 2.0, -1, "2", None):
        with pytest.raises(ValueError):
            pair_hop_counts(csr, ok, hops=bad)
        with pytest.raises(ValueError):
            hop_counts_reference(csr, ok, hops=bad)
    for bad in (torch.tensor([[0.0, 1.0], [2.0, 3.0]]), torch.tensor([[True, False], [False, True]]),
                torch.zeros(3, dtype=torch.int64), torch.zeros(3, 3, dtype=torch.int64)):
        with pytest.raises(ValueError):
            pair_hop_counts(csr, bad)
    for kw in ({"chunk": 0}, {"groups": 0}, {"groups": 65536}, {"workspace_mb": 0}, {"workspace_mb": -1.0}):
        with pytest.raises(ValueError):
            pair_hop_counts(csr, ok, **kw)
    with pytest.raises(TypeError):
        pair_hop_counts("not a graph", ok)


def test_host_fallback_returns_cpu_tensors():
    c = KC.case("H")
    sub = _t(c.pairs[:, ::5])
    fn = hop_counts_reference if torch.cuda.is_available() else pair_hop_counts   # (on a GPU: test_gpu_pair_hops.py)
    t = fn(c.csr, sub)
    assert not t.is_cuda and t.dtype == torch.int32
    np.testing.assert_array_equal(t.numpy(), HC.exact("H", 2)[::5])
    np.testing.assert_array_equal(fn(c.csr, sub.t().contiguous(), hops=1).numpy(), HC.exact("H", 1)[::5])   # [P, 2]
    for empty in (torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0, 2, dtype=torch.int64)):
        assert hop_counts_reference(c.csr, empty).shape == (0, 4, 4)
        assert hop_counts_reference(c.csr, empty, hops=1).shape == (0, 3, 3)
        assert elph_features(hop_counts_reference(c.csr, empty)).shape == (0, 8)
        assert ball_jaccard(hop_counts_reference(c.csr, empty)).shape == (0,)


def test_abi_registration_and_exports():
    assert _lib.ABI_VERSION == 16
    assert len(_lib.HIP_PROTOTYPES["lpf_pair_hop_counts_workspace_bytes"]) == 2
    assert len(_lib.HIP_PROTOTYPES["lpf_pair_hop_counts"]) == 13
    hip = _lib.hip()                                                          # loads without a GPU
    assert hip.lpf_abi_version() == 16
    assert hip.lpf_pair_hop_counts_workspace_bytes(1000, 3) == 16 + 3 * 8000
    assert hip.lpf_pair_hop_counts_workspace_bytes(0, 3) == 0 and hip.lpf_pair_hop_counts_workspace_bytes(5, 0) == 0
    for name in ("pair_hop_counts", "hop_counts_reference", "elph_features", "ball_jaccard"):
        assert getattr(lpformer_amd, name) is getattr(hops, name) and name in lpformer_amd.__all__
    assert hops.default_groups(235_868, 32_768, 1024) == ((1024 << 20) - 16) // (8 * 235_868)
    assert hops.default_groups(1000, 5, 1024) == 5 and hops.default_groups(1 << 30, 100, 1) == 1
