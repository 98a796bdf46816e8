"""Host checks of the hard-negative definition (no GPU): the numpy restatement in tests/hard_negatives_reference.py
against scipy, the interleave and padding rules on hand-written cases, argument errors, and chunk planning."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import lpformer_amd
from lpformer_amd import data as D
from lpformer_amd import graph
from lpformer_amd import hard_negatives as HN
from lpformer_amd.recommend import plan_chunks
from tests import hard_negatives_reference as R


def _adj(ei, n):
    ei = np.asarray(ei, np.int64)
    r, c = np.concatenate([ei[0], ei[1]]), np.concatenate([ei[1], ei[0]])
    keep = r != c
    m = sp.csr_matrix((np.ones(keep.sum()), (r[keep], c[keep])), shape=(n, n))
    m.sum_duplicates()
    m.data[:] = 1.0
    m.sort_indices()
    return m


@pytest.fixture(scope="module")
def small():
    n = 300
    ei, _ = D.chung_lu_graph(n, 1500, gamma=2.3, seed=3)
    A = _adj(ei, n)
    ppr = lpformer_amd.calc_ppr(np.asarray(ei, np.int64), n, 0.15, 1e-3)
    P = sp.csr_matrix((ppr.val, ppr.col, ppr.rowptr), shape=(n, n))
    P.sort_indices()
    x = np.random.default_rng(0).standard_normal((n, 16)).astype(np.float32)
    return n, A, P, x


def test_twohop_row_matches_scipy(small):
    n, A, _, _ = small
    w_aa, w_ra = R.weight_tables(A)
    A64 = A.astype(np.float64)
    CN = (A64 @ A64).toarray()
    AA = (A64 @ sp.diags(w_aa.astype(np.float64)) @ A64).toarray()
    RA = (A64 @ sp.diags(w_ra.astype(np.float64)) @ A64).toarray()
    for u in range(n):
        col, cn, aa, ra = R.twohop_row(A, u, w_aa, w_ra)
        np.testing.assert_array_equal(col, np.flatnonzero(CN[u] > 0))
        np.testing.assert_array_equal(cn, CN[u, col].astype(np.int32))      # exact
        assert cn.dtype == np.int32 and aa.dtype == np.float32 and ra.dtype == np.float32
        # fp64 sums in another order, then one fp32 rounding: within one fp32 spacing of the value
        np.testing.assert_array_less(np.abs(aa - AA[u, col]), np.spacing(np.abs(AA[u, col]).astype(np.float32)) + 1e-30)
        np.testing.assert_array_less(np.abs(ra - RA[u, col]), np.spacing(np.abs(RA[u, col]).astype(np.float32)) + 1e-30)
        ecol, ecn, _, _ = R.twohop_row(A, u, w_aa, w_ra, exclude=True)
        nbr = A.indices[A.indptr[u]:A.indptr[u + 1]]
        want = col[~np.isin(col, nbr) & (col != u)]
        np.testing.assert_array_equal(ecol, want)
        np.testing.assert_array_equal(ecn, CN[u, want].astype(np.int32))
    assert R.twohop_row(A, -1, w_aa, w_ra)[0].size == 0 and R.twohop_row(A, n, w_aa, w_ra)[0].size == 0


def test_pool_is_twohop_union_ppr_minus_neighbours(small):
    n, A, P, _ = small
    w_aa, w_ra = R.weight_tables(A)
    CN = (A @ A).toarray()
    for u in range(0, n, 7):
        members, vals = R.pool(A, P, u, w_aa, w_ra)
        want = set(np.flatnonzero(CN[u] > 0)) | set(P.indices[P.indptr[u]:P.indptr[u + 1]])
        want -= set(A.indices[A.indptr[u]:A.indptr[u + 1]]) | {u}
        assert members.tolist() == sorted(want)
        np.testing.assert_array_equal(vals["cn"], CN[u, members].astype(np.float32))
        np.testing.assert_array_equal(vals["ppr"], np.asarray(P[u, members].todense()).ravel().astype(np.float32))
        members0, vals0 = R.pool(A, None, u, w_aa, w_ra)
        assert set(members0) <= set(members) and not vals0["ppr"].any()


def test_rank_list_ties_zeros_and_nan():
    members = np.array([3, 5, 8, 9, 11, 20], np.int64)
    v = np.array([0.5, 2.0, 0.5, 0.0, np.nan, 2.0], np.float32)
    assert R.rank_list(members, v, 10).tolist() == [5, 20, 3, 8]          # ties to the smaller id; 0 and NaN unranked
    assert R.rank_list(members, v, 3).tolist() == [5, 20, 3]
    assert R.rank_list(members, -v, 3).tolist() == []                      # negative values do not rank
    assert R.rank_list(members[:0], v[:0], 3).tolist() == []


def test_interleave_rule():
    a, b, c = [1, 2, 3, 4], [2, 1, 9], [7]
    assert R.interleave([a, b, c], 10) == [1, 2, 7, 3, 9, 4]               # duplicates across heuristics kept once
    assert R.interleave([a, b, c], 3) == [1, 2, 7]
    assert R.interleave([b, a, c], 4) == [2, 1, 7, 9]                      # ties by the order of the heuristics
    assert R.interleave([[], [5, 6], []], 4) == [5, 6]                     # a heuristic with fewer than kh entries
    assert R.interleave([[], [], []], 4) == [] and R.interleave([], 4) == []


def test_padding_rules(small):
    n, A, P, x = small
    kh = 40
    for u in (0, 17, int(np.argmax(np.diff(A.indptr)))):
        nbr = A.indices[A.indptr[u]:A.indptr[u + 1]]
        start = [int(v) for v in np.setdiff1d(np.arange(n), np.append(nbr, u))[:5]]
        got = R.pad(start, u, nbr, n, kh, seed=11)
        assert got[:5] == start and len(got) == kh == len(set(got))
        assert u not in got and not np.isin(got, nbr).any() and min(got) >= 0 and max(got) < n
        assert got == R.pad(start, u, nbr, n, kh, seed=11)
        assert got != R.pad(start, u, nbr, n, kh, seed=12)
    with pytest.raises(ValueError):
        R.pad([], 0, np.arange(1, n - 3), n, kh, 0)
    # the hash is a bijection of the draw index: no draw repeats
    assert len({R.pad_draw(5, 9, d, 1 << 31) for d in range(1000)}) == 1000


def test_lists_do_not_depend_on_the_batch(small):
    n, A, P, x = small
    rng = np.random.default_rng(2)
    e = rng.integers(0, n, size=(2, 40))
    heur = ("ra", "ppr", "feat")
    neg, nr, nodes, lists, ranked, spare = R.heart_negatives(A, P, x, e, 20, heur, seed=4)
    assert neg.shape == (40, 20, 2) and nr.shape == (40, 2) and (nr <= 10).all()
    h1 = R.heart_negatives(A, P, x, e[:, :13], 20, heur, seed=4)
    h2 = R.heart_negatives(A, P, x, e[:, 13:][:, ::-1], 20, heur, seed=4)
    for part in (h1, h2):
        at = np.searchsorted(nodes, part[2])
        np.testing.assert_array_equal(lists[at], part[3])
        np.testing.assert_array_equal(ranked[at], part[4])
    np.testing.assert_array_equal(neg[:13], h1[0])
    # invariants of rule 6 and of the lists
    assert (neg[:, :10, 0] == e[0][:, None]).all() and (neg[:, 10:, 1] == e[1][:, None]).all()
    dense = A.toarray() > 0
    assert not dense[neg[..., 0], neg[..., 1]].any() and (neg[..., 0] != neg[..., 1]).all()
    for row in lists:
        assert len(set(row.tolist())) == row.size
    # a held-out positive whose other endpoint is in the list: dropped, the spare entry moves in
    i = int(np.flatnonzero(~dense[nodes[:, None], lists].any(axis=1))[0])
    u, b = int(nodes[i]), int(lists[i, 2])
    one = R.heart_negatives(A, P, x, np.array([[u], [b]]), 20, heur, seed=4)
    assert one[0][0, :10, 1].tolist() == lists[i, :2].tolist() + lists[i, 3:].tolist() + [int(spare[i])]
    assert b not in one[0][0, :10, 1] and one[3][list(one[2]).index(u)].tolist() == lists[i].tolist()


def test_argument_errors():
    e = torch.tensor([[0, 1], [2, 3]])
    for bad_k in (0, 1, 7, 1026, 2.0, True):
        with pytest.raises(ValueError):
            HN._check_args(e, bad_k, ("ra",), 0, 1)
    for bad_h in ((), ("ra", "bogus"), ("ra", "ra"), "xx"):
        with pytest.raises(ValueError):
            HN._check_args(e, 4, bad_h, 0, 1)
    with pytest.raises(ValueError):
        HN._check_args(e, 4, ("ra",), 0, 0)
    with pytest.raises(TypeError):
        HN._check_args(e, 4, ("ra",), 0.5, 1)
    with pytest.raises(TypeError):
        HN._check_args(e.float(), 4, ("ra",), 0, 1)
    with pytest.raises(ValueError):
        HN._check_args(torch.zeros(3, 3, dtype=torch.int64), 4, ("ra",), 0, 1)
    edges, heur, seed = HN._check_args(torch.tensor([[0, 1], [2, 3], [4, 5]]), 4, "cn", -1, 1)
    assert edges.shape == (2, 3) and heur == ("cn",) and seed == 0xFFFFFFFFFFFFFFFF
    csr = graph.mask_csr(np.array([[0, 1], [1, 2]]), 4, symmetric=True)
    with pytest.raises(ValueError, match="feat.*no x"):
        lpformer_amd.heart_negatives((csr, None, None), e, 2, heuristics=("ra", "feat"))
    with pytest.raises(ValueError, match="ppr"):
        lpformer_amd.heart_negatives(csr, e, 2, heuristics=("ppr",))
    with pytest.raises(ValueError):
        lpformer_amd.twohop_rows(csr, torch.tensor([0]), kinds=("cn", "ppr"))
    with pytest.raises(TypeError):
        lpformer_amd.twohop_rows(csr, torch.tensor([0.5]))


def test_plan_chunks_is_reused_at_chunk_boundaries():
    assert HN.plan_chunks is plan_chunks
    bound = np.array([5, 5, 0, 11, 3, 7])
    assert plan_chunks(bound, 10) == [(0, 3), (3, 4), (4, 6)]     # exactly full; a node above max_pairs alone
    assert plan_chunks(bound, 1 << 24) == [(0, 6)]
    assert plan_chunks(np.zeros(0, np.int64), 4) == []
