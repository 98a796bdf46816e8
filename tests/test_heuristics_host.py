"""CPU checks of the binned metrics (evaluate.metrics_by_bin / quantile_bins) against a numpy restatement of the
reference's test_by_metric (src/train/eval.py:62-73, as intended), and of pair_heuristics' argument checks."""
import math

import numpy as np
import pytest
import torch

from lpformer_amd import evaluate as E
from lpformer_amd import graph
from lpformer_amd.heuristics import pair_heuristics


def _np_hits(pos, neg, k):
    """OGB Evaluator hits@K (what evaluate_hits asks for, eval.py:6-17): 1.0 with fewer than K negatives."""
    if neg.size < k:
        return 1.0
    kth = np.sort(neg)[::-1][k - 1]
    return float(np.sum(pos > kth)) / pos.size


def _np_by_bin(pos, neg, vals, bins, k_list):
    """eval.py:69-73 with the bin list kept (the reference overwrites it at :68)."""
    out = []
    for lo, hi in bins:
        ix = (vals >= lo) & (vals < hi)
        res = {"bin": (lo, hi), "count": int(ix.sum())}
        for k in k_list:
            res[f"Hits@{k}"] = _np_hits(pos[ix], neg, k) if ix.any() else float("nan")
        out.append(res)
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], float) and math.isnan(a[k]):
            assert isinstance(b[k], float) and math.isnan(b[k]), k
        elif isinstance(a[k], float):
            assert a[k] == pytest.approx(b[k], abs=1e-7), k
        else:
            assert a[k] == b[k], k


def test_metrics_by_bin_matches_reference_logic_with_ties_and_edges():
    rng = np.random.default_rng(0)
    # scores on a coarse grid: many positive / negative ties at the K-th negative
    neg = rng.integers(0, 20, size=500).astype(np.float32) / 4
    pos = rng.integers(0, 24, size=300).astype(np.float32) / 4
    # CN-like values, many exactly on the bin edges 1, 3, 10; none >= 10 -> (10, 1e6) is empty
    vals = rng.choice(np.array([0, 1, 2, 3, 4, 9], np.float32), size=300)
    got = E.metrics_by_bin(torch.from_numpy(pos), torch.from_numpy(neg), torch.from_numpy(vals))
    want = _np_by_bin(pos, neg, vals, E.CN_BINS, (20, 50, 100))
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        _same(g, w)
    assert got[-1]["count"] == 0 and all(math.isnan(got[-1][f"Hits@{k}"]) for k in (20, 50, 100))
    assert sum(g["count"] for g in got) == 300
    # a value exactly on an edge lands in the bin that starts there (half-open [lo, hi))
    one = E.metrics_by_bin(torch.tensor([1.0]), torch.from_numpy(neg), torch.tensor([3.0]))
    assert [g["count"] for g in one] == [0, 0, 1, 0]


def test_metrics_by_bin_few_negatives_and_custom_bins():
    pos = torch.tensor([0.5, 0.7, 0.9, 0.1])
    neg = torch.tensor([0.6, 0.2])
    vals = torch.tensor([0.0, 5.0, 5.0, 20.0])
    got = E.metrics_by_bin(pos, neg, vals, bins=((0, 5), (5, 6), (6, 7)), k_list=(1, 2, 3))
    want = _np_by_bin(pos.numpy(), neg.numpy(), vals.numpy(), ((0, 5), (5, 6), (6, 7)), (1, 2, 3))
    for g, w in zip(got, want):
        _same(g, w)
    assert got[0]["Hits@3"] == 1.0          # fewer negatives than K: the OGB rule says 1.0
    assert got[1]["Hits@1"] == 1.0 and got[1]["Hits@2"] == 1.0


def test_metrics_by_bin_per_positive_negatives():
    rng = np.random.default_rng(1)
    pos = torch.from_numpy(rng.integers(0, 10, size=200).astype(np.float32))
    neg = torch.from_numpy(rng.integers(0, 10, size=(200, 150)).astype(np.float32))   # ties everywhere
    vals = torch.from_numpy(rng.integers(0, 12, size=200).astype(np.int32))
    got = E.metrics_by_bin(pos, neg, vals)
    for g, (lo, hi) in zip(got, E.CN_BINS):
        ix = (vals >= lo) & (vals < hi)
        assert g["bin"] == (lo, hi) and g["count"] == int(ix.sum())
        want = E.ranking_metrics(pos[ix], neg[ix])
        for k, v in want.items():
            assert g[k] == v
    empty = E.metrics_by_bin(pos, neg, vals, bins=((100, 200),))[0]
    assert empty["count"] == 0 and all(math.isnan(empty[k]) for k in ("Hits@10", "Hits@50", "Hits@100", "MRR"))


def test_metrics_by_bin_rejects_mismatched_shapes():
    with pytest.raises(ValueError):
        E.metrics_by_bin(torch.zeros(5), torch.zeros(10), torch.zeros(4))
    with pytest.raises(ValueError):
        E.metrics_by_bin(torch.zeros(5), torch.zeros(4, 3), torch.zeros(5))


def test_quantile_bins():
    v = torch.arange(1, 10, dtype=torch.float32)            # 1 .. 9: quartiles 3, 5, 7
    assert E.quantile_bins(v) == ((-math.inf, 3.0), (3.0, 5.0), (5.0, 7.0), (7.0, math.inf))
    assert E.quantile_bins(v, qs=(0.75,)) == ((-math.inf, 7.0), (7.0, math.inf))
    assert E.quantile_bins(torch.tensor([0.0, 1.0]), qs=(0.5,)) == ((-math.inf, 0.5), (0.5, math.inf))
    bins = E.quantile_bins(v)
    counts = [g["count"] for g in E.metrics_by_bin(v, torch.zeros(3), v, bins=bins)]
    assert counts == [2, 2, 2, 3]
    with pytest.raises(ValueError):
        E.quantile_bins(v, qs=(0.5, 0.25))
    with pytest.raises(ValueError):
        E.quantile_bins(torch.zeros(0))


def _csr():
    return graph.mask_csr(np.array([[0, 1, 2], [1, 2, 3]]), 4)


@pytest.mark.parametrize("kinds", [("cn", "katz"), (), ("CN",), ["aa", "shortest_path"]])
def test_pair_heuristics_rejects_bad_kinds(kinds):
    with pytest.raises(ValueError, match="kinds"):
        pair_heuristics(_csr(), torch.zeros(2, 3, dtype=torch.int64), kinds=kinds)


@pytest.mark.parametrize("edges", [torch.zeros(3, 3, dtype=torch.int64), torch.zeros(6, dtype=torch.int64),
                                   torch.zeros(2, 2, 2, dtype=torch.int64), torch.zeros(4, 5, dtype=torch.int64)])
def test_pair_heuristics_rejects_bad_edge_shapes(edges):
    with pytest.raises(ValueError):
        pair_heuristics(_csr(), edges)


def test_pair_heuristics_rejects_float_ids_and_bad_chunk_and_source():
    with pytest.raises(ValueError):
        pair_heuristics(_csr(), torch.zeros(2, 3))
    with pytest.raises(ValueError):
        pair_heuristics(_csr(), torch.zeros(2, 3, dtype=torch.int64), chunk=0)
    with pytest.raises(TypeError):
        pair_heuristics(np.eye(4), torch.zeros(2, 3, dtype=torch.int64))
