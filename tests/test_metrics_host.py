"""rank_counts / ranks / sample_hits / link_metrics / split_metrics on CPU tensors (the torch restatement inside
lpformer_amd.evaluate) against what the reference's evaluation.py computed (tests/golden/metrics_*.npz, written by
tests/golden/make_metrics_golden.py), against the literal torch expressions, and against sklearn.

Bounds.  Counts, ranks and per-sample hits: equal.  MRR, AUC and AP against recorded fp64 values: 1e-9 (an fp64 sum of
P <= 1e5 terms below 1 is off by at most P * 2^-53 ~ 1e-11).  Against the reference's own float32 means
(``evaluate_mrr``): 2e-6 -- a float32 mean of P <= 300 terms in [0, 1] is off by at most about P * 2^-24 / 2 ~ 9e-6 in
the worst case of a sequential sum, torch sums pairwise (log2(P) * 2^-24 ~ 5e-7), plus one rounding of 1 / rank
(6e-8)."""
import glob
import os

import numpy as np
import pytest
import torch

from lpformer_amd import evaluate as E
from tests.golden_util import GOLDEN_DIR

CASES = sorted(os.path.basename(p)[len("metrics_"):-len(".npz")] for p in glob.glob(f"{GOLDEN_DIR}/metrics_*.npz"))
F64_TOL = 1e-9
F32_MEAN_TOL = 2e-6


def load(case):
    z = np.load(f"{GOLDEN_DIR}/metrics_{case}.npz")
    return z, {k: torch.from_numpy(z[k]) for k in ("pos", "pos_train", "neg", "neg_rows", "pos_test", "neg_test")}


def test_cases_present():
    assert set(CASES) >= {"continuous", "quantised", "equal", "p1", "m1", "m_lt_k", "inf"}


@pytest.mark.parametrize("case", CASES)
def test_rows_layout_matches_reference(case):
    z, t = load(case)
    ks = tuple(int(k) for k in z["ks"])
    pos, neg = t["pos"], t["neg_rows"]
    ge, gt = E.rank_counts(pos, neg)
    assert ge.dtype == gt.dtype == torch.int32
    assert torch.equal(ge, (neg >= pos.view(-1, 1)).sum(1).int()) and torch.equal(gt, (neg > pos.view(-1, 1)).sum(1).int())
    r = E.ranks(pos, neg)
    assert r.dtype == torch.float32
    np.testing.assert_array_equal(r.numpy(), z["rows_ranking_list"])
    sh = E.sample_hits(pos, neg, ks=ks)
    for k in ks:
        np.testing.assert_array_equal(sh[f"Hits@{k}"].numpy(), z[f"rows_sample_Hits@{k}"])
    m = E.link_metrics(pos, neg, k_list=(10, 50, 100))
    assert abs(m["MRR"] - float(z["rows_mrr64"])) <= F64_TOL
    assert abs(m["MRR"] - float(z["rows_MRR"])) <= F32_MEAN_TOL
    for k in (10, 50, 100):
        assert abs(m[f"Hits@{k}"] - float(z[f"rows_Hits@{k}"])) <= F32_MEAN_TOL
    assert m["nan_pos"] == 0 and m["nan_neg"] == 0


@pytest.mark.parametrize("case", CASES)
def test_shared_layout_matches_reference(case):
    z, t = load(case)
    ks = tuple(int(k) for k in z["ks"])
    for tag, p, n in (("train", "pos_train", "neg"), ("valid", "pos", "neg"), ("test", "pos_test", "neg_test")):
        pos, neg = t[p], t[n]
        ge, gt = E.rank_counts(pos, neg)
        assert torch.equal(ge, (neg.view(1, -1) >= pos.view(-1, 1)).sum(1).int())
        assert torch.equal(gt, (neg.view(1, -1) > pos.view(-1, 1)).sum(1).int())
        np.testing.assert_array_equal(E.ranks(pos, neg).numpy(), z[f"shared_ranking_list_{tag}"])
        sh = E.sample_hits(pos, neg, ks=ks)
        for k in ks:
            np.testing.assert_array_equal(sh[f"Hits@{k}"].numpy(), z[f"shared_sample_{tag}_Hits@{k}"])
    out = E.split_metrics(t["pos_train"], t["pos"], t["neg"], t["pos_test"], t["neg_test"], k_list=ks)
    for k in ks:
        assert out[f"Hits@{k}"] == tuple(float(v) for v in z[f"split_Hits@{k}"])
    for i in range(3):
        assert abs(out["MRR"][i] - float(z["split_mrr64"][i])) <= F64_TOL
        assert abs(out["MRR"][i] - float(z["split_MRR"][i])) <= F32_MEAN_TOL
    assert out["nan_pos"] == (0, 0, 0) and out["nan_neg"] == (0, 0, 0)
    if int(z["has_auc"]):
        assert abs(out["AUC"][1] - float(z["auc"])) <= F64_TOL
        assert abs(out["AP"][1] - float(z["ap"])) <= F64_TOL
        assert round(out["AUC"][1], 4) == float(z["auc_rounded"])
        assert round(out["AP"][1], 4) == float(z["ap_rounded"])
        m = E.link_metrics(t["pos"], t["neg"], k_list=ks)
        assert (m["AUC"], m["AP"], m["MRR"]) == (out["AUC"][1], out["AP"][1], out["MRR"][1])


def test_some_case_records_auc():
    assert sum(int(np.load(f"{GOLDEN_DIR}/metrics_{c}.npz")["has_auc"]) for c in CASES) >= 6


def _tied(gen, shape, levels=8):
    return (torch.floor(torch.rand(shape, generator=gen) * levels) / levels).float()


@pytest.mark.parametrize("tied", [False, True])
@pytest.mark.parametrize("P,K", [(1, 1), (7, 3), (200, 64), (333, 257), (50, 1000)])
def test_link_metrics_rows_equals_ranking_metrics(P, K, tied):
    g = torch.Generator().manual_seed(P * 1000 + K)
    pos = _tied(g, P) if tied else torch.rand(P, generator=g)
    neg = _tied(g, (P, K)) if tied else torch.rand(P, K, generator=g)
    want = E.ranking_metrics(pos, neg)
    got = E.link_metrics(pos, neg, k_list=(10, 50, 100), accumulate=torch.float32)
    for key in ("Hits@10", "Hits@50", "Hits@100", "MRR"):
        assert got[key] == want[key], key
    # the fp64 accumulation (the default) agrees to what a float32 mean can hold
    got64 = E.link_metrics(pos, neg, k_list=(10, 50, 100))
    for key in ("Hits@10", "Hits@50", "Hits@100", "MRR"):
        assert abs(got64[key] - want[key]) <= F32_MEAN_TOL, key


@pytest.mark.parametrize("tied", [False, True])
@pytest.mark.parametrize("P,M", [(1, 1), (5, 19), (100, 20), (400, 1000), (77, 4097)])
def test_shared_hits_equals_hits_at_k(P, M, tied):
    g = torch.Generator().manual_seed(P * 7 + M)
    pos = _tied(g, P) if tied else torch.rand(P, generator=g)
    neg = _tied(g, M) if tied else torch.rand(M, generator=g)
    ks = (1, 20, 50, 100)
    got32 = E.link_metrics(pos, neg, k_list=ks, accumulate=torch.float32)
    got64 = E.link_metrics(pos, neg, k_list=ks)
    for k in ks:
        want = E.hits_at_k(pos, neg, k)
        assert got32[f"Hits@{k}"] == want
        assert abs(got64[f"Hits@{k}"] - want) <= 2.0 ** -24     # one float32 rounding of count / P
        if M >= k:
            assert got64[f"Hits@{k}"] == float((pos > torch.topk(neg, k).values[-1]).sum()) / P


def _special(n, seed):
    """Scores over a few values with NaNs of both signs, signed zeros and infinities."""
    nan_neg_sign = np.array([0xFFC00000], dtype=np.uint32).view(np.float32)[0]
    vals = np.array([np.nan, nan_neg_sign, 0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 0.5, 1e-45, -1e-45, 3e38],
                    dtype=np.float32)
    idx = np.random.default_rng(seed).integers(0, len(vals), size=n)
    return torch.from_numpy(vals[idx])


@pytest.mark.parametrize("shape", [(64, 33), (9, 1), (30, 300)])
def test_special_values_rows(shape):
    P, K = shape
    pos, neg = _special(P, 1), _special(P * K, 2).view(P, K)
    ge, gt = E.rank_counts(pos, neg)
    for i in range(P):
        assert int(ge[i]) == int((neg[i] >= pos[i]).sum()) and int(gt[i]) == int((neg[i] > pos[i]).sum())
    m = E.link_metrics(pos, neg, auc=False)
    assert m["nan_pos"] == int(torch.isnan(pos).sum()) and m["nan_neg"] == int(torch.isnan(neg).sum())
    assert m["nan_pos"] > 0 and m["nan_neg"] > 0


@pytest.mark.parametrize("P,M", [(40, 1), (40, 2), (64, 500), (10, 5000)])
def test_special_values_shared(P, M):
    pos, neg = _special(P, 3), _special(M, 4)
    ge, gt = E.rank_counts(pos, neg)
    for i in range(P):
        assert int(ge[i]) == int((neg >= pos[i]).sum()) and int(gt[i]) == int((neg > pos[i]).sum())
    sn = E.sort_negatives(neg)
    ge2, gt2 = E.rank_counts(pos, sn)
    assert torch.equal(ge, ge2) and torch.equal(gt, gt2)
    m = E.link_metrics(pos, sn)
    assert m["nan_pos"] == int(torch.isnan(pos).sum()) and m["nan_neg"] == int(torch.isnan(neg).sum())
    nanp = torch.isnan(pos)
    assert bool((ge[nanp] == 0).all()) and bool((gt[nanp] == 0).all())


def test_signed_zero_and_inf_literals():
    pos = torch.tensor([0.0, -0.0, float("inf"), float("-inf")])
    neg = torch.tensor([-0.0, 0.0, float("inf"), float("-inf"), float("nan")])
    ge, gt = E.rank_counts(pos, neg)
    assert ge.tolist() == [3, 3, 1, 4] and gt.tolist() == [1, 1, 0, 3]
    ge, gt = E.rank_counts(pos, neg.repeat(4, 1))
    assert ge.tolist() == [3, 3, 1, 4] and gt.tolist() == [1, 1, 0, 3]


def test_empty_inputs():
    e = torch.empty(0)
    ge, gt = E.rank_counts(e, torch.rand(5))
    assert ge.numel() == 0 and gt.numel() == 0
    ge, gt = E.rank_counts(torch.rand(4), e)
    assert ge.tolist() == [0] * 4 and gt.tolist() == [0] * 4
    ge, gt = E.rank_counts(torch.rand(4), torch.empty(4, 0))
    assert ge.tolist() == [0] * 4
    assert E.ranks(torch.rand(3), e).tolist() == [1.0] * 3
    m = E.link_metrics(torch.rand(4), e)
    assert m["Hits@20"] == 1.0 and m["MRR"] == 1.0 and np.isnan(m["AUC"])


def test_argument_errors():
    pos, neg = torch.rand(4), torch.rand(5, 3)
    with pytest.raises(ValueError):
        E.rank_counts(pos, neg)                           # one row per positive
    with pytest.raises(ValueError):
        E.rank_counts(pos, torch.rand(4, 3, 2))
    with pytest.raises(TypeError):
        E.rank_counts(pos, torch.ones(7, dtype=torch.int64))
    with pytest.raises(TypeError):
        E.rank_counts(torch.ones(4, dtype=torch.int32), torch.rand(7))
    with pytest.raises(ValueError):
        E.link_metrics(pos, torch.rand(7), k_list=(0,))
    with pytest.raises(ValueError):
        E.link_metrics(pos, torch.rand(7), accumulate=torch.float16)
    with pytest.raises(ValueError):
        E.split_metrics(pos, pos, torch.rand(7), pos, torch.rand(7), layout="columns")
    with pytest.raises(ValueError):
        E.split_metrics(pos, pos, torch.rand(7), pos, torch.rand(7), layout="rows")
    with pytest.raises(ValueError):
        E.split_metrics(torch.rand(3), pos, torch.rand(4, 6), pos, torch.rand(4, 6), layout="rows")


def test_split_metrics_rows_layout():
    g = torch.Generator().manual_seed(5)
    ptr, pv, pt = _tied(g, 30), _tied(g, 30), _tied(g, 21)
    nv, nt = _tied(g, (30, 40)), _tied(g, (21, 55))
    out = E.split_metrics(ptr, pv, nv, pt, nt, k_list=(20, 50), layout="rows")
    for i, (p, n) in enumerate(((ptr, nv), (pv, nv), (pt, nt))):
        one = E.link_metrics(p, n, k_list=(20, 50))
        for key in ("Hits@20", "Hits@50", "MRR", "AUC", "AP", "nan_pos", "nan_neg"):
            assert out[key][i] == one[key]
        flat = E.link_metrics(p, n.reshape(-1), k_list=(20,))
        assert (one["AUC"], one["AP"]) == (flat["AUC"], flat["AP"])
        assert abs(one["MRR"] - E.ranking_metrics(p, n)["MRR"]) <= F32_MEAN_TOL


SWEEP = [(seed, P, M, levels) for seed in range(4) for P, M in ((1, 1), (3, 50), (60, 7), (250, 400))
         for levels in (2, 8, 1 << 20)]


@pytest.mark.parametrize("seed,P,M,levels", SWEEP)
def test_auc_ap_identities_against_sklearn(seed, P, M, levels):
    metrics = pytest.importorskip("sklearn.metrics")
    g = torch.Generator().manual_seed(seed * 7919 + P * 31 + M + levels)
    pos, neg = _tied(g, P, levels), _tied(g, M, levels)
    m = E.link_metrics(pos, neg)
    pred = torch.cat([pos, neg]).numpy()
    true = np.concatenate([np.ones(P, np.int64), np.zeros(M, np.int64)])
    assert abs(m["AUC"] - float(metrics.roc_auc_score(true, pred))) <= F64_TOL
    assert abs(m["AP"] - float(metrics.average_precision_score(true, pred))) <= F64_TOL
