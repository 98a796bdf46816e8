"""lpformer_amd.bootstrap without a GPU: the numpy restatement against draws made one at a time on Python integers, what
a replicate means (link_metrics of the drawn positives), the statistics of the resampling (deterministic: the draw is a
pure function of the seed), the paired test and the argument errors."""
import math

import numpy as np
import pytest
import torch

from lpformer_amd import bootstrap as B
from lpformer_amd import evaluate as E
from lpformer_amd import negatives
from tests.bootstrap_cases import SEEDS, mrr_bound, np_indices, py_indices, scores, sum_bound, tables


# ------------------------------------------------------------------------------------- twin against brute force
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("p", (1, 3, 257))
def test_twin_against_python_integers(p, seed):
    reps, first = 4, 2
    icols, fcols = tables(p, 3, 2, rng_seed=p)
    idx = np.array([py_indices(p, first + r, seed) for r in range(reps)], dtype=np.int64)
    np.testing.assert_array_equal(B.bootstrap_indices(p, reps, seed, first=first), idx)
    isum, fsum = B.bootstrap_sums_reference(icols, fcols, reps, seed, first=first)
    want_i = [[sum(int(icols[i, c]) for i in row) for c in range(3)] for row in idx]
    np.testing.assert_array_equal(isum, np.array(want_i, dtype=np.int64))
    want_f = np.array([[math.fsum(fcols[i, c] for i in row) for c in range(2)] for row in idx])
    assert (np.abs(fsum - want_f) <= sum_bound(fcols, idx)).all()
    # one kind of column alone, 1-D columns, CPU tensors: the same numbers
    i1, f0 = B.bootstrap_sums(icols[:, 0], None, reps, seed, first=first)
    np.testing.assert_array_equal(i1[:, 0], isum[:, 0])
    assert f0.shape == (reps, 0)
    ti, tf = B.bootstrap_sums(torch.from_numpy(icols), torch.from_numpy(fcols), reps, seed, first=first)
    np.testing.assert_array_equal(ti.numpy(), isum)
    np.testing.assert_array_equal(tf.numpy(), fsum)


def test_twin_chunks_do_not_change_it(monkeypatch):
    icols, fcols = tables(300, 2, 1)
    want = B.bootstrap_sums_reference(icols, fcols, 9, 5)
    monkeypatch.setattr(B, "_TWIN_DRAWS", 128)          # cuts the replicates AND the draws
    got = B.bootstrap_sums_reference(icols, fcols, 9, 5)
    np.testing.assert_array_equal(got[0], want[0])
    idx = np_indices(300, 9, 5)
    assert (np.abs(got[1] - want[1]) <= sum_bound(fcols, idx)).all()
    a = B.bootstrap_sums_reference(icols, fcols, 4, 5, first=5)
    np.testing.assert_array_equal(a[0], want[0][5:])


# -------------------------------------------------------------------------------------------------------- meaning
KS = (1, 5, 20)


def _check_meaning(pos, neg, layout, reps, seed):
    p = pos.numel()
    out = B.bootstrap_metrics(pos, neg, k_list=KS, replicates=reps, seed=seed, return_replicates=True)
    lm = E.link_metrics(pos, neg, k_list=KS, auc=layout == "shared")
    names = [f"Hits@{k}" for k in KS] + ["MRR"] + (["AUC"] if layout == "shared" else [])
    assert [k for k in out if k not in ("n", "replicates")] == names
    assert out["n"] == p and out["replicates"] == reps
    idx = torch.from_numpy(np_indices(p, reps, seed))
    for name in names:
        assert out[name]["value"] == lm[name], name
        r = out[name]["replicates"]
        assert r.dtype == torch.float64 and r.shape == (reps,)
        assert out[name]["se"] == float(r.std(unbiased=True))
        a = (1 - 0.95) / 2                                            # the quantiles the docstring names, at level 0.95
        assert out[name]["lo"] == float(torch.quantile(r, a)) and out[name]["hi"] == float(torch.quantile(r, 1 - a))
    for b in range(reps):
        want = E.link_metrics(pos[idx[b]], neg if layout == "shared" else neg[idx[b]], k_list=KS, auc=layout == "shared")
        for name in names:
            got = float(out[name]["replicates"][b])
            if name == "MRR":
                assert abs(got - want[name]) <= mrr_bound(p, want[name]), (b, got, want[name])
            else:
                assert got == want[name], (name, b, got, want[name])
    return out


@pytest.mark.parametrize("layout", ("shared", "rows"))
def test_replicate_is_link_metrics_of_the_drawn_positives(layout):
    pos, neg = scores(257, layout)
    _check_meaning(pos, neg, layout, 12, SEEDS[1])


def test_fewer_negatives_than_k():
    pos, neg = scores(40, "shared", m=10)
    out = B.bootstrap_metrics(pos, neg, k_list=(5, 20), replicates=8)
    assert out["Hits@20"] == {"value": 1.0, "se": 0.0, "lo": 1.0, "hi": 1.0}
    assert out["Hits@5"]["value"] == E.link_metrics(pos, neg, k_list=(5,))["Hits@5"]


@pytest.mark.parametrize("layout", ("shared", "rows"))
def test_unit_of_one_positive_each_is_the_plain_bootstrap(layout):
    pos, neg = scores(101, layout)
    plain = B.bootstrap_metrics(pos, neg, k_list=KS, replicates=20, seed=3, return_replicates=True)
    unit = B.bootstrap_metrics(pos, neg, k_list=KS, replicates=20, seed=3, unit=torch.arange(101) * 7 + 2,
                               return_replicates=True)
    assert unit["units"] == 101
    for name in plain:
        if name in ("n", "replicates"):
            continue
        assert torch.equal(plain[name]["replicates"], unit[name]["replicates"]), name
        assert plain[name]["value"] == unit[name]["value"]


def test_repeated_units_against_a_hand_built_ratio_of_sums():
    p, reps, seed = 90, 15, 11
    pos, neg = scores(p, "shared")
    unit = torch.tensor([(7 * j) % 13 for j in range(p)])           # 13 units of unequal size, out of order
    out = B.bootstrap_metrics(pos, neg, k_list=(5,), replicates=reps, seed=seed, unit=unit, return_replicates=True)
    ge, gt = E.rank_counts(pos, neg)
    ge, gt = ge.numpy().astype(np.int64), gt.numpy().astype(np.int64)
    m = neg.numel()
    units = sorted(set(unit.tolist()))
    assert out["units"] == len(units) and out["n"] == p
    rows = [np.flatnonzero(unit.numpy() == u) for u in units]
    hit = np.array([(ge[r] < 5).sum() for r in rows])
    cnt = np.array([len(r) for r in rows])
    aucn = np.array([(2 * m - ge[r] - gt[r]).sum() for r in rows])
    rr = np.array([math.fsum(2.0 / (ge[r] + gt[r] + 2)) for r in rows])
    idx = np_indices(len(units), reps, seed)
    for b in range(reps):
        n = int(cnt[idx[b]].sum())
        assert float(out["Hits@5"]["replicates"][b]) == int(hit[idx[b]].sum()) / n
        assert float(out["AUC"]["replicates"][b]) == int(aucn[idx[b]].sum()) / (2 * m * n)
        want = math.fsum(rr[idx[b]]) / n
        assert abs(float(out["MRR"]["replicates"][b]) - want) <= mrr_bound(p, want)
    lm = E.link_metrics(pos, neg, k_list=(5,))
    assert out["Hits@5"]["value"] == lm["Hits@5"] and out["AUC"]["value"] == lm["AUC"]


# ----------------------------------------------------------------------------------------------------- statistics
def test_standard_error_and_bias_of_a_bernoulli_column():
    p, reps = 4096, 2000
    hits = (np.random.default_rng(7).random(p) < 0.3).astype(np.int64)
    phat = hits.mean()
    for seed in range(5):
        isum, _ = B.bootstrap_sums(hits, None, reps, seed)
        r = isum[:, 0] / p
        se = r.std(ddof=1)
        ratio = se / math.sqrt(phat * (1 - phat) / p)
        bias = abs(r.mean() - phat) / se
        print(f"seed {seed}: se ratio {ratio:.4f}, |bias| / se {bias:.4f}")
        assert 0.92 <= ratio <= 1.08
        assert bias < 0.1


def test_draws_are_uniform():
    p, reps = 257, 4000
    for seed in (3,):
        cells = np.bincount(B.bootstrap_indices(p, reps, seed).reshape(-1), minlength=p)
        chi2 = ((cells - reps) ** 2 / reps).sum()
        z = (chi2 - (p - 1)) / math.sqrt(2 * (p - 1))
        print(f"seed {seed}: chi2 z {z:.3f}")
        assert abs(z) <= 5


# --------------------------------------------------------------------------------------------------------- paired
def _paired_scores():
    p = 4096
    rng = np.random.default_rng(7)
    hit = rng.random(p) < 0.3
    extra = (~hit) & (rng.random(p) < 0.05 / 0.7)                    # about 5 % of the positives
    neg = torch.arange(100, dtype=torch.float32)
    pos_a = torch.where(torch.from_numpy(hit), 200.0, 50.5).float()
    pos_b = torch.where(torch.from_numpy(hit | extra), 200.0, 50.5).float()
    return pos_a, pos_b, neg


def test_paired_test_finds_the_extra_hits():
    reps = 2000
    pos_a, pos_b, neg = _paired_scores()
    out = B.compare_metrics(pos_a, neg, pos_b, neg, k_list=(20,), mrr=False, auc=False, replicates=reps,
                            return_replicates=True)["Hits@20"]
    assert int((out["replicates"] <= 0).sum()) == 0
    assert out["p"] == 2 / (reps + 1)
    assert out["a"] == E.link_metrics(pos_a, neg, k_list=(20,))["Hits@20"]
    assert out["b"] == E.link_metrics(pos_b, neg, k_list=(20,))["Hits@20"]
    assert out["diff"] == out["b"] - out["a"] and out["lo"] > 0
    # the same draws for both systems: the differences are those of two separate bootstraps under one seed
    ra = B.bootstrap_metrics(pos_a, neg, k_list=(20,), mrr=False, auc=False, replicates=reps, return_replicates=True)
    rb = B.bootstrap_metrics(pos_b, neg, k_list=(20,), mrr=False, auc=False, replicates=reps, return_replicates=True)
    assert torch.equal(out["replicates"], rb["Hits@20"]["replicates"] - ra["Hits@20"]["replicates"])


@pytest.mark.parametrize("layout", ("shared", "rows"))
def test_a_system_against_itself(layout):
    pos, neg = scores(200, layout)
    out = B.compare_metrics(pos, neg, pos, neg, k_list=KS, replicates=50)
    for name, res in out.items():
        if name in ("n", "replicates"):
            continue
        assert res["diff"] == 0.0 and res["se"] == 0.0 and res["p"] == 1.0 and res["lo"] == res["hi"] == 0.0


def test_more_than_eight_columns_share_the_draws():
    pos, neg = scores(150, "shared")
    ks = (1, 2, 3, 5, 8, 13, 20)                                      # 8 integer columns per system with AUC: 16 in all
    out = B.compare_metrics(pos, neg, pos + 0.5, neg, k_list=ks, replicates=30, seed=4, return_replicates=True)
    for k in ks:
        a = B.bootstrap_metrics(pos, neg, k_list=(k,), mrr=False, auc=False, replicates=30, seed=4, return_replicates=True)
        b = B.bootstrap_metrics(pos + 0.5, neg, k_list=(k,), mrr=False, auc=False, replicates=30, seed=4,
                                return_replicates=True)
        assert torch.equal(out[f"Hits@{k}"]["replicates"], b[f"Hits@{k}"]["replicates"] - a[f"Hits@{k}"]["replicates"])


# -------------------------------------------------------------------------------------------------------- by bin
@pytest.mark.parametrize("layout", ("shared", "rows"))
def test_by_bin(layout):
    pos, neg = scores(300, layout)
    values = torch.arange(300) % 9                                   # nothing in [10, 1e6)
    plain = E.metrics_by_bin(pos, neg, values, k_list=KS)
    out = B.bootstrap_by_bin(pos, neg, values, k_list=KS, replicates=25, seed=6, return_replicates=True)
    assert [r["bin"] for r in out] == [r["bin"] for r in plain] and [r["count"] for r in out] == [r["count"] for r in plain]
    for i, res in enumerate(out):
        m = (values >= res["bin"][0]) & (values < res["bin"][1])
        if res["count"] == 0:
            assert i == 3
            for name in [f"Hits@{k}" for k in KS] + ["MRR"] + (["AUC"] if layout == "shared" else []):
                assert all(math.isnan(res[name][f]) for f in ("value", "se", "lo", "hi"))
            continue
        want = B.bootstrap_metrics(pos[m], neg[m] if layout == "rows" else neg, k_list=KS, replicates=25,
                                   seed=negatives.step_seed(6, i), return_replicates=True)
        for name in want:
            if name in ("n", "replicates"):
                continue
            assert torch.equal(res[name]["replicates"], want[name]["replicates"])
            assert res[name]["value"] == want[name]["value"]
        lm = E.link_metrics(pos[m], neg[m] if layout == "rows" else neg, k_list=KS, auc=False)
        assert all(res[f"Hits@{k}"]["value"] == lm[f"Hits@{k}"] for k in KS) and res["MRR"]["value"] == lm["MRR"]


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors():
    pos, neg = scores(20, "shared")
    _, rows = scores(20, "rows")
    with pytest.raises(ValueError):
        B.bootstrap_metrics(pos, rows, auc=True)
    with pytest.raises(ValueError):
        B.compare_metrics(pos, rows, pos, rows, auc=True)
    with pytest.raises(ValueError):
        B.bootstrap_metrics(pos, rows[:-1])
    with pytest.raises(ValueError):
        B.compare_metrics(pos, neg, pos[:-1], neg)
    with pytest.raises(ValueError):
        B.bootstrap_metrics(pos, neg, unit=torch.arange(19))
    with pytest.raises(ValueError):
        B.bootstrap_by_bin(pos, neg, torch.arange(19))
    for level in (0.0, 1.0, -0.5, 1.5):
        with pytest.raises(ValueError):
            B.bootstrap_metrics(pos, neg, level=level)
    for reps in (0, -3):
        with pytest.raises(ValueError):
            B.bootstrap_metrics(pos, neg, replicates=reps)
        with pytest.raises(ValueError):
            B.bootstrap_sums(np.zeros(4, dtype=np.int64), replicates=reps)
    with pytest.raises(ValueError):
        B.bootstrap_sums(np.zeros((4, 2), dtype=np.int64), np.zeros((5, 1)))
    with pytest.raises(ValueError):
        B.bootstrap_sums(np.zeros((4, 9), dtype=np.int64))
    with pytest.raises(ValueError):
        B.bootstrap_sums()
    with pytest.raises(ValueError):
        B.bootstrap_sums(np.zeros((0, 1), dtype=np.int64))
    with pytest.raises(ValueError):
        B.bootstrap_metrics(pos[:0], neg)


def test_a_table_of_two_to_the_31_rows_is_refused_without_allocating():
    one = np.zeros((1, 1), dtype=np.int64)
    for table in (np.broadcast_to(one, (2 ** 31, 1)), torch.zeros(1, 1, dtype=torch.int64).expand(2 ** 31, 1)):
        with pytest.raises(ValueError, match="2\\^31"):
            B.bootstrap_sums(table, None, 1)                          # a copy of it would be 16 GiB
    with pytest.raises(ValueError, match="2\\^31"):
        B.bootstrap_sums_reference(np.broadcast_to(one, (2 ** 31, 1)), None, 1)
    with pytest.raises(ValueError):
        B.bootstrap_indices(2 ** 31)
