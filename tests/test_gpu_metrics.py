"""lpf_rank_rows_f32 / lpf_rank_shared_f32 behind lpformer_amd.evaluate on the MI355X: against the CPU path of the
same functions, the literal torch expressions and the reference's recorded outputs (tests/golden/metrics_*.npz).
Counts are compared for equality; aggregates to 1e-9 (fp64 sums of P <= 1e5 terms: P * 2^-53 with room)."""
import numpy as np
import pytest
import torch

from lpformer_amd import _lib
from lpformer_amd import evaluate as E
from tests.golden_util import LP_CASES, Fixture
from tests.test_metrics_host import CASES, F64_TOL, _special, _tied, load

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
AGG = ("MRR", "AUC", "AP")


def _same_metrics(got, want, exact=False):
    assert got.keys() == want.keys()
    for k, w in want.items():
        ws, gs = (w, got[k]) if isinstance(w, tuple) else ((w,), (got[k],))
        for g1, w1 in zip(gs, ws):
            if isinstance(w1, float) and np.isnan(w1):
                assert np.isnan(g1), k
            elif exact or not k.startswith(AGG):
                assert g1 == w1, (k, g1, w1)
            else:
                assert abs(g1 - w1) <= F64_TOL, (k, g1, w1)


def _literal_rows(pos, neg):
    col = pos.reshape(-1, 1)
    return (neg >= col).sum(1).int(), (neg > col).sum(1).int()


@pytest.mark.parametrize("case", CASES)
def test_fixtures_on_device(case):
    z, t = load(case)
    d = {k: v.to(DEV) for k, v in t.items()}
    ks = tuple(int(k) for k in z["ks"])
    np.testing.assert_array_equal(E.ranks(d["pos"], d["neg_rows"]).cpu().numpy(), z["rows_ranking_list"])
    for tag, p, n in (("train", "pos_train", "neg"), ("valid", "pos", "neg"), ("test", "pos_test", "neg_test")):
        np.testing.assert_array_equal(E.ranks(d[p], d[n]).cpu().numpy(), z[f"shared_ranking_list_{tag}"])
        sh = E.sample_hits(d[p], d[n], ks=ks)
        for k in ks:
            np.testing.assert_array_equal(sh[f"Hits@{k}"].cpu().numpy(), z[f"shared_sample_{tag}_Hits@{k}"])
    out = E.split_metrics(d["pos_train"], d["pos"], d["neg"], d["pos_test"], d["neg_test"], k_list=ks)
    _same_metrics(out, E.split_metrics(t["pos_train"], t["pos"], t["neg"], t["pos_test"], t["neg_test"], k_list=ks))
    for k in ks:
        assert out[f"Hits@{k}"] == tuple(float(v) for v in z[f"split_Hits@{k}"])
    for i in range(3):
        assert abs(out["MRR"][i] - float(z["split_mrr64"][i])) <= F64_TOL
    if int(z["has_auc"]):
        assert abs(out["AUC"][1] - float(z["auc"])) <= F64_TOL and abs(out["AP"][1] - float(z["ap"])) <= F64_TOL
        assert round(out["AUC"][1], 4) == float(z["auc_rounded"]) and round(out["AP"][1], 4) == float(z["ap_rounded"])
    m = E.link_metrics(d["pos"], d["neg_rows"], k_list=(10, 50, 100))
    _same_metrics(m, E.link_metrics(t["pos"], t["neg_rows"], k_list=(10, 50, 100)))
    assert abs(m["MRR"] - float(z["rows_mrr64"])) <= F64_TOL


@pytest.mark.parametrize("layout", ["plain", "strided", "unaligned"])
@pytest.mark.parametrize("K", [1, 3, 63, 64, 65, 100, 257, 1000, 4099])
def test_rows_kernel(K, layout):
    P = 301
    g = torch.Generator().manual_seed(K)
    pos = _tied(g, P, 64).to(DEV)
    if layout == "plain":
        neg = _tied(g, (P, K), 64).to(DEV)
    elif layout == "strided":                     # a view with row stride K + 5
        neg = _tied(g, (P, K + 5), 64).to(DEV)[:, 3:3 + K]
        assert neg.stride(0) == K + 5
    else:                                         # the base one float past a 16-byte boundary
        neg = _tied(g, P * K + 1, 64).to(DEV)[1:].view(P, K)
        assert neg.data_ptr() % 16 == 4
    ge, gt = E.rank_counts(pos, neg)
    wge, wgt = _literal_rows(pos, neg)
    assert torch.equal(ge, wge) and torch.equal(gt, wgt)
    cge, cgt = E.rank_counts(pos.cpu(), neg.cpu())
    assert torch.equal(ge.cpu(), cge) and torch.equal(gt.cpu(), cgt)
    ge2, gt2 = E.rank_counts(pos, neg)
    assert torch.equal(ge, ge2) and torch.equal(gt, gt2)
    want = E.ranking_metrics(pos, neg)
    got = E.link_metrics(pos, neg, k_list=(10, 50, 100), accumulate=torch.float32)
    for key in want:
        assert got[key] == want[key], key
    _same_metrics(E.link_metrics(pos, neg), E.link_metrics(pos.cpu(), neg.cpu()))


@pytest.mark.parametrize("K", [3, 100, 1000])
def test_rows_kernel_special_values(K):
    P = 200
    pos, neg = _special(P, K).to(DEV), _special(P * K, K + 1).view(P, K).to(DEV)
    ge, gt = E.rank_counts(pos, neg)
    wge, wgt = _literal_rows(pos, neg)
    assert torch.equal(ge, wge) and torch.equal(gt, wgt)
    m = E.link_metrics(pos, neg)
    assert m["nan_pos"] == int(torch.isnan(pos).sum()) > 0 and m["nan_neg"] == int(torch.isnan(neg).sum()) > 0
    _same_metrics(m, E.link_metrics(pos.cpu(), neg.cpu()))


@pytest.mark.parametrize("kind", ["random", "tied", "special"])
@pytest.mark.parametrize("M", [1, 2, 4095, 4096, 4097, 100_003])
def test_shared_kernel(M, kind):
    P = 1000
    g = torch.Generator().manual_seed(M)
    if kind == "random":
        pos, neg = torch.rand(P, generator=g), torch.rand(M, generator=g)
    elif kind == "tied":
        pos, neg = _tied(g, P), _tied(g, M)
    else:
        pos, neg = _special(P, M), _special(M, M + 1)
    dpos, dneg = pos.to(DEV), neg.to(DEV)
    ge, gt = E.rank_counts(dpos, dneg)
    cge, cgt = E.rank_counts(pos, neg)
    assert torch.equal(ge.cpu(), cge) and torch.equal(gt.cpu(), cgt)
    lge = torch.stack([(dneg >= p).sum() for p in dpos[:64]]).int()
    lgt = torch.stack([(dneg > p).sum() for p in dpos[:64]]).int()
    assert torch.equal(ge[:64], lge) and torch.equal(gt[:64], lgt)
    # a second set of positives against the sorted negatives: no second sort, the same bits
    sn = E.sort_negatives(dneg)
    keys = sn.keys.clone()
    ge2, gt2 = E.rank_counts(dpos, sn)
    ge3, gt3 = E.rank_counts(dpos, sn)
    assert torch.equal(ge, ge2) and torch.equal(gt, gt2) and torch.equal(ge, ge3) and torch.equal(gt, gt3)
    assert torch.equal(keys, sn.keys)
    m = E.link_metrics(dpos, sn)
    assert m["nan_pos"] == int(torch.isnan(pos).sum()) and m["nan_neg"] == int(torch.isnan(neg).sum())
    if kind == "special":
        assert m["nan_pos"] > 0 and (m["nan_neg"] > 0 or M <= 2)
        nanp = torch.isnan(dpos)
        assert bool((ge[nanp] == 0).all()) and bool((gt[nanp] == 0).all())
    _same_metrics(m, E.link_metrics(pos, neg))
    _same_metrics(E.link_metrics(dpos, dneg), m, exact=True)


def test_shared_kernel_nan_of_both_signs():
    bits = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x3F800000, 0x80000000, 0, 0xFF800000,
                     0x7F800000], dtype=np.uint32)
    neg = torch.from_numpy(np.tile(bits, 700).view(np.float32).copy())
    pos = torch.tensor([1.0, 0.0, -0.0, float("inf"), float("-inf"), float("nan"), 2.0, -3.0])
    ge, gt = E.rank_counts(pos.to(DEV), neg.to(DEV))
    assert ge.tolist() == [(neg >= p).sum().item() for p in pos] and gt.tolist() == [(neg > p).sum().item() for p in pos]
    m = E.link_metrics(pos.to(DEV), neg.to(DEV))
    assert m["nan_pos"] == 1 and m["nan_neg"] == 4 * 700


def test_collab_valid_size():
    P, M = 60_084, 100_000
    rng = np.random.default_rng(0)
    pos = rng.random(P, dtype=np.float32)
    neg = np.round(rng.random(M, dtype=np.float32) * 30000) / np.float32(30000)
    pos[::7] = neg[:len(pos[::7])]                      # ties across the classes
    srt = np.sort(neg)
    wge = (M - np.searchsorted(srt, pos, side="left")).astype(np.int32)
    wgt = (M - np.searchsorted(srt, pos, side="right")).astype(np.int32)
    dpos, dneg = torch.from_numpy(pos).to(DEV), torch.from_numpy(neg).to(DEV)
    ge, gt = E.rank_counts(dpos, dneg)
    np.testing.assert_array_equal(ge.cpu().numpy(), wge)
    np.testing.assert_array_equal(gt.cpu().numpy(), wgt)
    nbytes = int(_lib.hip().lpf_rank_shared_workspace_bytes(P, M))
    assert 0 < nbytes <= 64 * (P + M) + (1 << 20)
    m = E.link_metrics(dpos, dneg, k_list=(20, 50, 100))
    _same_metrics(m, E.link_metrics(torch.from_numpy(pos), torch.from_numpy(neg), k_list=(20, 50, 100)))
    _same_metrics(E.link_metrics(dpos, dneg, k_list=(20, 50, 100)), m, exact=True)
    for k in (20, 50, 100):
        assert abs(m[f"Hits@{k}"] - E.hits_at_k(dpos, dneg, k)) <= 2.0 ** -24


def _split_data(fx, heart, seed=0):
    rng = np.random.default_rng(seed)
    ei = fx.edge_index
    n = fx.n

    def some(count):
        return torch.from_numpy(ei[:, rng.permutation(ei.shape[1])[:count]].T.copy())

    def rand(*shape):
        return torch.from_numpy(rng.integers(0, n, size=shape + (2,)))

    data = {"train_pos_val": some(50), "valid_pos": some(50), "test_pos": some(40)}
    data["valid_neg"] = rand(50, 30) if heart else rand(600)
    data["test_neg"] = rand(40, 30) if heart else rand(500)
    return data


@pytest.mark.parametrize("heart", [False, True])
@pytest.mark.parametrize("case", [LP_CASES[0], LP_CASES[2]])
def test_evaluate_model(case, heart):
    from tests.test_gpu_recommend import _build
    fx = Fixture(case)
    model, score = _build(fx)
    data = _split_data(fx, heart)
    ks = (10, 20)
    out = E.evaluate_model(model, score, data, batch_size=256, k_list=ks, heart=heart)
    sc = {k: E.score_edges(model, score, data[k], 256, test_set=k.startswith("test")) for k in
          ("train_pos_val", "valid_pos", "test_pos")}
    if heart:
        nv = E.score_negatives(model, score, data["valid_neg"], 256)
        nt = E.score_negatives(model, score, data["test_neg"], 256, test_set=True)
        assert nv.shape == (50, 30) and nt.shape == (40, 30)
    else:
        nv = E.score_edges(model, score, data["valid_neg"], 256)
        nt = E.score_edges(model, score, data["test_neg"], 256, test_set=True)
    layout = "rows" if heart else "shared"
    want = E.split_metrics(sc["train_pos_val"], sc["valid_pos"], nv, sc["test_pos"], nt, k_list=ks, layout=layout)
    _same_metrics(out, want, exact=True)
    host = E.split_metrics(sc["train_pos_val"].cpu(), sc["valid_pos"].cpu(), nv.cpu(), sc["test_pos"].cpu(), nt.cpu(),
                           k_list=ks, layout=layout)
    _same_metrics(out, host)
    assert set(out) == {"Hits@10", "Hits@20", "MRR", "AUC", "AP", "nan_pos", "nan_neg"}
    assert all(len(v) == 3 for v in out.values()) and out["nan_pos"] == (0, 0, 0)
    _same_metrics(E.evaluate_model(model, score, data, batch_size=256, k_list=ks, heart=heart), out, exact=True)


def test_cpu_tensors_do_not_need_the_device_and_mixing_is_an_error():
    with pytest.raises(ValueError):
        E.rank_counts(torch.rand(4, device=DEV), torch.rand(9))
    with pytest.raises(ValueError):
        E.rank_counts(torch.rand(4), E.sort_negatives(torch.rand(9, device=DEV)))
