"""pair_heuristics (lpf_pair_heuristics_f32 + the PPR / feature lookups) and the binned metrics on the MI355X, against
scipy on the host: CN = A A^T, AA / RA = A diag(w) A^T in fp64 (the dense rows of src/train/eval.py:21-41)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import lpformer_amd
from lpformer_amd import data as D
from lpformer_amd import evaluate as E
from lpformer_amd import graph, sources
from lpformer_amd.heuristics import pair_heuristics
from tests.golden_util import Fixture

pytestmark = pytest.mark.gpu
RTOL = 1e-5
DEV = torch.device("cuda:0")


def _build(fx):
    """Model + score head on cuda:0 from a fixture, graph entries as torch sparse COO tensors (as the parity tests)."""
    n = fx.n
    data = {"x": torch.from_numpy(fx["x"]).to(DEV), "num_nodes": n}

    def pack(ei_key, w_key, ppr_prefix):
        ei = fx[ei_key].astype(np.int64)
        adj_t = graph.csr_from_coo(ei[0], ei[1], fx[w_key], n)
        mask = graph.mask_csr(ei, n, symmetric=True)
        ppr = graph.csr_from_coo(fx[ppr_prefix + "row"], fx[ppr_prefix + "col"], fx[ppr_prefix + "val"], n)
        return adj_t.to_torch_sparse_coo().to(DEV), mask.to_torch_sparse_coo().to(DEV).int(), \
            ppr.to_torch_sparse_coo().to(DEV)

    data["adj_t"], data["adj_mask"], data["ppr"] = pack("edge_index", "edge_weight", "ppr_")
    if fx.test_set:
        data["full_adj_t"], data["full_adj_mask"], data["ppr_test"] = pack("full_edge_index", "full_edge_weight",
                                                                            "ppr_test_")
    else:
        data["full_adj_t"], data["full_adj_mask"], data["ppr_test"] = data["adj_t"], data["adj_mask"], data["ppr"]
    cfg = {k: fx.cfg[k] for k in ("thresh_cn", "thresh_1hop", "thresh_non1hop", "dim", "trans_layers", "num_heads",
                                  "att_drop", "dropout", "gnn_drop", "feat_drop", "gcn_cache", "gnn_layers",
                                  "residual", "layer_norm", "relu")}
    model = lpformer_amd.LinkTransformer(cfg, data, device=DEV).to(DEV)
    score = lpformer_amd.mlp_score(model.out_dim, model.out_dim, 1, fx.cfg["pred_layers"]).to(DEV)
    m_sd, s_sd = fx.state_dicts()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in m_sd.items()}, strict=True)
    score.load_state_dict({k: torch.from_numpy(v) for k, v in s_sd.items()}, strict=True)
    return model.eval(), score.eval()


def _adj(ei, n):
    """Binary symmetric adjacency (the typing adjacency: adj_t.to_symmetric() ... .bool().int(), read_datasets.py)."""
    m = graph.mask_csr(np.asarray(ei, np.int64), n, symmetric=True)
    return sp.csr_matrix((np.ones(m.nnz), m.col, m.rowptr), shape=(n, n))


def _weights(A):
    deg = np.asarray(A.sum(axis=1)).ravel()
    with np.errstate(divide="ignore"):
        w_aa = np.where(deg > 1, 1.0 / np.log(np.maximum(deg, 2.0)), 0.0)
        w_ra = np.where(deg > 0, 1.0 / np.maximum(deg, 1.0), 0.0)
    return w_aa, w_ra


def _scipy_full(A, pairs):
    """CN / AA / RA of the pairs from the full products A A^T and A diag(w) A^T (fp64; small graphs)."""
    w_aa, w_ra = _weights(A)
    a, b = pairs
    cn = np.asarray((A @ A.T)[a, b]).ravel()
    aa = np.asarray((A @ sp.diags(w_aa) @ A.T)[a, b]).ravel()
    ra = np.asarray((A @ sp.diags(w_ra) @ A.T)[a, b]).ravel()
    return cn, aa, ra


def _scipy_rows(A, pairs):
    """Same quantities restricted to the requested pairs: row a of A .* row b of A, then @ (1, w_aa, w_ra) in fp64
    (a hub graph's A A^T holds hundreds of millions of entries)."""
    w_aa, w_ra = _weights(A)
    a, b = pairs
    cn, aa, ra = [], [], []
    for lo in range(0, a.size, 50_000):
        M = A[a[lo:lo + 50_000]].multiply(A[b[lo:lo + 50_000]]).tocsr()
        cn.append(np.asarray(M.sum(axis=1)).ravel())
        aa.append(M @ w_aa)
        ra.append(M @ w_ra)
    return np.concatenate(cn), np.concatenate(aa), np.concatenate(ra)


def _check(h, ref, what=""):
    cn, aa, ra = ref
    got_cn = h["cn"].cpu().numpy()
    assert got_cn.dtype == np.int32
    np.testing.assert_array_equal(got_cn, cn.astype(np.int64), err_msg=f"cn {what}")
    for k, r in (("aa", aa), ("ra", ra)):
        g = h[k].cpu().numpy().astype(np.float64)
        bad = np.abs(g - r) > RTOL * np.abs(r)
        assert not bad.any(), f"{k} {what}: {int(bad.sum())} pairs off, e.g. got {g[bad][:4]} want {r[bad][:4]}"


def _extra_pairs(n, deg, rng, count=400):
    """Fixture batch extras: a == b, isolated nodes (if any), both orders of random pairs."""
    iso = np.flatnonzero(deg == 0)
    nodes = np.arange(n)
    self_pairs = np.stack([nodes, nodes])
    rnd = rng.integers(0, n, size=(2, count))
    extra = [self_pairs, rnd, rnd[::-1]]
    if iso.size:
        extra.append(np.stack([iso, rng.integers(0, n, size=iso.size)]))
        extra.append(np.stack([iso, iso]))
    return np.concatenate(extra, axis=1).astype(np.int64)


@pytest.mark.parametrize("case", ["lp_all_d64", "lp_all_d128_weighted", "lp_all_d64_maskedadj"])
def test_fixtures_match_scipy(case):
    fx = Fixture(case)
    model, _ = _build(fx)
    A = _adj(fx["edge_index"], fx.n)
    rng = np.random.default_rng(0)
    pairs = np.concatenate([fx["batch"].astype(np.int64), _extra_pairs(fx.n, np.diff(A.indptr), rng)], axis=1)
    h = pair_heuristics(model, torch.from_numpy(pairs))
    assert all(v.is_cuda and v.shape == (pairs.shape[1],) for v in h.values())
    _check(h, _scipy_full(A, pairs), case)
    # a == b: deg(a) common neighbours; the [P, 2] layout gives the same bits
    same = pairs[0] == pairs[1]
    np.testing.assert_array_equal(h["cn"].cpu().numpy()[same], np.diff(A.indptr)[pairs[0][same]])
    h2 = pair_heuristics(model, torch.from_numpy(pairs.T.copy()).to(DEV))
    for k in ("cn", "aa", "ra"):
        assert torch.equal(h[k], h2[k])
    # ids outside [0, n): zeros, no fault
    bad = torch.tensor([[-1, fx.n, 0, 5], [3, 2, fx.n + 7, -9]])
    hb = pair_heuristics(model, bad)
    assert not hb["cn"].any() and not hb["aa"].any() and not hb["ra"].any()


@pytest.fixture(scope="module")
def hub_graph():
    n = 30_000
    ei, _ = D.chung_lu_graph(n, 300_000, gamma=2.2, seed=5)
    A = _adj(ei, n)
    deg = np.diff(A.indptr)
    assert deg.max() >= 2000          # hubs of thousands: hub x hub pairs walk long rows
    hubs = np.argsort(-deg, kind="stable")[:64]
    leaves = np.flatnonzero((deg > 0) & (deg <= 3))[:300]
    rng = np.random.default_rng(1)
    hh = np.stack(np.meshgrid(hubs, hubs, indexing="ij")).reshape(2, -1)
    hl = np.stack(np.meshgrid(hubs, leaves, indexing="ij")).reshape(2, -1)
    pairs = np.concatenate([hh, hl, hl[::-1], rng.integers(0, n, size=(2, 200_000))], axis=1).astype(np.int64)
    csr = graph.mask_csr(ei, n, symmetric=True)
    return csr, A, pairs, _scipy_rows(A, pairs)


def test_hub_graph_default_and_split_path(hub_graph):
    csr, A, pairs, ref = hub_graph
    dcsr = csr.to_device(DEV)
    e = torch.from_numpy(pairs).to(DEV)
    h_def = pair_heuristics(dcsr, e)
    _check(h_def, ref, "default threshold")
    h_split = pair_heuristics(dcsr, e, split_threshold=0)        # every pair with a non-empty walk: a workgroup each
    _check(h_split, ref, "split path only")
    assert torch.equal(h_def["cn"], h_split["cn"])
    h_csr = pair_heuristics(csr, e)                              # a host CSR source: uploaded (and cached) once
    for k in ("cn", "aa", "ra"):
        assert torch.equal(h_def[k], h_csr[k])


@pytest.mark.parametrize("thr", [-1, 0, 16])
def test_bitwise_symmetric_and_repeatable(hub_graph, thr):
    csr, _, pairs, _ = hub_graph
    dcsr = csr.to_device(DEV)
    e = torch.from_numpy(pairs).to(DEV)
    h1 = pair_heuristics(dcsr, e, split_threshold=thr)
    h2 = pair_heuristics(dcsr, e, split_threshold=thr)
    hf = pair_heuristics(dcsr, e.flip(0), split_threshold=thr)
    perm = torch.randperm(e.shape[1], generator=torch.Generator().manual_seed(3)).to(DEV)
    hp = pair_heuristics(dcsr, e[:, perm], split_threshold=thr)
    for k in ("cn", "aa", "ra"):
        assert torch.equal(h1[k], h2[k]), k
        assert torch.equal(h1[k].view(torch.int32), hf[k].view(torch.int32)), k     # h(a, b) == h(b, a), bitwise
        assert torch.equal(h1[k][perm].view(torch.int32), hp[k].view(torch.int32)), k   # position in the batch


def test_test_set_uses_full_adjacency():
    fx = Fixture("lp_all_d64_residual_valtest")
    model, _ = _build(fx)
    rng = np.random.default_rng(2)
    pairs = np.concatenate([fx["batch"].astype(np.int64), rng.integers(0, fx.n, size=(2, 20_000))], axis=1)
    e = torch.from_numpy(pairs)
    h_tr = pair_heuristics(model, e, test_set=False)
    h_te = pair_heuristics(model, e, test_set=True)
    _check(h_tr, _scipy_full(_adj(fx["edge_index"], fx.n), pairs), "train adjacency")
    _check(h_te, _scipy_full(_adj(fx["full_edge_index"], fx.n), pairs), "full adjacency")
    assert not torch.equal(h_tr["cn"], h_te["cn"])


@pytest.mark.parametrize("case", ["lp_all_d64", "lp_all_d64_residual_valtest"])
def test_ppr_and_feature_kinds(case):
    fx = Fixture(case)
    model, _ = _build(fx)
    rng = np.random.default_rng(4)
    pairs = np.concatenate([fx["batch"].astype(np.int64), rng.integers(0, fx.n, size=(2, 3000))], axis=1)
    h = pair_heuristics(model, torch.from_numpy(pairs), test_set=fx.test_set, kinds=("ppr", "feat"))
    assert set(h) == {"ppr_ab", "ppr_ba", "feat"}
    r, c, v = fx.ppr_coo
    M = graph.csr_from_coo(r, c, v, fx.n)
    P = sp.csr_matrix((M.val, M.col, M.rowptr), shape=(fx.n, fx.n))
    assert P.dtype == np.float32
    want_ab = np.asarray(P[pairs[0], pairs[1]]).ravel().astype(np.float32)
    want_ba = np.asarray(P[pairs[1], pairs[0]]).ravel().astype(np.float32)
    np.testing.assert_array_equal(h["ppr_ab"].cpu().numpy().view(np.uint32), want_ab.view(np.uint32))
    np.testing.assert_array_equal(h["ppr_ba"].cpu().numpy().view(np.uint32), want_ba.view(np.uint32))
    x = torch.from_numpy(fx["x"])
    want = torch.nn.functional.cosine_similarity(x[pairs[0]], x[pairs[1]], dim=1)
    assert float((h["feat"].cpu() - want).abs().max()) <= 1e-6
    # x as an nn.Parameter (ogbl-ddi learns its node embedding)
    model.data["x"] = torch.nn.Parameter(torch.from_numpy(fx["x"]).to(DEV))
    hp = pair_heuristics(model, torch.from_numpy(pairs), kinds="feat")
    assert float((hp["feat"].cpu() - want).abs().max()) <= 1e-6


def test_model_sources_are_the_resident_graphs():
    """The analysis entry points read the resident graphs the selection reads, and make no copy of their own."""
    fx = Fixture("lp_all_d64_residual_valtest")
    model, _ = _build(fx)
    e = torch.from_numpy(fx["batch"].astype(np.int64))
    lpformer_amd.pair_heuristics(model, e, test_set=True)
    resident = len(model._graphs)
    lpformer_amd.pair_distance(model, e, test_set=True)
    lpformer_amd.threshold_profile(model, e, test_set=True)
    lpformer_amd.pair_heuristics(model, e, test_set=True, kinds=("ppr",))
    assert len(model._graphs) == resident
    for ts in (False, True):
        dev, adj, ppr = sources.model_graphs(model, ts, "test")
        assert dev == model.device
        assert adj is model._device_graph("mask", model._data_obj("mask", ts))
        assert ppr is model._device_graph("ppr", model._data_obj("ppr", ts))
    assert adj is not sources.model_graphs(model, False, "test")[1]       # (this fixture's splits differ)


def _np_hits(pos, neg, k):
    if neg.size < k:
        return 1.0
    return float(np.sum(pos > np.sort(neg)[::-1][k - 1])) / pos.size


def test_end_to_end_binned_hits():
    fx = Fixture("lp_all_d64")
    model, score = _build(fx)
    rng = np.random.default_rng(5)
    pos = fx["batch"].astype(np.int64)
    neg = rng.integers(0, fx.n, size=(2, 700))
    pos_s = E.score_edges(model, score, torch.from_numpy(pos))
    neg_s = E.score_edges(model, score, torch.from_numpy(neg))
    cn = pair_heuristics(model, torch.from_numpy(pos), kinds=("cn",))["cn"]
    assert set(pair_heuristics(model, torch.from_numpy(pos), kinds=("cn",))) == {"cn"}
    got = E.metrics_by_bin(pos_s, neg_s, cn)
    ref_cn = _scipy_full(_adj(fx["edge_index"], fx.n), pos)[0]
    ps, ns = pos_s.cpu().numpy(), neg_s.cpu().numpy()
    for g, (lo, hi) in zip(got, E.CN_BINS):
        ix = (ref_cn >= lo) & (ref_cn < hi)
        assert g["count"] == int(ix.sum())
        for k in (20, 50, 100):
            if ix.any():
                assert g[f"Hits@{k}"] == pytest.approx(_np_hits(ps[ix], ns, k), abs=1e-7)
            else:
                assert np.isnan(g[f"Hits@{k}"])
    assert sum(g["count"] for g in got) == pos.shape[1]


def test_empty_single_and_chunked_batches(hub_graph):
    csr, A, pairs, ref = hub_graph
    dcsr = csr.to_device(DEV)
    h0 = pair_heuristics(dcsr, torch.zeros(2, 0, dtype=torch.int64))
    assert set(h0) == {"cn", "aa", "ra"} and all(v.numel() == 0 and v.is_cuda for v in h0.values())
    h0 = pair_heuristics(dcsr, torch.zeros(0, 2, dtype=torch.int64), kinds=("ra",))
    assert set(h0) == {"ra"} and h0["ra"].numel() == 0
    hub = int(np.argmax(np.diff(A.indptr)))
    one = np.array([[hub], [hub]])
    h1 = pair_heuristics(dcsr, torch.from_numpy(one))
    _check(h1, _scipy_rows(A, one), "single pair")
    sub = pairs[:, -10_000:]
    e = torch.from_numpy(sub).to(DEV)
    whole = pair_heuristics(dcsr, e)
    for chunk in (1, 63, 64, 4097):
        parts = pair_heuristics(dcsr, e, chunk=chunk)
        for k in ("cn", "aa", "ra"):
            assert torch.equal(whole[k], parts[k]), (chunk, k)
    _check(whole, tuple(r[-10_000:] for r in ref), "chunk boundaries")
    only_aa = pair_heuristics(dcsr, e, kinds=("aa",), chunk=999)
    assert set(only_aa) == {"aa"} and torch.equal(only_aa["aa"], whole["aa"])
