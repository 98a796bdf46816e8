"""recommend (lpf_rec_candidate_count / _fill, lpf_segment_topk_f32, score_edges in between) on the MI355X, against
numpy restatements on the host: candidates = PPR row (or every node) minus the exclusion row minus u; top-K = a stable
lexsort of (score key descending, position ascending)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import lpformer_amd
from lpformer_amd import data as D
from lpformer_amd import evaluate as E
from lpformer_amd import graph
from lpformer_amd.recommend import generate_candidates, segment_topk
from oracle import lpformer_oracle as O
from tests.golden_util import LP_CASES, Fixture

pytestmark = pytest.mark.gpu
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


# ------------------------------------------------------------------------------------------------ host restatements
def _sp_ppr(row, col, val, n):
    m = sp.csr_matrix((np.asarray(val, np.float32), (np.asarray(row, np.int64), np.asarray(col, np.int64))),
                      shape=(n, n))
    m.sort_indices()
    return m


def _sp_adj(ei, n):
    ei = np.asarray(ei, np.int64)
    r, c = np.concatenate([ei[0], ei[1]]), np.concatenate([ei[1], ei[0]])
    m = sp.csr_matrix((np.ones(r.size), (r, c)), shape=(n, n))
    m.sum_duplicates()
    m.sort_indices()
    return m


def _np_candidates(sources, n, ppr, min_ppr, exc, exclude_self):
    """Per source: ascending v of (PPR row with value > 0 and >= min_ppr, or all of [0, n)) minus exc row minus u."""
    out = []
    for u in sources:
        if ppr is None:
            v = np.arange(n, dtype=np.int64)
        else:
            lo, hi = ppr.indptr[u], ppr.indptr[u + 1]
            cols, vals = ppr.indices[lo:hi].astype(np.int64), ppr.data[lo:hi].astype(np.float32)
            v = cols[(vals > 0) & (vals >= np.float32(min_ppr))]
        if exc is not None:
            v = v[~np.isin(v, exc.indices[exc.indptr[u]:exc.indptr[u + 1]])]
        if exclude_self:
            v = v[v != u]
        out.append(v)
    return out


def _order_key(s):
    """The documented ranking key of float32 scores as uint32: -0.0 -> +0.0, NaN below -inf."""
    b = np.asarray(s, np.float32).view(np.uint32).copy()
    b[b == 0x80000000] = 0
    key = np.where(b & 0x80000000, ~b, b | 0x80000000).astype(np.uint32)
    key[np.isnan(np.asarray(s, np.float32))] = 0
    return key


def _np_topk(seg_ptr, score, cand, k):
    S = len(seg_ptr) - 1
    ids = np.full((S, k), -1, np.int64)
    out = np.full((S, k), -np.inf, np.float32)
    cnt = np.zeros(S, np.int64)
    key = _order_key(score)
    for s in range(S):
        lo, hi = seg_ptr[s], seg_ptr[s + 1]
        pos = np.arange(hi - lo)
        order = np.lexsort((pos, -key[lo:hi].astype(np.int64)))[:k]     # key descending, then position ascending
        c = order.size
        ids[s, :c], out[s, :c], cnt[s] = cand[lo:hi][order], score[lo:hi][order], c
    return ids, out, cnt


def _run_candidates(sources, n, include, min_ppr, exclude, exclude_self, thr=-1):
    src = torch.as_tensor(np.asarray(sources, np.int64)).to(DEV)
    counts, fill = generate_candidates(n, src, include, min_ppr, exclude, exclude_self, thr)
    total = int(counts.sum())
    pairs = fill(0, src.numel(), total).cpu().numpy()
    return counts.cpu().numpy(), pairs


def _check_candidates(sources, counts, pairs, want, what):
    np.testing.assert_array_equal(counts, [w.size for w in want], err_msg=f"counts {what}")
    np.testing.assert_array_equal(pairs[0], np.repeat(np.asarray(sources, np.int64), counts), err_msg=f"u {what}")
    np.testing.assert_array_equal(pairs[1], np.concatenate(want + [np.zeros(0, np.int64)]), err_msg=f"v {what}")


def _fixture_graphs(fx, test_set):
    n = fx.n
    p = "ppr_test_" if test_set else "ppr_"
    ppr = _sp_ppr(fx[p + "row"], fx[p + "col"], fx[p + "val"], n)
    adj = _sp_adj(fx["full_edge_index" if test_set else "edge_index"], n)
    return ppr, adj


def _sources(n, rng, extra=()):
    return np.concatenate([np.arange(n), rng.integers(0, n, size=64), np.asarray(extra, np.int64)]).astype(np.int64)


# ------------------------------------------------------------------------------------------------ 1. candidates
@pytest.mark.parametrize("case", LP_CASES)
def test_candidates_match_numpy_on_fixtures(case):
    fx = Fixture(case)
    model, score = _build(fx)
    rng = np.random.default_rng(0)
    n = fx.n
    src = _sources(n, rng)
    splits = (False, True) if case == "lp_all_d64_residual_valtest" else (False,)
    for test_set in splits:
        ppr_np, adj_np = _fixture_graphs(fx, test_set)
        ppr = model._device_graph("ppr", model._data_obj("ppr", test_set))
        adj = model._device_graph("mask", model._data_obj("mask", test_set))
        for mode in ("ppr", "all"):
            for min_ppr in ((0.0, 1e-3) if mode == "ppr" else (0.0,)):
                for exclude in ("adj", None):
                    for self_ in (True, False):
                        counts, pairs = _run_candidates(src, n, ppr if mode == "ppr" else None, min_ppr,
                                                        adj if exclude else None, self_)
                        want = _np_candidates(src, n, ppr_np if mode == "ppr" else None, min_ppr,
                                              adj_np if exclude else None, self_)
                        _check_candidates(src, counts, pairs, want, f"{case} {test_set} {mode} {min_ppr} {exclude} "
                                                                    f"{self_}")
    # the public entry point sees the same candidates: n_candidates == counts
    rec = lpformer_amd.recommend(model, score, torch.from_numpy(src[:32]), k=5)
    want = _np_candidates(src[:32], n, _fixture_graphs(fx, False)[0], 0.0, _fixture_graphs(fx, False)[1], True)
    np.testing.assert_array_equal(rec.n_candidates.cpu().numpy(), [w.size for w in want])


@pytest.fixture(scope="module")
def hub():
    n = 4000
    ei, _ = D.chung_lu_graph(n, 60_000, gamma=2.1, seed=7)
    ei = np.asarray(ei, np.int64)
    ppr = lpformer_amd.calc_ppr(ei, n, 0.15, 1e-4)
    adj = graph.mask_csr(ei, n, symmetric=True)
    assert np.diff(ppr.rowptr).max() > 64       # rows past thr = 64: both classes run in one call
    return n, ppr, adj


@pytest.mark.parametrize("thr", [-1, 0, 64, 1 << 30])
def test_candidates_hub_graph_each_work_class(hub, thr):
    n, ppr, adj = hub
    ppr_np = sp.csr_matrix((ppr.val, ppr.col, ppr.rowptr), shape=(n, n))
    adj_np = sp.csr_matrix((np.ones(adj.nnz), adj.col, adj.rowptr), shape=(n, n))
    rng = np.random.default_rng(1)
    src = _sources(n, rng)
    dppr, dadj = ppr.to_device(DEV), adj.to_device(DEV)
    for mode in ("ppr", "all"):
        for min_ppr in (0.0, 1e-3):
            counts, pairs = _run_candidates(src, n, dppr if mode == "ppr" else None, min_ppr, dadj, True, thr)
            want = _np_candidates(src, n, ppr_np if mode == "ppr" else None, min_ppr, adj_np, True)
            _check_candidates(src, counts, pairs, want, f"thr {thr} {mode} {min_ppr}")
    # two runs: the same bits
    c1, p1 = _run_candidates(src, n, dppr, 0.0, dadj, False, thr)
    c2, p2 = _run_candidates(src, n, dppr, 0.0, dadj, False, thr)
    assert np.array_equal(c1, c2) and np.array_equal(p1, p2)


# ------------------------------------------------------------------------------------------------ 2. top-K
def _tie_scores(rng, size):
    s = (rng.integers(-6, 7, size=size) / 4.0).astype(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan], np.float32)
    m = rng.random(size) < 0.05
    s[m] = rng.choice(special, size=int(m.sum()))
    return s


@pytest.mark.parametrize("k", [1, 7, 100, 1024])
def test_segment_topk_bitwise_against_lexsort(k):
    rng = np.random.default_rng(k)
    lengths = [0, 1, max(k - 1, 0), k, k + 1, 4095, 70_000, 1 << 21, 3, 256, 257, 4096, 4097, 0]
    seg_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    P = int(seg_ptr[-1])
    score = _tie_scores(rng, P)
    cand = rng.integers(0, 1 << 40, size=P).astype(np.int64)
    args = [torch.from_numpy(seg_ptr).to(DEV), torch.from_numpy(score).to(DEV), torch.from_numpy(cand).to(DEV), k]
    ids, out, cnt = segment_topk(*args)
    ids2, out2, cnt2 = segment_topk(*args)
    w_ids, w_out, w_cnt = _np_topk(seg_ptr, score, cand, k)
    np.testing.assert_array_equal(cnt.cpu().numpy(), w_cnt)
    np.testing.assert_array_equal(ids.cpu().numpy(), w_ids)
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), w_out.view(np.uint32))
    assert torch.equal(ids, ids2) and torch.equal(cnt, cnt2)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32))


def test_segment_topk_many_short_and_all_equal():
    rng = np.random.default_rng(11)
    lengths = rng.integers(0, 300, size=5000)
    lengths[:50] = 5000                                  # a few block-class segments among them
    seg_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    P = int(seg_ptr[-1])
    for score in (_tie_scores(rng, P), np.full(P, 0.5, np.float32)):   # all-equal: ties broken by position alone
        cand = np.arange(P, dtype=np.int64)
        ids, out, cnt = segment_topk(torch.from_numpy(seg_ptr).to(DEV), torch.from_numpy(score).to(DEV),
                                     torch.from_numpy(cand).to(DEV), 100)
        w_ids, w_out, w_cnt = _np_topk(seg_ptr, score, cand, 100)
        np.testing.assert_array_equal(ids.cpu().numpy(), w_ids)
        np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), w_out.view(np.uint32))
        np.testing.assert_array_equal(cnt.cpu().numpy(), w_cnt)


# ------------------------------------------------------------------------------------------------ 3. end to end
def _lexsort_topk(model, score, pairs, counts, k, batch_size, test_set):
    lg = E.score_edges(model, score, torch.from_numpy(pairs).to(DEV), batch_size, test_set=test_set,
                       logits=True).cpu().numpy()
    seg_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return _np_topk(seg_ptr, lg, pairs[1], k)


@pytest.mark.parametrize("case,test_set", [("lp_all_d64", False), ("lp_all_d128_weighted", False),
                                           ("lp_all_d64_heads2", False), ("lp_all_d64_residual_valtest", True)])
def test_recommend_end_to_end(case, test_set):
    fx = Fixture(case)
    model, score = _build(fx)
    n = fx.n
    rng = np.random.default_rng(5)
    src = np.concatenate([rng.integers(0, n, size=200), [int(rng.integers(0, n))] * 3]).astype(np.int64)
    ppr_np, adj_np = _fixture_graphs(fx, test_set)
    k, bs = 20, 4096
    for mode in ("ppr", "all"):
        rec = lpformer_amd.recommend(model, score, torch.from_numpy(src), k, candidates=mode, test_set=test_set,
                                     batch_size=bs, logits=True)
        assert rec.ids.shape == (src.size, k) and rec.ids.dtype == torch.int64 and rec.scores.dtype == torch.float32
        want = _np_candidates(src, n, ppr_np if mode == "ppr" else None, 0.0, adj_np, True)
        counts = np.array([w.size for w in want], np.int64)
        np.testing.assert_array_equal(rec.n_candidates.cpu().numpy(), counts)
        pairs = np.stack([np.repeat(src, counts), np.concatenate(want)])
        w_ids, w_out, w_cnt = _lexsort_topk(model, score, pairs, counts, k, bs, test_set)
        ids, out = rec.ids.cpu().numpy(), rec.scores.cpu().numpy()
        np.testing.assert_array_equal(ids, w_ids, err_msg=f"{case} {mode}")
        np.testing.assert_array_equal(out.view(np.uint32), w_out.view(np.uint32), err_msg=f"{case} {mode}")
        np.testing.assert_array_equal(rec.counts.cpu().numpy(), w_cnt)
        # probabilities: sigmoid of the same logits, same ids
        prob = lpformer_amd.recommend(model, score, torch.from_numpy(src), k, candidates=mode, test_set=test_set,
                                      batch_size=bs)
        assert torch.equal(prob.ids, rec.ids)
        live = rec.ids >= 0
        assert torch.equal(prob.scores[live], torch.sigmoid(rec.scores[live]))
        assert bool((prob.scores[~live] == float("-inf")).all())
        if fx.cfg.get("num_heads", 1) == 1 and fx.cfg.get("trans_layers", 1) == 1 and mode == "ppr":
            # a sample of returned pairs against the CPU oracle
            s_ix, c_ix = np.nonzero(ids >= 0)
            pick = rng.choice(s_ix.size, size=min(256, s_ix.size), replace=False)
            batch = np.stack([src[s_ix[pick]], ids[s_ix[pick], c_ix[pick]]])
            p = "ppr_test_" if test_set else "ppr_"
            ei = fx["full_edge_index" if test_set else "edge_index"].astype(np.int64)
            ew = fx["full_edge_weight" if test_set else "edge_weight"]
            ppr_o = O.csr_from_coo(fx[p + "row"].astype(np.int64), fx[p + "col"].astype(np.int64), fx[p + "val"], n)
            ref = O.forward(batch, fx["x"], O.gcn_norm(ei, ew, n), O.symmetric_mask_csr(ei, n), ppr_o, fx.params,
                            fx.cfg)
            err = np.abs(out[s_ix[pick], c_ix[pick]] - ref["logit"]).max()
            assert err <= 1e-4 * max(1.0, float(np.abs(ref["logit"]).max())), (case, err)


# ------------------------------------------------------------------------------------------------ 4. chunks, edges
def test_chunking_explicit_isolated_and_range():
    fx = Fixture("lp_all_d64")
    model, score = _build(fx)
    n = fx.n
    rng = np.random.default_rng(9)
    src = torch.from_numpy(rng.integers(0, n, size=300).astype(np.int64))
    h = model.propagate()
    for mode in ("ppr", "all"):
        big = lpformer_amd.recommend(model, score, src, 50, candidates=mode, h=h, logits=True)
        one = int(big.n_candidates.max())
        small = lpformer_amd.recommend(model, score, src, 50, candidates=mode, h=h, logits=True, max_pairs=one,
                                       batch_size=777)
        # candidates and ranking are pure functions of the logits; score_edges itself moves a pair's logit by a few
        # ulps with the batch the pair lands in (<= 1e-6 measured), so the ids must agree and the scores to that level
        assert torch.equal(big.ids, small.ids) and torch.equal(big.counts, small.counts)
        live = big.ids >= 0
        torch.testing.assert_close(small.scores[live], big.scores[live], rtol=0, atol=4e-6)
        assert torch.equal(small.scores[~live], big.scores[~live])
        tiny = lpformer_amd.recommend(model, score, src[:20], 50, candidates=mode, h=h, logits=True, max_pairs=1)
        assert torch.equal(tiny.ids, big.ids[:20])
        torch.testing.assert_close(tiny.scores[live[:20]], big.scores[:20][live[:20]], rtol=0, atol=4e-6)
        # the same chunking twice: the same bits
        again = lpformer_amd.recommend(model, score, src, 50, candidates=mode, h=h, logits=True, max_pairs=one,
                                       batch_size=777)
        assert torch.equal(again.ids, small.ids) and torch.equal(again.scores.view(torch.int32),
                                                                  small.scores.view(torch.int32))

    # explicit [S, M] candidates with duplicates: score_negatives + lexsort
    S, M, k = 64, 40, 16
    srcs = rng.integers(0, n, size=S).astype(np.int64)
    cand = rng.integers(0, n, size=(S, M)).astype(np.int64)
    cand[:, 5] = cand[:, 2]
    cand[:, 7] = srcs                                     # v = u is kept: explicit candidates are taken as given
    rec = lpformer_amd.recommend(model, score, torch.from_numpy(srcs), k, candidates=torch.from_numpy(cand),
                                 logits=True, batch_size=1000)
    neg = np.stack([np.broadcast_to(srcs[:, None], (S, M)), cand], axis=-1)
    lg = E.score_negatives(model, score, torch.from_numpy(neg), 1000, logits=True).cpu().numpy().reshape(-1)
    w_ids, w_out, w_cnt = _np_topk(np.arange(S + 1, dtype=np.int64) * M, lg, cand.reshape(-1), k)
    np.testing.assert_array_equal(rec.ids.cpu().numpy(), w_ids)
    np.testing.assert_array_equal(rec.scores.cpu().numpy().view(np.uint32), w_out.view(np.uint32))
    assert (rec.n_candidates.cpu().numpy() == M).all()

    # an isolated source (no PPR row entries, no neighbours): count 0, ids -1, scores -inf
    ppr_np, adj_np = _fixture_graphs(fx, False)
    empty = np.flatnonzero(np.diff(ppr_np.indptr) == 0)
    iso = int(empty[0]) if empty.size else None
    if iso is None:      # no empty PPR row in this fixture: a source whose candidates are all excluded
        want = _np_candidates(np.arange(n), n, ppr_np, 0.0, adj_np, True)
        iso = int(np.argmin([w.size for w in want]))
        assert want[iso].size == 0, "the fixture has no source without candidates"
    r = lpformer_amd.recommend(model, score, torch.tensor([iso, iso]), 10)
    assert (r.counts.cpu() == 0).all() and (r.n_candidates.cpu() == 0).all()
    assert (r.ids.cpu() == -1).all() and bool((r.scores.cpu() == float("-inf")).all())

    # ids outside [0, n): IndexError before anything runs
    for bad in ([0, n], [-1], [n + 5, 1]):
        with pytest.raises(IndexError):
            lpformer_amd.recommend(model, score, torch.tensor(bad), 10)
    with pytest.raises(IndexError):
        lpformer_amd.recommend(model, score, torch.tensor([0]), 10, candidates=torch.tensor([[n]]))
    model.train()
    try:
        with pytest.raises(NotImplementedError):
            lpformer_amd.recommend(model, score, torch.tensor([0]), 10)
    finally:
        model.eval()


def test_recommendation_metrics_on_device():
    fx = Fixture("lp_all_d64")
    model, score = _build(fx)
    rng = np.random.default_rng(2)
    src = torch.from_numpy(rng.integers(0, fx.n, size=100).astype(np.int64))
    rec = lpformer_amd.recommend(model, score, src, 50, candidates="all")
    held = torch.stack([src.repeat_interleave(2), rec.ids[:, [0, 40]].cpu().reshape(-1)], 1)
    m = E.recommendation_metrics(rec, src.to(DEV), held.to(DEV), ks=(1, 50))
    assert m["n_sources"] == 100
    assert m["hit@1"] == 1.0 and m["recall@1"] == pytest.approx(0.5) and m["recall@50"] == 1.0
