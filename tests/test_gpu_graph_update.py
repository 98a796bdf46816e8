"""Graph edits on the MI355X: lpf_ppr_affected_rows, lpf_ppr_push_f64_sources and lpf_ppr_splice_csr against numpy and
the full producers, bit by bit; ``update_graph`` on a live model against a fresh model of the edited graph."""
import numpy as np
import pytest
import torch

import lpformer_amd
from lpformer_amd import _lib, graph
from lpformer_amd import data as D
from lpformer_amd import graph_update as U
from lpformer_amd.ppr import calc_ppr, calc_ppr_gpu
from tests.golden_util import GOLDEN_DIR, Fixture
from tests.test_graph_update_host import ALPHA, EPS, N, assert_same_csr, edit_cases, edited_edge_list, random_pairs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-4  # the parity tests' bound on logits (tests/test_gpu_parity.py)


@pytest.fixture(scope="module")
def base():
    ei, _ = D.chung_lu_graph(N, 12000, seed=1)
    return ei, calc_ppr(ei, N, ALPHA, EPS)


def _host_triple(t, n):
    return graph.CSR(t[0].cpu().numpy(), t[1].cpu().numpy(), t[2].cpu().numpy(), n)


# ------------------------------------------------------------------------------------------------ kernels
def _np_affected(ppr, mask):
    rows = np.repeat(np.arange(ppr.n), np.diff(ppr.rowptr))
    return np.unique(rows[mask[ppr.col]]).astype(np.int32)


def _check_affected(ppr, mask, what):
    want = _np_affected(ppr, mask)
    d = ppr.to_device(DEV)
    for mode in (0, 1, -1):        # global-memory bitmap, LDS bitmap, the library's choice
        flag, lst, count = U.affected_rows_device(d, mask, bitmap_mode=mode)
        k = int(count.item())
        assert k == want.size, (what, mode)
        got = lst[:k].cpu().numpy()
        np.testing.assert_array_equal(got, want, err_msg=f"{what} mode {mode}")
        want_flag = np.zeros(ppr.n, np.int32)
        want_flag[want] = 1
        np.testing.assert_array_equal(flag.cpu().numpy(), want_flag, err_msg=f"{what} mode {mode}")


@pytest.mark.parametrize("case", ["ppr_push_small", "ppr_push_powerlaw"])
def test_affected_rows_on_golden_graphs(case):
    z = np.load(f"{GOLDEN_DIR}/{case}.npz")
    n = int(z["n"])
    ppr = calc_ppr(z["edge_index"], n, ALPHA, float(z["eps_list"][-1]))
    rng = np.random.default_rng(0)
    for k in (1, 5, n // 4):
        mask = np.zeros(n, bool)
        mask[rng.choice(n, k, replace=False)] = True
        _check_affected(ppr, mask, f"{case} {k} keys")
    _check_affected(ppr, np.zeros(n, bool), f"{case} no key")          # empty key set -> empty list
    _check_affected(ppr, np.ones(n, bool), f"{case} all keys")         # all keys -> all rows


def test_affected_rows_on_synthetic_graph_with_long_rows():
    n = 20000
    ei, _ = D.chung_lu_graph(n, 90000, gamma=2.3, seed=5)
    ppr = calc_ppr(ei, n, ALPHA, 1e-4)                                  # rows longer than one 256-entry step of a wavefront
    assert np.diff(ppr.rowptr).max() > 256
    rng = np.random.default_rng(1)
    for k in (1, 40, 2000):
        mask = np.zeros(n, bool)
        mask[rng.choice(n, k, replace=False)] = True
        _check_affected(ppr, mask, f"synthetic {k} keys")
    mask = np.zeros(n, bool)
    mask[[n - 1, 31, 32]] = True                                        # word boundaries of the bitmap
    _check_affected(ppr, mask, "synthetic boundary keys")
    with pytest.raises(_lib.LpfError):                                  # the LDS form is refused where it cannot fit
        big = graph.CSR(np.zeros(600001, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), 600000)
        U.affected_rows_device(big.to_device(DEV), np.zeros(600000, bool), bitmap_mode=1)


def test_push_sources_equals_full_push_rows_and_host_twin(base):
    ei, full = base
    g = graph.csr_from_coo(ei[0], ei[1], None, N)
    gpu_full = calc_ppr_gpu(ei, N, ALPHA, EPS, device=DEV)
    assert_same_csr(gpu_full, full)
    src = np.unique(np.random.default_rng(1).integers(0, N, 300)).astype(np.int32)
    rowptr, col = torch.from_numpy(g.rowptr).to(DEV), torch.from_numpy(g.col).to(DEV)
    h_rp, h_c, h_v = U._push_sources_host(g.rowptr, g.col, N, src, ALPHA, EPS)
    for waves, cap in ((0, 0), (4, 0), (64, 1000)):                     # (a tiny pool forces the exact-size rerun)
        s = torch.from_numpy(src).to(DEV)
        row_off, row_len, pc, pv, nnz = U.push_sources_device(rowptr, col, N, s, ALPHA, EPS, n_waves=waves,
                                                              pool_capacity=cap)
        assert nnz == int(h_rp[-1])
        ro, rl, pc, pv = row_off.cpu().numpy(), row_len.cpu().numpy(), pc.cpu().numpy(), pv.cpu().numpy()
        for i, v in enumerate(src):
            order = np.argsort(pc[ro[i]:ro[i] + rl[i]])
            a0, a1 = full.rowptr[v], full.rowptr[v + 1]
            np.testing.assert_array_equal(pc[ro[i]:ro[i] + rl[i]][order], full.col[a0:a1])
            np.testing.assert_array_equal(pv[ro[i]:ro[i] + rl[i]][order].view(np.uint32),
                                          full.val[a0:a1].view(np.uint32))
            np.testing.assert_array_equal(h_c[h_rp[i]:h_rp[i + 1]], full.col[a0:a1])
            np.testing.assert_array_equal(h_v[h_rp[i]:h_rp[i + 1]].view(np.uint32), full.val[a0:a1].view(np.uint32))


@pytest.mark.parametrize("case", ["add", "remove", "mixed", "noop", "noop_plus_real", "hub", "isolated",
                                  "twin_reversed"])
def test_update_ppr_device_equals_full_producer_and_host_path(base, case):
    ei, old = base
    add, remove = edit_cases(ei)[case]
    ei2 = edited_edge_list(ei, N, add, remove)
    want = calc_ppr_gpu(ei2, N, ALPHA, EPS, device=DEV)
    host, hs = lpformer_amd.update_ppr(old, ei, add=add, remove=remove, alpha=ALPHA, eps=EPS, full_above=1.0)
    # host container in -> host container out
    got, stats = lpformer_amd.update_ppr(old, ei, add=add, remove=remove, alpha=ALPHA, eps=EPS, device=DEV,
                                         full_above=1.0, verify=4)
    assert stats["path"] == "incremental" and stats["n_affected"] == hs["n_affected"] and \
        stats["n_keys"] == hs["n_keys"]
    assert_same_csr(got, want, case)
    assert_same_csr(got, host, case)
    # device triple in -> device triple out, indistinguishable from calc_ppr_gpu(..., to_host=False)
    old_d = calc_ppr_gpu(ei, N, ALPHA, EPS, device=DEV, to_host=False)
    want_d = calc_ppr_gpu(ei2, N, ALPHA, EPS, device=DEV, to_host=False)
    for mode in (0, 1):
        got_d, stats = lpformer_amd.update_ppr(old_d, ei, add=add, remove=remove, alpha=ALPHA, eps=EPS, device=DEV,
                                               full_above=1.0, bitmap_mode=mode)
        assert stats["path"] == "incremental"
        for a, b in zip(got_d, want_d):
            assert a.is_cuda and a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(got_d[0], want_d[0]) and torch.equal(got_d[1], want_d[1])
        assert torch.equal(got_d[2].view(torch.int32), want_d[2].view(torch.int32))
    full, stats = lpformer_amd.update_ppr(old_d, ei, add=add, remove=remove, alpha=ALPHA, eps=EPS, device=DEV,
                                          full_above=-1.0)
    assert stats["path"] == "full"
    assert_same_csr(_host_triple(full, N), want, case)


# ------------------------------------------------------------------------------------------------ model level
CFG_KEYS = ("thresh_cn", "thresh_1hop", "thresh_non1hop", "dim", "trans_layers", "num_heads", "att_drop", "dropout",
            "gnn_drop", "feat_drop", "gcn_cache", "gnn_layers", "residual", "layer_norm", "relu")


def _model(cfg, data, state=None, pred_layers=2, seed=0):
    torch.manual_seed(seed)
    model = lpformer_amd.LinkTransformer(cfg, data, device=DEV).to(DEV)
    score = lpformer_amd.mlp_score(model.out_dim, model.out_dim, 1, pred_layers).to(DEV)
    if state is not None:
        model.load_state_dict(state[0], strict=True)
        score.load_state_dict(state[1], strict=True)
    return model.eval(), score.eval()


def _setup(kind):
    """(cfg, n, x, edge list, weights, eps, state dicts or None, pred_layers)."""
    if kind == "chung_lu_d128":
        c = D.CONFIGS["tiny"]
        n = c["n"]
        ei, w = D.chung_lu_graph(n, c["edges"], seed=1, max_weight=c["max_weight"])
        x = np.random.default_rng(0).standard_normal((n, c["f_in"])).astype(np.float32)
        return dict(D.train_args_for(c), dim=128), n, x, ei, w, c["eps"], None, 2
    fx = Fixture(kind)
    m_sd, s_sd = fx.state_dicts()
    state = ({k: torch.from_numpy(v) for k, v in m_sd.items()}, {k: torch.from_numpy(v) for k, v in s_sd.items()})
    return ({k: fx.cfg[k] for k in CFG_KEYS}, fx.n, fx["x"], fx["edge_index"].astype(np.int64), fx["edge_weight"],
            fx.cfg["eps"], state, fx.cfg["pred_layers"])


def _edit_for(ei, n, seed=0):
    rng = np.random.default_rng(seed)
    add = rng.integers(0, n, size=(2, 12))
    add = add[:, add[0] != add[1]]
    remove = ei[:, rng.choice(ei.shape[1], 3, replace=False)]
    return add, remove


def _edited_weights(ei, w, ei2, n, new_weight=1.0):
    old = dict(zip((ei[0] * n + ei[1]).tolist(), np.asarray(w, np.float32).tolist()))
    return np.array([old.get(k, new_weight) for k in (ei2[0] * n + ei2[1]).tolist()], np.float32)


@pytest.mark.parametrize("kind", ["lp_all_d64", "lp_1hop_d64_dense", "chung_lu_d128"])     # mask modes "all", "1-hop"; D = 128
def test_update_graph_equals_fresh_model_of_edited_graph(kind):
    """Selected index sets bit-exact; logits of score_pairs and forward within the parity tests' TOL (they are printed:
    the two models run the same kernels on equal graph arrays, so the difference is expected to be 0)."""
    cfg, n, x, ei, w, eps, state, pred = _setup(kind)
    w = np.ones(ei.shape[1], np.float32) if w is None else w
    data = D.build_data(ei, x, n, edge_weight=w, eps=eps)
    model, score = _model(cfg, data, state, pred)
    state = state or (model.state_dict(), score.state_dict())
    batch0 = torch.from_numpy(D.sample_pairs(ei, n, 512, seed=3)).to(DEV)
    before = model.score_pairs(batch0, model.propagate(), score, logits=True).clone()    # (graph state exists before the edit)
    add, remove = _edit_for(ei, n)
    stats = lpformer_amd.update_graph(model, add=add, remove=remove, alpha=ALPHA, eps=eps, full_above=1.0, verify=4)
    assert stats["ppr"]["path"] == "incremental" and model._graph_epoch == 1
    for k in ("upload_s", "walk_index_s", "gcn_norm_s", "encoder_s", "data_s"):
        assert stats[k] >= 0.0
    ei2 = edited_edge_list(ei, n, add, remove)
    fresh_data = D.build_data(ei2, x, n, edge_weight=_edited_weights(ei, w, ei2, n), eps=eps, ppr_device=DEV)
    for k in ("adj_t", "adj_mask", "ppr"):
        assert_same_csr(model.data[k], fresh_data[k], k)
    fresh, fscore = _model(cfg, fresh_data, state, pred)
    batch = torch.from_numpy(D.sample_pairs(ei2, n, 512, seed=4)).to(DEV)
    sel_a, sel_b = model.compute_node_mask(batch), fresh.compute_node_mask(batch)
    for ia, ib in zip(sel_a, sel_b):
        if ia is None or ib is None:
            assert ia is None and ib is None
            continue
        assert len(ia) == len(ib)
        for ta, tb in zip(ia, ib):
            assert torch.equal(ta, tb) if isinstance(ta, torch.Tensor) else ta == tb
    la = model.score_pairs(batch, model.propagate(), score, logits=True)
    lb = fresh.score_pairs(batch, fresh.propagate(), fscore, logits=True)
    assert model.check_selection() and fresh.check_selection()
    fa, fb = score.logits(model(batch)), fscore.logits(fresh(batch))
    d1, d2 = float((la - lb).abs().max()), float((fa - fb).abs().max())
    print(f"{kind}: max |logit difference| score_pairs {d1:.3e}, forward {d2:.3e}")
    assert d1 <= TOL and d2 <= TOL
    # the edit changed something the old graph's scores saw
    after0 = model.score_pairs(batch0, model.propagate(), score, logits=True)
    assert not torch.equal(before, after0)


def test_recommend_accept_top1_then_recommend_again():
    cfg, n, x, ei, w, eps, state, pred = _setup("lp_all_d64")
    data = D.build_data(ei, x, n, edge_weight=w, eps=eps)
    model, score = _model(cfg, data, state, pred)
    sources = torch.arange(0, n, 7)
    rec = lpformer_amd.recommend(model, score, sources, k=5)
    have = (rec.counts > 0).cpu()
    src, top1 = sources[have].numpy(), rec.ids[:, 0].cpu()[have].numpy()
    assert src.size > 10
    add = np.stack([src, top1])
    lpformer_amd.update_graph(model, add=add, alpha=ALPHA, eps=eps, full_above=1.0)
    rec2 = lpformer_amd.recommend(model, score, sources, k=5)
    ids2 = rec2.ids.cpu()[have].numpy()
    assert not np.any(ids2 == top1[:, None])            # an accepted link is an edge now: no candidate any more
    ei2 = edited_edge_list(ei, n, add)
    fresh, fscore = _model(cfg, D.build_data(ei2, x, n, edge_weight=_edited_weights(ei, w, ei2, n), eps=eps), state, pred)
    rec3 = lpformer_amd.recommend(fresh, fscore, sources, k=5)
    assert torch.equal(rec2.ids, rec3.ids) and torch.equal(rec2.counts, rec3.counts)
    assert torch.equal(rec2.n_candidates, rec3.n_candidates)
    fin = torch.isfinite(rec3.scores)
    assert torch.equal(fin, torch.isfinite(rec2.scores))
    assert float((rec2.scores[fin] - rec3.scores[fin]).abs().max()) <= TOL


@pytest.mark.parametrize("cls", ["PlannedScorer", "GraphedScorer"])
def test_scorer_recorded_before_update_raises(cls):
    """A recorded scorer holds pointers into the old graph's indexes and the old encoder output: after update_graph its
    next call raises (it never returns the old graph's scores); a new scorer scores the new graph."""
    cfg, n, x, ei, w, eps, state, pred = _setup("chung_lu_d128")
    data = D.build_data(ei, x, n, edge_weight=w, eps=eps)
    model, score = _model(cfg, data, None, pred)
    batch = torch.from_numpy(D.sample_pairs(ei, n, 512, seed=3)).to(DEV)
    scorer = getattr(lpformer_amd, cls)(model, score, model.propagate(), batch, logits=True)
    old = scorer(batch).clone()
    add, remove = _edit_for(ei, n)
    lpformer_amd.update_graph(model, add=add, remove=remove, alpha=ALPHA, eps=eps)
    with pytest.raises(_lib.LpfError, match="update_graph"):
        scorer(batch)
    with pytest.raises(_lib.LpfError, match="update_graph"):
        scorer(batch, validate=False)
    h = model.propagate()
    new = getattr(lpformer_amd, cls)(model, score, h, batch, logits=True)(batch)
    torch.cuda.synchronize()
    new = new.clone()
    assert float((new - model.score_pairs(batch, h, score, logits=True)).abs().max()) <= TOL
    assert not torch.equal(new, old)
