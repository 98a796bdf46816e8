"""lpformer_amd.explain on the device: lpf_pair_explain_f32 against its torch restatement on synthetic input, ``explain``
against the reference fixtures and against the CPU oracle, and the properties of the public call."""
import importlib

import numpy as np
import pytest
import torch

import lpformer_amd
from lpformer_amd import data as D
from oracle import lpformer_oracle as O
from tests.golden_util import LP_CASES, Fixture
from tests.test_explain_host import oracle_scores
from tests.test_gpu_parity import _build

X = importlib.import_module("lpformer_amd.explain")   # (the package attribute of that name is the function)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4   # the project's parity bound
FIXTURES = [c for c in LP_CASES if Fixture(c).cfg["dim"] in (64, 128)]   # one layer, one head; modes "all" and "1-hop"


# ------------------------------------------------------------------------------------------ 1. kernel vs restatement
def _synthetic(top, seed):
    """Pairs whose union has 0, 1, top-1, top, top+1, 63, 64, 65, ~1,000 and ~5,000 entries, spread over the three types
    in several ways (one type alone, two, all three); scores are multiples of 0.5 within +-20 (many equal)."""
    rng = np.random.default_rng(seed)
    lengths = [0, 1, top - 1, top, top + 1, 63, 64, 65, 257, 1000, 1024, 1025, 1031, 5003]
    splits = []
    for n in lengths:
        a, b = sorted(rng.integers(0, n + 1, 2).tolist())
        splits += [(n, 0, 0), (0, n, 0), (0, 0, n), (a, b - a, n - b), (a, 0, n - a), (0, n - b, b)]
    splits = [splits[i] for i in rng.permutation(len(splits))]
    bs = len(splits)
    tp = np.zeros((3, bs + 1), np.int64)
    per_type = [[], [], []]
    for p, cnt in enumerate(splits):
        ids = rng.permutation(200_000)[:sum(cnt)]           # a node occurs once per pair
        spread = rng.choice([1, 3, 40])                      # few distinct scores -> long runs of ties
        lo = 0
        for t in range(3):
            mine = np.sort(ids[lo:lo + cnt[t]])
            lo += cnt[t]
            tp[t, p + 1] = tp[t, p] + cnt[t]
            sc = rng.integers(-spread, spread + 1, cnt[t]) * 0.5
            per_type[t].append((mine, sc))
    node = np.concatenate([m for t in range(3) for m, _ in per_type[t]]).astype(np.int32)
    score = np.concatenate([s for t in range(3) for _, s in per_type[t]]).astype(np.float32)
    pa = rng.random(node.size, dtype=np.float32)
    pb = rng.random(node.size, dtype=np.float32)
    return tuple(torch.from_numpy(a) for a in (tp, node, pa, pb, score))


@pytest.mark.parametrize("top", [1, 8, 32])
def test_kernel_matches_the_restatement(top):
    cpu = _synthetic(top, seed=top)
    want = X.explain_from_scores(*cpu, top=top, want_all=True)
    got = X.explain_from_scores(*(t.to(DEV) for t in cpu), top=top, want_all=True)
    torch.cuda.synchronize()
    for name in ("nodes", "types", "ppr_a", "ppr_b"):
        assert torch.equal(getattr(got, name).cpu(), getattr(want, name)), name
    for g, w, name in zip(got.all[:3], want.all[:3], ("all_ptr", "all_node", "all_type")):
        assert g.dtype == w.dtype and torch.equal(g.cpu(), w), name
    dw = float((got.weights.cpu() - want.weights).abs().max())
    da = float((got.all[3].cpu() - want.all[3]).abs().max())
    dm = float((got.mass.cpu() - want.mass).abs().max())
    de = float((got.entropy.cpu() - want.entropy).abs().max())
    print(f"top={top}: |dw| {dw:.3g} |dall| {da:.3g} |dmass| {dm:.3g} |dentropy| {de:.3g}")
    assert dw <= 1e-6 and da <= 1e-6 and dm <= 1e-6
    # entropy H <= ln(5003) = 8.5 nats.  d(-a ln a) = -(ln a + 1) da, so alphas that differ by a relative r between two
    # exp implementations move H by at most (H + 1) r: r <= 4 ulp = 4.8e-7 (exp and the denominator, <= 2 ulp each) gives
    # 4.6e-6, plus half an ulp of the fp32 result (4.8e-7)
    assert de <= 1e-5
    # the top list without the full list is the same launch with the list skipped
    lean = X.explain_from_scores(*(t.to(DEV) for t in cpu), top=top)
    assert lean.all is None
    for name in ("nodes", "weights", "types", "ppr_a", "ppr_b", "mass", "entropy"):
        assert torch.equal(getattr(lean, name), getattr(got, name)), name


# ------------------------------------------------------------------------------------------ 2./3. against references
def _check(expl, ref, tol=TOL):
    """The four per-pair checks.  ref: per pair a dict node -> (type, alpha, pa, pb) of the reference."""
    nodes, w, ty = expl.nodes.cpu().numpy(), expl.weights.cpu().numpy(), expl.types.cpu().numpy()
    pa, pb = expl.ppr_a.cpu().numpy(), expl.ppr_b.cpu().numpy()
    top = nodes.shape[1]
    assert nodes.shape[0] == len(ref)
    worst = 0.0
    for p, sel in enumerate(ref):
        k = min(top, len(sel))
        assert (nodes[p, k:] == -1).all() and (w[p, k:] == 0).all() and (ty[p, k:] == 0).all()
        assert len(set(nodes[p, :k].tolist())) == k
        for j in range(k):
            t, a, ra, rb = sel[int(nodes[p, j])]          # KeyError: a node outside the pair's selected set
            assert t == ty[p, j]
            assert np.float32(ra).view(np.uint32) == pa[p, j].view(np.uint32)
            assert np.float32(rb).view(np.uint32) == pb[p, j].view(np.uint32)
            worst = max(worst, abs(float(w[p, j]) - a))
            if j:
                assert w[p, j] < w[p, j - 1] or (w[p, j] == w[p, j - 1] and nodes[p, j] > nodes[p, j - 1])
        if k < len(sel):
            shown = set(nodes[p, :k].tolist())
            rest = max(a for v, (_, a, _, _) in sel.items() if v not in shown)
            assert rest <= float(w[p, k - 1]) + 2 * tol
    assert worst <= tol, worst
    return worst


def _ref_from_sel(bs, sel_list, alpha):
    """sel_list: [(type, ix [2, n], pa, pb)] in the order of ``alpha`` (type-major)."""
    ref = [dict() for _ in range(bs)]
    base = 0
    for t, ix, pa, pb in sel_list:
        for j in range(ix.shape[1]):
            ref[int(ix[0, j])][int(ix[1, j])] = (t, float(alpha[base + j]), pa[j], pb[j])
        base += ix.shape[1]
    assert base == len(alpha)
    return ref


def _mass_entropy(ref):
    mass = np.zeros((len(ref), 3))
    ent = np.zeros(len(ref))
    for p, sel in enumerate(ref):
        for t, a, _, _ in sel.values():
            mass[p, t - 1] += a
            ent[p] -= a * np.log(a) if a > 0 else 0.0
    return mass, ent


@pytest.mark.parametrize("case", FIXTURES)
def test_explain_vs_reference_fixture(case):
    fx = Fixture(case)
    assert fx.cfg["trans_layers"] == 1 and fx.cfg["num_heads"] == 1
    model, _ = _build(fx)
    batch = torch.from_numpy(fx["batch"])
    bs = batch.shape[1]
    tags = {"cn": 1, "onehop": 2, "non1hop": 3}
    sel_list = [(tags[t], fx[f"sel_{t}_ix"], fx[f"sel_{t}_pa"], fx[f"sel_{t}_pb"]) for t in fx.sel_tags()]
    np.testing.assert_array_equal(fx["att_weights"][0], np.concatenate([s[1][0] for s in sel_list]))
    ref = _ref_from_sel(bs, sel_list, fx["att_weights"][1])
    expl = lpformer_amd.explain(model, batch, top=8, test_set=fx.test_set)
    assert expl.scores is None and expl.all is None
    worst = _check(expl, ref)
    counts = np.zeros((bs, 3), np.int32)
    for t, ix, _, _ in sel_list:
        counts[:, t - 1] = np.bincount(ix[0], minlength=bs)
    np.testing.assert_array_equal(expl.counts.cpu().numpy(), counts)
    mass, ent = _mass_entropy(ref)
    assert np.abs(expl.mass.cpu().numpy() - mass).max() <= TOL
    # Entropy against the fp64 entropy of the reference alphas.  Bound: 8 x the largest deviation the CPU fp32
    # restatement (fed with the oracle's scores of the same call) shows against that value, floor 1e-6 -- the margin
    # covers differing exp / log implementations and summation order.
    # Observed on the fixtures: restatement 5.3e-7 .. 1.5e-6 (bounds 4.2e-6 .. 1.2e-5), kernel 7.0e-7 .. 2.1e-6;
    # per fixture the kernel is at 0.7 .. 1.6 x the restatement's deviation.
    rest = X.explain_from_scores(*oracle_scores(fx)[:5], top=8)
    dev_rest = float(np.abs(rest.entropy.numpy().astype(np.float64) - ent).max())
    dev_kern = float(np.abs(expl.entropy.cpu().numpy().astype(np.float64) - ent).max())
    print(f"{case}: weights {worst:.3g}; entropy restatement {dev_rest:.3g} kernel {dev_kern:.3g}")
    assert dev_kern <= max(8 * dev_rest, 1e-6)


def _random_model(seed, n, edges, gamma, dim, th, eps, weighted):
    rng = np.random.default_rng(100 + seed)
    ei, w = D.chung_lu_graph(n, edges, gamma=gamma, seed=seed, max_weight=6 if weighted else 0)
    x = rng.standard_normal((n, 40)).astype(np.float32)
    ppr = lpformer_amd.calc_ppr(ei, n, 0.15, eps)
    d = D.build_data(ei, x, n, edge_weight=w, ppr=ppr)
    cfg = D.train_args_for(dict(thresholds=th, dim=dim, gnn_layers=2, residual=False))
    torch.manual_seed(seed)
    model = lpformer_amd.LinkTransformer(cfg, d, device=DEV).to(DEV).eval()
    score = lpformer_amd.mlp_score(2 * dim, 2 * dim, 1, 2).to(DEV).eval()
    with torch.no_grad():
        for p in list(model.parameters()) + list(score.parameters()):
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    P = {f"model.{k}": v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    P.update({f"score.{k}": v.detach().cpu().numpy() for k, v in score.state_dict().items()})
    batch = D.sample_pairs(ei, n, 700, seed=seed + 50)
    hub = int(np.argmax(np.bincount(ei[0], minlength=n)))
    batch[:, :6] = np.array([[0, 5, 7, 7, hub, hub], [0, 5, 9, 9, (hub + 1) % n, hub]])  # a == b, duplicates, hub pairs
    return model, score, P, cfg, ei, w, x, ppr, batch


def _oracle_ref(batch, x_node, sel, P):
    _, parts = O.calc_pairwise(batch, x_node, sel, P, want_parts=True)
    tags = {"cn": 1, "onehop": 2, "non1hop": 3}
    sel_list = [(tags[t], sel[t][0], sel[t][1], sel[t][2]) for t in ("cn", "onehop", "non1hop") if t in sel]
    np.testing.assert_array_equal(parts["ix"], np.concatenate([s[1] for s in sel_list], axis=1))
    return _ref_from_sel(batch.shape[1], sel_list, parts["alpha"])


# the graph sizes of tests/test_gpu_random_sweep.py: mode "all" with hubs, mode "cn"
@pytest.mark.parametrize("case", [(1, 900, 9000, 2.05, 64, (0.0, 1e-4, 1e-2), 1e-4, True),
                                  (5, 1200, 15000, 2.05, 128, (0.0, 1e-5, 1e-3), 5e-5, True),
                                  (8, 700, 9000, 2.3, 64, (0.0, 1.0, 1.0), 1e-4, False)],
                         ids=["all_d64", "all_d128", "cn_d64"])
def test_explain_vs_oracle(case):
    seed, n, edges, gamma, dim, th, eps, weighted = case
    model, _, P, cfg, ei, w, x, ppr, batch = _random_model(*case)
    assert model.mask == ("cn" if th[1] == 1.0 else "all")
    pc = (ppr.rowptr, ppr.col.astype(np.int64), ppr.val)
    mask_full = O.symmetric_mask_csr(ei, n)
    x_node = O.propagate(x, O.gcn_norm(ei, w, n), P, dict(cfg, pred_layers=2))
    sel = O.select_nodes(batch, mask_full, pc, th, n=n)
    ref = _oracle_ref(batch, x_node, sel, P)
    assert sum(len(r) for r in ref) > 100 and max(len(r) for r in ref) > 8
    expl = lpformer_amd.explain(model, torch.from_numpy(batch), top=8)
    worst = _check(expl, ref)
    mass, ent = _mass_entropy(ref)
    assert np.abs(expl.mass.cpu().numpy() - mass).max() <= TOL
    counts = np.array([[sum(1 for v in r.values() if v[0] == t) for t in (1, 2, 3)] for r in ref], np.int32)
    np.testing.assert_array_equal(expl.counts.cpu().numpy(), counts)
    print(f"seed {seed}: weights {worst:.3g}, entropy {np.abs(expl.entropy.cpu().numpy() - ent).max():.3g}")
    if model.mask != "all":
        return
    # an adj_mask override (the training loop's masked typing adjacency): the batch's positive edges removed
    und = ei[:, ei[0] < ei[1]]
    rng = np.random.default_rng(seed)
    pos = und[:, rng.integers(0, und.shape[1], 300)]
    mb = np.concatenate([pos, pos[::-1, :40], batch[:, :100]], axis=1).astype(np.int64)
    gone = set((pos[0] * n + pos[1]).tolist()) | set((pos[1] * n + pos[0]).tolist())
    keep = np.array([k not in gone for k in (ei[0] * n + ei[1]).tolist()])
    kr, kc = torch.from_numpy(ei[0][keep]).to(DEV), torch.from_numpy(ei[1][keep]).to(DEV)
    masked_t = torch.sparse_coo_tensor(torch.stack([kr, kc]), torch.ones(kr.numel(), dtype=torch.int32, device=DEV),
                                       (n, n)).coalesce()
    sel_m = O.select_nodes(mb, O.symmetric_mask_csr(ei[:, keep], n), pc, th, n=n, adj_unmasked=mask_full)
    ref_m = _oracle_ref(mb, x_node, sel_m, P)
    plain = O.select_nodes(mb, mask_full, pc, th, n=n)
    assert plain["onehop"][0].shape != sel_m["onehop"][0].shape, "the removed edges must matter"
    for ov in (masked_t, lpformer_amd.RemovedEdges(torch.from_numpy(pos))):
        _check(lpformer_amd.explain(model, torch.from_numpy(mb), top=8, adj_mask=ov), ref_m)


# ------------------------------------------------------------------------------------------ 4. properties
def test_properties_of_the_public_call():
    model, score, P, cfg, ei, w, x, ppr, batch = _random_model(1, 900, 9000, 2.05, 64, (0.0, 1e-4, 1e-2), 1e-4, True)
    tb = torch.from_numpy(batch).to(DEV)
    h = model.propagate()
    one = lpformer_amd.explain(model, tb, top=8, score_func=score, weights="all", h=h)
    # independent of batch_size (also given as [P, 2])
    for bsz in (64, 333):
        cut = lpformer_amd.explain(model, tb.t(), top=8, score_func=score, weights="all", batch_size=bsz)
        for name in ("nodes", "types", "counts"):
            assert torch.equal(getattr(cut, name), getattr(one, name)), name
        for name in ("weights", "mass", "entropy", "ppr_a", "ppr_b"):
            assert float((getattr(cut, name) - getattr(one, name)).abs().max()) <= 1e-6, name
        for a, b in zip(cut.all[:3], one.all[:3]):
            assert torch.equal(a, b)
        assert float((cut.all[3] - one.all[3]).abs().max()) <= 1e-6
        assert float((cut.scores - one.scores).abs().max()) <= 1e-5 * max(1.0, float(one.scores.abs().max()))
    # weights="all" is return_weights with node ids: same (pair, node) set, same alpha
    ptr, a_node, a_type, a_w = one.all
    _, attw = model.calc_pairwise(tb, h, return_weights=True)
    infos = model.compute_node_mask(tb)
    ix = torch.cat([i[0] for i in infos if i is not None], dim=1)
    assert torch.equal(attw[0].long(), ix[0]) and ptr[-1].item() == ix.shape[1] == a_node.numel()
    a_pair = torch.repeat_interleave(torch.arange(batch.shape[1], device=DEV), ptr[1:] - ptr[:-1])
    ka, kb = a_pair * 900 + a_node, ix[0] * 900 + ix[1]
    oa, ob = torch.sort(ka), torch.sort(kb)
    assert torch.equal(oa.values, ob.values) and oa.values.unique().numel() == ka.numel()
    assert float((a_w[oa.indices] - attw[1][ob.indices]).abs().max()) <= 1e-6
    assert torch.equal(one.counts.sum(dim=1).long(), ptr[1:] - ptr[:-1])
    # scores are the score_pairs logits
    lg = model.score_pairs(tb, h, score, logits=True)
    assert model.check_selection()
    assert torch.equal(one.scores, lg)
    # top-only and full runs agree; the profile is one row per bin
    lean = lpformer_amd.explain(model, tb, top=3)
    assert torch.equal(lean.nodes, one.nodes[:, :3]) and torch.equal(lean.weights, one.weights[:, :3])
    rows = lpformer_amd.attention_profile(one, values=one.counts[:, 0])
    assert len(rows) == 4 and sum(r["count"] for r in rows) == batch.shape[1]
    assert abs(sum(rows[1][k] for k in ("mass_cn", "mass_1hop", "mass_non1hop")) + rows[1]["empty"] - 1.0) <= 1e-5 \
        or rows[1]["count"] == 0
    # recommend -> pairs_of -> explain: one row per recommended pair
    src = torch.tensor([3, 17, int(batch[0, 4]), 250], device=DEV)
    rec = lpformer_amd.recommend(model, score, src, k=5, h=h)
    edges, row, col = lpformer_amd.pairs_of(src, rec)
    ex = lpformer_amd.explain(model, edges, top=4, score_func=score, h=h)
    assert ex.nodes.shape == (int(rec.counts.sum()), 4) and edges.shape[1] == int(rec.counts.sum())
    assert torch.equal(edges[0], src[row]) and torch.equal(edges[1], rec.ids[row, col])
    assert float((torch.sigmoid(ex.scores) - rec.scores[row, col]).abs().max()) <= 1e-5
    # no pairs
    none = lpformer_amd.explain(model, torch.empty(2, 0, dtype=torch.int64), top=4, score_func=score, weights="all")
    assert none.nodes.shape == (0, 4) and none.scores.shape == (0,) and none.all[0].tolist() == [0]
    # argument and mode errors
    with pytest.raises(IndexError):
        lpformer_amd.explain(model, torch.tensor([[0], [900]]))
    with pytest.raises(ValueError):
        lpformer_amd.explain(model, tb, top=33)
    model.train()
    with pytest.raises(NotImplementedError):
        lpformer_amd.explain(model, tb)
    model.eval()


@pytest.mark.parametrize("heads,layers", [(2, 1), (1, 2)])
def test_multi_head_and_two_layer_models_raise(heads, layers):
    rng = np.random.default_rng(3)
    n = 300
    ei, w = D.chung_lu_graph(n, 1500, seed=3)
    d = D.build_data(ei, rng.standard_normal((n, 16)).astype(np.float32), n, ppr=lpformer_amd.calc_ppr(ei, n, 0.15, 1e-3))
    cfg = dict(D.train_args_for(dict(thresholds=(0.0, 1e-3, 1e-2), dim=32, gnn_layers=1, residual=False)),
               num_heads=heads, trans_layers=layers)
    model = lpformer_amd.LinkTransformer(cfg, d, device=DEV).to(DEV).eval()
    with pytest.raises(NotImplementedError):
        lpformer_amd.explain(model, torch.tensor([[1, 2], [3, 4]]))
