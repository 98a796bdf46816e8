"""similar_nodes (lpf_similar_topm_f32, csrc/similar.hip) on the MI355X: bit for bit against the numpy restatement on
integer data, within the standard fp32 dot-product bound of fp64 on real data, and the two recommend modes on it."""
import numpy as np
import pytest
import torch

import lpformer_amd
from lpformer_amd import evaluate as E
from lpformer_amd import graph, similar
from tests import similar_cases as SC
from tests.golden_util import Fixture

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SPECS = SC.exact_specs()


def _device_csr(exc, n):
    return None if exc is None else graph.CSR(exc[0], exc[1].astype(np.int32), None, n).to_device(DEV)


def _run(case, n_ranges, Q=None, T=None):
    """The kernel on a case: rows with ld > D and NaN in the padding columns."""
    D = case["D"]
    Q = torch.from_numpy(SC.padded(case["Q"])).to(DEV)[:, :D] if Q is None else Q
    T = torch.from_numpy(SC.padded(case["T"], extra=8)).to(DEV)[:, :D] if T is None else T

    def dev(a, dtype):
        return None if a is None else torch.from_numpy(np.asarray(a, dtype)).to(DEV)
    got = similar.topm(Q, T, case["m"], q_scale=dev(case["q_scale"], np.float32), t_scale=dev(case["t_scale"], np.float32),
                       src_ids=dev(case["src_ids"], np.int64), exclude=_device_csr(case["exclude"], case["n"]),
                       exclude_self=case["exclude_self"], n_ranges=n_ranges)
    return got.ids.cpu().numpy(), got.scores.cpu().numpy(), got.counts.cpu().numpy()


# ------------------------------------------------------------------------------------------------------ 1. exact cases
@pytest.mark.parametrize("spec", SPECS, ids=lambda s: SC.make_case(**s)["id"])
def test_exact_cases_equal_the_reference_at_every_n_ranges(spec):
    case = SC.make_case(**spec)
    want = similar.similar_reference(case["Q"], case["T"], case["m"], q_scale=case["q_scale"], t_scale=case["t_scale"],
                                     src_ids=case["src_ids"], exclude=case["exclude"],
                                     exclude_self=case["exclude_self"])
    for n_ranges in SC.N_RANGES:
        ids, scores, counts = _run(case, n_ranges)
        np.testing.assert_array_equal(counts, want[2], err_msg=f"counts, n_ranges {n_ranges}")
        np.testing.assert_array_equal(ids, want[0], err_msg=f"ids, n_ranges {n_ranges}")
        assert SC.same_bits(scores, want[1]), f"scores, n_ranges {n_ranges}"
        # padding is never returned, and nothing but padding lies past counts
        live = np.arange(case["m"])[None, :] < counts[:, None]
        assert (ids[live] >= 0).all() and (ids[~live] == -1).all() and np.isneginf(scores[~live]).all()


@pytest.mark.parametrize("kind", ["random", "increasing", "decreasing"])
def test_merge_of_more_keys_than_its_buffer_holds(kind):
    """40 ranges x 256 keys per source, 10,240 against a buffer of 4,096: the merge kernel sorts, raises its threshold
    and goes on -- with "increasing" every later key beats the threshold, with "decreasing" none does."""
    case = SC.make_case(n=20000, S=3, D=3, m=256, exclusion="csr", kind=kind)
    want = similar.similar_reference(case["Q"], case["T"], case["m"], src_ids=case["src_ids"], exclude=case["exclude"])
    for n_ranges in (40, 313, -1):
        ids, scores, counts = _run(case, n_ranges)
        np.testing.assert_array_equal(counts, want[2])
        np.testing.assert_array_equal(ids, want[0], err_msg=f"ids, n_ranges {n_ranges}")
        assert SC.same_bits(scores, want[1])


def test_hub_source_returns_fewer_than_m_and_specials_rank_as_documented():
    case = SC.make_case(n=1000, S=17, D=36, m=256, exclusion="hub", metric="cosine")
    ids, scores, counts = _run(case, -1)
    assert counts[0] <= 3 and counts[1] == 256             # the hub source: 3 eligible nodes (2 if it is one of them)
    case = SC.make_case(n=1000, S=17, D=3, m=256, exclusion="self", metric="dot", kind="special")
    ids, scores, counts = _run(case, 7)
    for s in np.flatnonzero(counts > 0):
        sc = scores[s, :counts[s]]
        nan = np.isnan(sc)
        assert not nan[:-1][~nan[1:]].any()                # NaN only at the end of a row
        assert (sc[~nan][:-1] >= sc[~nan][1:]).all()       # the rest descending, -inf above NaN
        zero = ids[s, :counts[s]][sc == 0]
        assert (np.diff(zero) > 0).all()                   # -0.0 ties +0.0: one run, ascending ids
        assert not np.signbit(sc[sc == 0]).any()


# ------------------------------------------------------------------------------------------------- 2. real-valued cases
@pytest.mark.parametrize("D", [36, 128, 257])
def test_normal_tables_within_the_dot_product_bound(D):
    n, S, m = 3000, 37, 64
    rng = np.random.default_rng(D)
    T = rng.standard_normal((n, D)).astype(np.float32)
    src = rng.integers(0, n, size=S).astype(np.int64)
    src[3] = src[2]
    exc = SC.random_csr(n, rng)
    Td = torch.from_numpy(T).to(DEV)
    got = lpformer_amd.similar_nodes(None, torch.from_numpy(src), m, table=Td, metric="dot",
                                     exclude=graph.CSR(exc[0], exc[1], None, n))
    score64, B = SC.dot_bound(T[src], T, D)
    ok = SC.eligible_mask(n, src, exc, True)
    a, c = SC.check_real(got.ids.cpu().numpy(), got.scores.cpu().numpy(), got.counts.cpu().numpy(), score64, B, ok, m)
    print(f"D {D}: largest error / B = {a:.3f}, largest slack used / allowed = {c:.3f}, max B = {B.max():.2e}")


@pytest.mark.parametrize("case,metric", [("lp_all_d64", "cosine"), ("lp_all_d128_weighted", "dot")])
def test_fixture_embedding_with_adjacency_exclusion(case, metric):
    fx = Fixture(case)
    model, _ = SC.build_model(fx, DEV)
    n, m = fx.n, 64
    rng = np.random.default_rng(1)
    src = np.concatenate([rng.integers(0, n, size=36), [0]]).astype(np.int64)
    h = model.propagate()
    got = lpformer_amd.similar_nodes(model, torch.from_numpy(src), m, metric=metric, h=h)
    again = lpformer_amd.similar_nodes(model, torch.from_numpy(src), m, metric=metric)       # propagates itself
    assert torch.equal(got.ids, again.ids) and torch.equal(got.scores.view(torch.int32), again.scores.view(torch.int32))
    hn = h.float().cpu().numpy()
    qs = ts = None
    if metric == "cosine":
        ts = similar._inv_norm(h.float()).cpu().numpy()
        qs = similar._inv_norm(h.float()[torch.from_numpy(src).to(DEV)]).cpu().numpy()
    score64, B = SC.dot_bound(hn[src], hn, hn.shape[1], qs, ts)
    adj = model._device_graph("mask", model._data_obj("mask", False)).to_host()
    ok = SC.eligible_mask(n, src, (adj.rowptr, adj.col), True)
    a, c = SC.check_real(got.ids.cpu().numpy(), got.scores.cpu().numpy(), got.counts.cpu().numpy(), score64, B, ok, m)
    print(f"{case} {metric}: largest error / B = {a:.3f}, largest slack used / allowed = {c:.3f}")
    # the raw features as the table: the same checks
    x = fx["x"].astype(np.float32)
    gx = lpformer_amd.similar_nodes(model, torch.from_numpy(src), m, table="x", metric="dot", exclude=None,
                                    exclude_self=False)
    score64, B = SC.dot_bound(x[src], x, x.shape[1])
    SC.check_real(gx.ids.cpu().numpy(), gx.scores.cpu().numpy(), gx.counts.cpu().numpy(), score64, B,
                  np.ones((src.size, n), bool), m)


# ------------------------------------------------------------------------------------------------------- 3. recommend
def _candidates_of(rec):
    """Per source the set of a mode's candidates, from a result whose k holds them all."""
    assert int(rec.n_candidates.max()) <= rec.ids.shape[1]
    return [np.sort(row[row >= 0]) for row in rec.ids.cpu().numpy()]


def _ranked(model, score, src, cands, k, bs, h):
    counts = np.array([c.size for c in cands], np.int64)
    pairs = np.stack([np.repeat(src, counts), np.concatenate(cands)])
    lg = E.score_edges(model, score, torch.from_numpy(pairs).to(DEV), bs, h=h, logits=True).cpu().numpy()
    return SC.np_topk(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), lg, pairs[1], k), counts


def test_recommend_similar_ranks_the_similar_nodes():
    fx = Fixture("lp_all_d64")
    model, score = SC.build_model(fx, DEV)
    rng = np.random.default_rng(5)
    src = np.concatenate([rng.integers(0, fx.n, size=60), [7, 7]]).astype(np.int64)
    h = model.propagate()
    k, bs = 20, 4096
    for table, metric, n_sim in (("embedding", "cosine", 32), ("x", "dot", 50)):
        rec = lpformer_amd.recommend(model, score, torch.from_numpy(src), k, candidates="similar", n_similar=n_sim,
                                     similar_table=table, similar_metric=metric, h=h, batch_size=bs, logits=True)
        sim = lpformer_amd.similar_nodes(model, torch.from_numpy(src), n_sim, table=table, metric=metric, h=h)
        ids = sim.ids.cpu().numpy()
        cands = [row[row >= 0] for row in ids]                  # similarity order, padding dropped
        (w_ids, w_out, w_cnt), counts = _ranked(model, score, src, cands, k, bs, h)
        np.testing.assert_array_equal(rec.n_candidates.cpu().numpy(), counts)
        np.testing.assert_array_equal(rec.n_candidates.cpu().numpy(), sim.counts.cpu().numpy())
        np.testing.assert_array_equal(rec.ids.cpu().numpy(), w_ids)
        assert SC.same_bits(rec.scores.cpu().numpy(), w_out)
        np.testing.assert_array_equal(rec.counts.cpu().numpy(), w_cnt)


def test_recommend_ppr_plus_similar_is_the_sorted_union_whatever_the_chunking():
    """The candidates and the ranking are pure functions of the logits; ``score_edges`` itself moves a pair's logit by a
    few ulps with the batch the pair lands in (recommend's docstring: at most 9e-7 on the fixtures), so across
    ``max_pairs`` the ids, counts and n_candidates must be identical and the scores agree to 4e-6, the bound
    tests/test_gpu_recommend.py holds the existing modes to; at one chunking two calls give the same bits."""
    fx = Fixture("lp_all_d64")
    model, score = SC.build_model(fx, DEV)
    rng = np.random.default_rng(6)
    src = np.concatenate([rng.integers(0, fx.n, size=40), [3, 3]]).astype(np.int64)
    st = torch.from_numpy(src)
    h = model.propagate()
    k, bs, n_sim = 1024, 4096, 48
    kw = dict(h=h, batch_size=bs, logits=True)
    ppr = _candidates_of(lpformer_amd.recommend(model, score, st, k, candidates="ppr", **kw))
    sim = _candidates_of(lpformer_amd.recommend(model, score, st, k, candidates="similar", n_similar=n_sim, **kw))
    union = [np.union1d(a, b) for a, b in zip(ppr, sim)]
    assert any(u.size < a.size + b.size for u, a, b in zip(union, ppr, sim))      # some ids are in both
    assert any(u.size > a.size for u, a in zip(union, ppr))                       # and some similar ids are new
    k = 30
    big = lpformer_amd.recommend(model, score, st, k, candidates="ppr+similar", n_similar=n_sim, **kw)
    (w_ids, w_out, w_cnt), counts = _ranked(model, score, src, union, k, bs, h)
    np.testing.assert_array_equal(big.n_candidates.cpu().numpy(), counts)
    np.testing.assert_array_equal(big.ids.cpu().numpy(), w_ids)
    assert SC.same_bits(big.scores.cpu().numpy(), w_out)
    np.testing.assert_array_equal(big.counts.cpu().numpy(), w_cnt)
    live = big.ids >= 0
    for max_pairs in (1, int(counts.max())):
        small = lpformer_amd.recommend(model, score, st, k, candidates="ppr+similar", n_similar=n_sim,
                                       max_pairs=max_pairs, **kw)
        assert torch.equal(small.ids, big.ids) and torch.equal(small.counts, big.counts)
        assert torch.equal(small.n_candidates, big.n_candidates)
        print(f"max_pairs {max_pairs}: max |score difference| = "
              f"{float((small.scores[live] - big.scores[live]).abs().max()):.2e}")
        torch.testing.assert_close(small.scores[live], big.scores[live], rtol=0, atol=4e-6)
        assert torch.equal(small.scores[~live], big.scores[~live])
        again = lpformer_amd.recommend(model, score, st, k, candidates="ppr+similar", n_similar=n_sim,
                                       max_pairs=max_pairs, **kw)
        assert torch.equal(again.ids, small.ids)
        assert torch.equal(again.scores.view(torch.int32), small.scores.view(torch.int32))


def test_existing_modes_are_untouched_by_the_new_keywords():
    fx = Fixture("lp_all_d64")
    model, score = SC.build_model(fx, DEV)
    rng = np.random.default_rng(8)
    st = torch.from_numpy(rng.integers(0, fx.n, size=50).astype(np.int64))
    h = model.propagate()
    from lpformer_amd.recommend import _exclusion, generate_candidates, segment_topk
    from lpformer_amd.sources import model_graphs
    dev, adj, ppr = model_graphs(model, False, "test")
    for mode in ("ppr", "all", "2hop"):
        a = lpformer_amd.recommend(model, score, st, 25, candidates=mode, h=h, logits=True)
        b = lpformer_amd.recommend(model, score, st, 25, candidates=mode, h=h, logits=True, n_similar=3,
                                   similar_table="x", similar_metric="dot")
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                               y.view(torch.int32) if y.dtype == torch.float32 else y), mode
        if mode == "2hop":
            continue
        # the same three steps by hand, as before this feature: candidates, score_edges, segmented top-K
        src = st.to(DEV)
        counts, fill = generate_candidates(fx.n, src, ppr if mode == "ppr" else None, 0.0,
                                           _exclusion(model, "adj", adj, dev), True)
        pairs = fill(0, src.numel(), int(counts.sum()))
        lg = E.score_edges(model, score, pairs, 32768, h=h, logits=True)
        seg = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), torch.cumsum(counts, 0)])
        ids, out, cnt = segment_topk(seg, lg, pairs[1], 25)
        assert torch.equal(ids, a.ids) and torch.equal(cnt, a.counts) and torch.equal(counts, a.n_candidates)
        assert torch.equal(out.view(torch.int32), a.scores.view(torch.int32))


# ----------------------------------------------------------------------------------------------------- 4. determinism
def test_two_runs_give_the_same_bits():
    rng = np.random.default_rng(12)
    n, S, D = 3001, 33, 128
    T = torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)).to(DEV)
    nodes = torch.from_numpy(rng.integers(0, n, size=S))
    exc = graph.CSR(*SC.random_csr(n, rng), None, n).to_device(DEV)
    runs = [lpformer_amd.similar_nodes(None, nodes, 100, table=T, exclude=exc, n_ranges=r) for r in (-1, -1, 3)]
    for other in runs[1:]:
        assert torch.equal(runs[0].ids, other.ids) and torch.equal(runs[0].counts, other.counts)
        assert torch.equal(runs[0].scores.view(torch.int32), other.scores.view(torch.int32))
    free = lpformer_amd.similar_nodes(None, queries=T[:5].cpu(), m=4, table=T, metric="dot", exclude=None)
    assert free.ids[:, 0].tolist() == [0, 1, 2, 3, 4]          # a row's best match by inner product is itself here
