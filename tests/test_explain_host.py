"""Host checks of lpformer_amd.explain: the torch restatement of ``explain_from_scores`` on hand-built cases and on the
reference fixtures (fed with the oracle's attention scores), ``attention_profile``, ``pairs_of`` and the argument errors.
No device needed."""
import importlib
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import lpformer_amd
from oracle import lpformer_oracle as O
from tests.golden_util import LP_CASES, Fixture

X = importlib.import_module("lpformer_amd.explain")   # (the package attribute of that name is the function)

TOL = 1e-4   # the project's parity bound


def _layout(pairs):
    """pairs: per pair a list of (type 1..3, node, score[, pa, pb]) -> the exported type-major layout."""
    bs = len(pairs)
    tp = torch.zeros(3, bs + 1, dtype=torch.int64)
    node, pa, pb, sc = [], [], [], []
    for t in range(3):
        for p, ent in enumerate(pairs):
            mine = sorted((e for e in ent if e[0] == t + 1), key=lambda e: e[1])
            tp[t, p + 1] = tp[t, p] + len(mine)
            for e in mine:
                node.append(e[1])
                sc.append(e[2])
                pa.append(e[3] if len(e) > 3 else 0.25 * e[1])
                pb.append(e[4] if len(e) > 4 else -0.5 * e[1])
    return (tp, torch.tensor(node, dtype=torch.int32), torch.tensor(pa, dtype=torch.float32),
            torch.tensor(pb, dtype=torch.float32), torch.tensor(sc, dtype=torch.float32))


def _softmax64(scores):
    s = np.asarray(scores, np.float64)
    e = np.exp(s - s.max())
    return e / (e.sum() + 1e-16)


def test_empty_single_and_padding():
    pairs = [[], [(2, 7, 1.5, 0.125, 0.75)], []]
    r = X.explain_from_scores(*_layout(pairs), top=3)
    assert r.nodes.tolist() == [[-1, -1, -1], [7, -1, -1], [-1, -1, -1]]
    assert r.types.tolist() == [[0, 0, 0], [2, 0, 0], [0, 0, 0]]
    assert r.weights.tolist() == [[0, 0, 0], [1.0, 0, 0], [0, 0, 0]]
    assert r.ppr_a[1].tolist() == [0.125, 0, 0] and r.ppr_b[1].tolist() == [0.75, 0, 0]
    assert r.mass.tolist() == [[0, 0, 0], [0, 1.0, 0], [0, 0, 0]]
    assert r.entropy.tolist() == [0, 0, 0]
    assert r.nodes.dtype == torch.int64 and r.types.dtype == torch.int8 and r.all is None


def test_no_pairs_at_all():
    z = torch.zeros(3, 1, dtype=torch.int64)
    e = torch.empty(0)
    r = X.explain_from_scores(z, e.int(), e, e, e, top=4, want_all=True)
    assert r.nodes.shape == (0, 4) and r.mass.shape == (0, 3) and r.entropy.shape == (0,)
    assert r.all[0].tolist() == [0] and r.all[1].numel() == 0


@pytest.mark.parametrize("n", [2, 3, 4, 9])     # fewer than, exactly and more than top = 3
def test_fewer_exactly_more_than_top(n):
    rng = np.random.default_rng(n)
    sc = rng.permutation(n) * 0.5 - 1.0           # distinct
    ent = [(1 + i % 3, 10 + i, float(sc[i])) for i in range(n)]
    r = X.explain_from_scores(*_layout([ent]), top=3)
    alpha = _softmax64(sc)
    order = np.argsort(-alpha)[:3]
    k = min(n, 3)
    assert r.nodes[0, :k].tolist() == [10 + int(i) for i in order[:k]]
    assert r.types[0, :k].tolist() == [1 + int(i) % 3 for i in order[:k]]
    np.testing.assert_allclose(r.weights[0, :k].numpy(), alpha[order[:k]], atol=1e-6)
    assert r.nodes[0, k:].tolist() == [-1] * (3 - k) and r.weights[0, k:].tolist() == [0.0] * (3 - k)
    assert r.ppr_a[0, :k].tolist() == [0.25 * (10 + int(i)) for i in order[:k]]
    assert r.ppr_b[0, :k].tolist() == [-0.5 * (10 + int(i)) for i in order[:k]]
    for t in range(3):
        assert abs(float(r.mass[0, t]) - alpha[[i for i in range(n) if i % 3 == t]].sum()) <= 1e-6
    assert abs(float(r.mass[0].sum()) - 1.0) <= 1e-6
    assert abs(float(r.entropy[0]) + (alpha * np.log(alpha)).sum()) <= 1e-6


def test_missing_type_and_joint_softmax():
    # one softmax across the types jointly: a high-scoring >1-hop node takes mass from the common neighbours
    pairs = [[(1, 3, 0.0), (1, 5, 0.0), (3, 4, math.log(2.0))]]
    r = X.explain_from_scores(*_layout(pairs), top=8)
    np.testing.assert_allclose(r.mass[0].numpy(), [0.5, 0.0, 0.5], atol=1e-6)
    assert r.nodes[0, :3].tolist() == [4, 3, 5] and r.types[0, :3].tolist() == [3, 1, 1]
    np.testing.assert_allclose(r.weights[0, :3].numpy(), [0.5, 0.25, 0.25], atol=1e-6)


def test_ties_go_to_the_smaller_node_id_across_types():
    pairs = [[(3, 2, 1.0), (1, 9, 1.0), (2, 4, 1.0), (1, 6, 1.0), (2, 1, 0.5)]]
    r = X.explain_from_scores(*_layout(pairs), top=5)
    assert r.nodes[0].tolist() == [2, 4, 6, 9, 1]
    assert r.types[0].tolist() == [3, 2, 1, 1, 2]
    w = r.weights[0]
    assert float(w[0]) == float(w[1]) == float(w[2]) == float(w[3]) > float(w[4])


def test_nan_alpha_ranks_last_and_zero_alpha_adds_no_entropy():
    # a score far below the maximum underflows to alpha = 0: its entropy term is 0, not NaN
    r = X.explain_from_scores(*_layout([[(1, 1, 0.0), (1, 2, -200.0)]]), top=2)
    assert r.weights[0].tolist() == [1.0, 0.0] and float(r.entropy[0]) == 0.0
    # a NaN score makes every alpha of ITS pair NaN (as the softmax does); order then falls back to the node id
    r = X.explain_from_scores(*_layout([[(1, 8, float("nan")), (2, 3, 0.0)], [(1, 1, 0.0)]]), top=2)
    assert r.nodes[0].tolist() == [3, 8] and bool(torch.isnan(r.weights[0]).all())
    assert r.weights[1].tolist() == [1.0, 0.0]


@pytest.mark.parametrize("n", [1, 2, 7, 64, 1000])
def test_uniform_segment_has_entropy_ln_n(n):
    ent = [(1 + i % 2, i, -3.0) for i in range(n)]
    r = X.explain_from_scores(*_layout([ent]), top=4)
    assert abs(float(r.entropy[0]) - math.log(n)) <= 1e-5 * max(1.0, math.log(n))
    assert abs(float(r.mass[0].sum()) - 1.0) <= 1e-6
    assert r.nodes[0, :min(n, 4)].tolist() == list(range(min(n, 4)))


def test_all_list_round_trips_to_the_input_order():
    rng = np.random.default_rng(5)
    pairs = []
    for p in range(6):
        ids = rng.permutation(40)[:rng.integers(0, 12)]
        pairs.append([(int(rng.integers(1, 4)), int(v), float(rng.integers(-6, 6)) * 0.5) for v in ids])
    tp, node, pa, pb, sc = _layout(pairs)
    r = X.explain_from_scores(tp, node, pa, pb, sc, top=2, want_all=True)
    ptr, a_node, a_type, a_w = r.all
    assert ptr.tolist() == np.concatenate([[0], np.cumsum([len(e) for e in pairs])]).tolist()
    tbase = [0, int(tp[0, -1]), int(tp[0, -1] + tp[1, -1])]
    for p, ent in enumerate(pairs):
        lo, hi = int(ptr[p]), int(ptr[p + 1])
        want_nodes, want_types, src = [], [], []
        for t in range(3):
            s0, s1 = int(tp[t, p]), int(tp[t, p + 1])
            src += list(range(tbase[t] + s0, tbase[t] + s1))
            want_types += [t + 1] * (s1 - s0)
        want_nodes = node[src].tolist()
        assert a_node[lo:hi].tolist() == want_nodes and a_type[lo:hi].tolist() == want_types
        if ent:
            np.testing.assert_allclose(a_w[lo:hi].numpy(), _softmax64(sc[src].numpy()), atol=1e-6)
            # ... and the top list is the head of the same weights
            best = max(range(lo, hi), key=lambda j: (float(a_w[j]), -int(a_node[j])))
            assert int(r.nodes[p, 0]) == int(a_node[best]) and float(r.weights[p, 0]) == float(a_w[best])


def oracle_scores(fx):
    """The oracle's attention scores of a fixture's recorded call in the exported layout: ``link_attention``'s score
    (oracle/lpformer_oracle.py, layers.py:206-218) from ``calc_pairwise``'s parts.  Returns (type_ptr, node, pa, pb,
    score, alpha_ref per entry)."""
    adj_norm = O.gcn_norm(fx.edge_index, fx.edge_weight, fx.n)
    mask = O.symmetric_mask_csr(fx.edge_index, fx.n)
    r, c, v = fx.ppr_coo
    res = O.forward(fx["batch"], fx["x"], adj_norm, mask, O.csr_from_coo(r, c, v, fx.n), fx.params, fx.cfg,
                    want_parts=True)
    return scores_from_parts(fx["batch"].astype(np.int64), res, fx.params) + (fx["att_weights"][1],)


def scores_from_parts(batch, res, P, prefix="model.att_layers.0"):
    ix, x_node = res["ix"], res["x_node"]
    pair, node = ix[0], ix[1]
    k = O.linear(np.concatenate([x_node[node], res["pes"]], axis=1), P[f"{prefix}.att.lin_r.weight"],
                 P[f"{prefix}.att.lin_r.bias"])
    w_l, b_l = P[f"{prefix}.att.lin_l.weight"], P[f"{prefix}.att.lin_l.bias"]
    q = O.linear(x_node[batch[0]], w_l, b_l) + O.linear(x_node[batch[1]], w_l, b_l)
    s = k * q[pair]
    s = np.where(s > 0, s, np.float32(0.2) * s).astype(np.float32)
    score = (s * P[f"{prefix}.att.att"].reshape(-1)).sum(axis=1, dtype=np.float32)
    bs = batch.shape[1]
    tags = [t for t in ("cn", "onehop", "non1hop") if t in res["sel"]]
    tp = np.zeros((3, bs + 1), np.int64)
    pa, pb = [], []
    for t, tag in enumerate(tags):
        tp[t, 1:] = np.cumsum(np.bincount(res["sel"][tag][0][0], minlength=bs))
        pa.append(res["sel"][tag][1])
        pb.append(res["sel"][tag][2])
    return (torch.from_numpy(tp), torch.from_numpy(node.astype(np.int32)), torch.from_numpy(np.concatenate(pa)),
            torch.from_numpy(np.concatenate(pb)), torch.from_numpy(score))


FIXTURES = [c for c in LP_CASES if "att_weights" in Fixture(c) and Fixture(c).cfg["dim"] in (64, 128)]


@pytest.mark.parametrize("case", FIXTURES)
def test_restatement_reproduces_the_reference_alpha(case):
    fx = Fixture(case)
    tp, node, pa, pb, score, alpha_ref = oracle_scores(fx)
    assert score.numel() == alpha_ref.size > 0
    r = X.explain_from_scores(tp, node, pa, pb, score, top=32, want_all=True)
    ptr, a_node, a_type, a_w = r.all
    # the reference's order is type-major (att_weights row 0 = pair position): map both to (pair, type, node)
    bs = tp.shape[1] - 1
    ref = {}
    base = 0
    for t in range(3):
        for p in range(bs):
            for j in range(int(tp[t, p]), int(tp[t, p + 1])):
                assert int(fx["att_weights"][0][base + j]) == p
                ref[(p, int(node[base + j]))] = (t + 1, float(alpha_ref[base + j]))
        base += int(tp[t, bs])
    assert len(ref) == score.numel()
    worst = 0.0
    for p in range(bs):
        for j in range(int(ptr[p]), int(ptr[p + 1])):
            t, a = ref[(p, int(a_node[j]))]
            assert t == int(a_type[j])
            worst = max(worst, abs(a - float(a_w[j])))
        k = min(32, int(ptr[p + 1] - ptr[p]))
        for j in range(k):
            t, a = ref[(p, int(r.nodes[p, j]))]
            assert t == int(r.types[p, j]) and abs(a - float(r.weights[p, j])) <= TOL
    assert worst <= TOL, worst


def _expl(mass, ent, w0, empty):
    P = len(ent)
    nodes = torch.where(torch.tensor(empty), -1, 5).view(P, 1)
    z = torch.zeros(P, 1)
    return X.Explanation(nodes, torch.tensor(w0).view(P, 1), z.to(torch.int8), z, z, torch.zeros(P, 3, dtype=torch.int32),
                         torch.tensor(mass), torch.tensor(ent), None, None)


def test_attention_profile():
    e = _expl([[1.0, 0, 0], [0.5, 0.5, 0], [0, 0, 0], [0.2, 0.2, 0.6]], [0.0, 0.7, 0.0, 1.0], [1.0, 0.5, 0.0, 0.6],
              [False, False, True, False])
    one = X.attention_profile(e)
    assert len(one) == 1 and one[0]["bin"] is None and one[0]["count"] == 4
    assert one[0]["mass_cn"] == pytest.approx(0.425) and one[0]["mass_1hop"] == pytest.approx(0.175)
    assert one[0]["mass_non1hop"] == pytest.approx(0.15) and one[0]["entropy"] == pytest.approx(0.425)
    assert one[0]["top1"] == pytest.approx(0.525) and one[0]["empty"] == pytest.approx(0.25)
    rows = X.attention_profile(e, values=torch.tensor([0, 1, 2, 3]))       # CN_BINS: [0,1) [1,3) [3,10) [10,1e6)
    assert [r["bin"] for r in rows] == list(lpformer_amd.evaluate.CN_BINS)
    assert [r["count"] for r in rows] == [1, 2, 1, 0]
    assert rows[1]["mass_cn"] == pytest.approx(0.25) and rows[1]["empty"] == pytest.approx(0.5)
    assert rows[2]["mass_non1hop"] == pytest.approx(0.6) and math.isnan(rows[3]["entropy"])
    rows = X.attention_profile(e, values=[0.5, 0.5, 2.0, 2.0], bins=((0.0, 1.0), (1.0, 2.0)))   # half-open
    assert [r["count"] for r in rows] == [2, 0]
    with pytest.raises(ValueError):
        X.attention_profile(e, values=[1, 2])
    with pytest.raises(ValueError):
        X.attention_profile(e, bins=((0, 1),))


def test_pairs_of():
    rec = lpformer_amd.Recommendations(ids=torch.tensor([[4, 2, -1], [-1, -1, -1], [9, 8, 7]]),
                                       scores=torch.zeros(3, 3), counts=torch.tensor([2, 0, 3]),
                                       n_candidates=torch.tensor([2, 0, 11]))
    edges, row, col = X.pairs_of(torch.tensor([10, 11, 12]), rec)
    assert edges.tolist() == [[10, 10, 12, 12, 12], [4, 2, 9, 8, 7]]
    assert row.tolist() == [0, 0, 2, 2, 2] and col.tolist() == [0, 1, 0, 1, 2]
    assert edges.dtype == torch.int64
    with pytest.raises(ValueError):
        X.pairs_of(torch.tensor([1, 2]), rec)


def test_argument_errors():
    lay = _layout([[(1, 1, 0.0)]])
    for bad in (0, 33, -1, 2.5):
        with pytest.raises(ValueError):
            X.explain_from_scores(*lay, top=bad)
    with pytest.raises(ValueError):
        X.explain_from_scores(torch.tensor([[0, 2], [0, 0], [0, 0]]), *lay[1:], top=2)   # pointers past the entries
    with pytest.raises(TypeError):
        X.explain_from_scores(lay[0], lay[1].float(), *lay[2:], top=2)

    class Stub(SimpleNamespace):     # explain() checks its arguments before it touches the model's kernels
        def _check_supported(self):
            raise AssertionError("reached the model")
    stub = Stub(num_nodes=10, training=False)
    for bad in (0, 33):
        with pytest.raises(ValueError):
            X.explain(stub, torch.tensor([[1], [2]]), top=bad)
    with pytest.raises(ValueError):
        X.explain(stub, torch.tensor([[1], [2]]), weights="some")
    with pytest.raises(ValueError):
        X.explain(stub, torch.tensor([[1], [2]]), batch_size=0)
    for bad in ([[1], [10]], [[-1], [2]]):
        with pytest.raises(IndexError):
            X.explain(stub, torch.tensor(bad))
    assert {"explain", "explain_from_scores", "pairs_of", "attention_profile", "Explanation"} <= set(lpformer_amd.__all__)


def test_abi_carries_the_entry_point():
    from lpformer_amd import _lib
    assert _lib.ABI_VERSION >= 15 and "lpf_pair_explain_f32" in _lib.HIP_PROTOTYPES
    assert hasattr(_lib.hip(), "lpf_pair_explain_f32")
