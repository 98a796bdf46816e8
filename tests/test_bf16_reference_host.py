"""The fp64 restatement of the folded scoring path (tests/bf16_reference.py) on the CPU: with every rounding switch off it
is the oracle on the reference-recorded fixtures; its bf16 rounding agrees bit for bit with torch's cast, the host
images (fold.to_bf16_bits) and the kernels' NaN quieting; its flip flags sit where they should."""
import numpy as np
import pytest
import torch

from lpformer_amd import fold
from oracle import lpformer_oracle as O
from tests import bf16_reference as R
from tests.golden_util import LP_CASES, Fixture
from tests.test_oracle_golden import FLOAT_TOL

TAGS = ("cn", "onehop", "non1hop")


def _mode(cfg):
    if cfg["thresh_non1hop"] == 1 and cfg["thresh_1hop"] == 1:
        return "cn", 1, 1
    if cfg["thresh_non1hop"] == 1:
        return "1-hop", 2, 3
    return "all", 3, 4


def _folded_case(fx):
    """Everything the restatement takes, from the fixture's own parameters: the fold tables (lpformer_amd/fold.py),
    the fp32 node table Z and the queries q, the selection records and the tail's tables (the score fold of
    LinkTransformer._score_fold, fp64 stored as fp32)."""
    P = fx.params
    d = fx.cfg["dim"]
    _, n_types, n_counts = _mode(fx.cfg)
    sd = {k[len("model."):]: torch.from_numpy(np.asarray(v)) for k, v in P.items() if k.startswith("model.")}
    w = fold.fold_attention(sd, d, n_types)
    w["pe_tab"], w["pe_stat"] = fold.pe_tables(sd, d, n_types)
    x = fx["x_node"].astype(np.float64)
    batch = fx["batch"].astype(np.int64)
    z = (x @ w["w_rx"].astype(np.float64).T + w["b_r"]).astype(np.float32)
    wl, bl = P["model.att_layers.0.att.lin_l.weight"].astype(np.float64), P["model.att_layers.0.att.lin_l.bias"]
    q = (x[batch[0]] @ wl.T + bl + x[batch[1]] @ wl.T + bl).astype(np.float32)
    sel = [(fx[f"sel_{t}_ix"], fx[f"sel_{t}_pa"], fx[f"sel_{t}_pb"]) if f"sel_{t}_ix" in fx else None for t in TAGS]
    f64 = lambda k: P[k].astype(np.float64)  # noqa: E731
    we1, be1 = f64("model.elementwise_lin.linears.1.weight"), f64("model.elementwise_lin.linears.1.bias")
    wp1, bp1 = f64("model.pairwise_lin.linears.1.weight"), f64("model.pairwise_lin.linears.1.bias")
    ws0, bs0 = f64("score.lins.0.weight"), f64("score.lins.0.bias")
    a = np.concatenate([ws0[:, :d] @ we1, ws0[:, d:] @ wp1], axis=1)
    c = bs0 + ws0[:, :d] @ be1 + ws0[:, d:] @ bp1
    tabs = {"w_p0": P["model.pairwise_lin.linears.0.weight"], "b_p0": P["model.pairwise_lin.linears.0.bias"],
            "lnB_g": P["model.pairwise_lin.norm.weight"], "lnB_b": P["model.pairwise_lin.norm.bias"],
            "A": a.astype(np.float32), "c": c.astype(np.float32), "w_dot": P["score.lins.1.weight"].reshape(-1),
            "b_dot": P["score.lins.1.bias"]}
    r_e = R.elementwise_hidden(x, batch, P["model.elementwise_lin.linears.0.weight"],
                               P["model.elementwise_lin.linears.0.bias"], P["model.elementwise_lin.norm.weight"],
                               P["model.elementwise_lin.norm.bias"])
    return w, z, q, sel, tabs, r_e, n_counts, (wp1, bp1)


@pytest.mark.parametrize("case", LP_CASES)
def test_restatement_matches_reference_fixtures(case):
    """Rounding switches off: attention rows before and after post_att_norm, pairwise features and logits of the
    folded restatement against the reference's recorded outputs and the oracle, to the oracle's own FLOAT_TOL."""
    fx = Fixture(case)
    P = fx.params
    w, z, q, sel, tabs, r_e, n_counts, (wp1, bp1) = _folded_case(fx)
    bs = fx["batch"].shape[1]
    att = R.attention_ref(sel, z, q, w, P["model.att_layers.0.att.bias"],
                          P["model.att_layers.0.post_att_norm.weight"], P["model.att_layers.0.post_att_norm.bias"], bs)
    tail = R.tail_ref(att["post"], R.count_features(att["counts"], n_counts), r_e, tabs)
    pairwise = tail["r_p"] @ wp1.T + bp1
    got = {"att_pre_ln": att["pre"], "att_post_ln": att["post"], "pairwise_feats": pairwise, "logit": tail["logit"]}
    for key, v in got.items():
        err = np.abs(v - fx[key]).max()
        assert err <= FLOAT_TOL, f"{case}:{key} max abs err {err}"
    assert att["n_flag"] == tail["n_flag"] == 0 and not att["d_post"].any() and not tail["d_logit"].any()
    # ... and the oracle's own restatement agrees on the same case
    adj_norm = O.gcn_norm(fx.edge_index, fx.edge_weight, fx.n)
    r, cc, v = fx.ppr_coo
    ref = O.forward(fx["batch"], fx["x"], adj_norm, O.symmetric_mask_csr(fx.edge_index, fx.n),
                    O.csr_from_coo(r, cc, v, fx.n), P, fx.cfg, x_node=fx["x_node"])
    assert np.abs(tail["logit"] - ref["logit"]).max() <= FLOAT_TOL


@pytest.mark.parametrize("case", LP_CASES)
def test_encoder_restatement_matches_reference_fixtures(case):
    """The encoder restatement (aggregate-then-transform order, as the fused layer kernel computes it) without
    rounding: the reference's recorded node embeddings."""
    fx = Fixture(case)
    P, cfg = fx.params, fx.cfg
    rp, col, val = O.gcn_norm(fx.edge_index, fx.edge_weight, fx.n)
    pre = "model.node_encoder.gnn_encoder"
    layers = [(P[f"{pre}.convs.{i}.lin.weight"], P[f"{pre}.convs.{i}.bias"],
               P.get(f"{pre}.lns.{i}.weight") if cfg["layer_norm"] else None,
               P.get(f"{pre}.lns.{i}.bias") if cfg["layer_norm"] else None) for i in range(cfg["gnn_layers"])]
    res = R.encoder_ref(fx["x"], rp, col, val, layers, residual=cfg["residual"], relu=cfg["relu"],
                        final_ln=(P["model.gnn_norm.weight"], P["model.gnn_norm.bias"]))
    assert np.abs(res["out"] - fx["x_node"]).max() <= FLOAT_TOL
    assert res["n_flag"] == 0 and not res["d_out"].any()


def _special_bits():
    return np.array([
        0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,        # ties: to even downwards, upwards (both signs)
        0x3F808001, 0x3F807FFF, 0x3F80FFFF,                    # just above / below a tie; carry into the exponent
        0x00000000, 0x80000000,                                # +-0
        0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x80018000,   # subnormals (ties too), largest -> min normal
        0x00800000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7FFFFF,   # min normal, max finite, overflow to inf
        0x7F800000, 0xFF800000,                                # inf
    ], np.uint32)


NAN_BITS = np.array([0x7FC00000, 0x7F800001, 0x7FBFFFFF, 0x7FFFFFFF, 0xFF812345, 0xFFFFFFFF], np.uint32)


def test_rne_bf16_bit_exact():
    """rne_bf16 against torch's cast and the host image fold.to_bf16_bits, bit for bit, on the edge cases and on a
    million random bit patterns; NaN is quieted as lpf_f32_to_bf16 does (high half | 0x40), and stays NaN in torch."""
    rng = np.random.default_rng(0)
    rand = rng.integers(0, 2 ** 32, 1_000_000, dtype=np.uint64).astype(np.uint32)
    for bits in (_special_bits(), rand):
        x = bits.view(np.float32)
        num = ~np.isnan(x)
        mine = R.rne_bf16_bits(x)
        tb = torch.from_numpy(x[num].copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        np.testing.assert_array_equal(mine[num], tb)
        np.testing.assert_array_equal(mine, fold.to_bf16_bits(x))
        # the fp64 values round the same way (the restatement rounds fp64 values, not fp32 ones)
        np.testing.assert_array_equal(R.rne_bf16(x[num]).astype(np.float32),
                                      torch.from_numpy(x[num].copy()).to(torch.bfloat16).float().numpy())
    want = np.array([0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x3F81, 0x3F80, 0x3F81, 0, 0x8000, 0, 0, 2, 0x80, 0x8002,
                     0x80, 0x7F7F, 0x7F80, 0x7F80, 0xFF80, 0x7F80, 0xFF80], np.uint16)
    np.testing.assert_array_equal(R.rne_bf16_bits(_special_bits().view(np.float32)), want)
    x = NAN_BITS.view(np.float32)
    want = ((NAN_BITS >> 16) | 0x40).astype(np.uint16)
    np.testing.assert_array_equal(R.rne_bf16_bits(x), want)
    np.testing.assert_array_equal(fold.to_bf16_bits(x), want)          # (no NaN may become inf or zero)
    assert torch.from_numpy(x.copy()).to(torch.bfloat16).isnan().all()
    assert np.isnan(R.rne_bf16(x)).all()
    # truncation (the near-miss the tests build) differs exactly where RNE rounds away from zero
    v = rand.view(np.float32)
    v = v[np.isfinite(v)].astype(np.float64)
    up = np.abs(R.rne_bf16(v)) > np.abs(R.trunc_bf16(v))
    assert 0.4 < up.mean() < 0.6


@pytest.mark.parametrize("k", [1, 16, 132])
def test_flip_flags_on_both_sides_of_a_midpoint(k):
    """A value within K 2^-24 (relative) of a rounding midpoint is flagged and charged one bf16 spacing; one just
    outside the window is not -- on both sides of the midpoint, both signs, several binades."""
    v = np.array([1.0 + 3 * 2.0 ** -7, -(2.0 ** 5) * (1.0 + 2.0 ** -7), 2.0 ** -20 * 1.5])   # bf16 values
    sp = R.bf16_spacing(v)
    mid = v + np.sign(v) * sp / 2
    win = k * R.U32 * np.abs(mid)
    for side in (-1.0, 1.0):
        inside = mid + side * 0.9 * win
        outside = mid + side * 1.1 * win * (1 + 1e-12)
        assert R.near_midpoint(inside, R.flag_window(inside, k)).all()
        assert not R.near_midpoint(outside, R.flag_window(outside, k)).any()
        r, fl, ch = R.rounded(inside, R.flag_window(inside, k))
        assert fl.all() and np.array_equal(ch, R.bf16_spacing(inside))
        # a value so close to the midpoint that fp32 error could tip it: either neighbour is one spacing away
        assert (np.abs(r - inside) <= 0.5 * sp * (1 + 1e-9)).all()
    # the floor of LayerNorm outputs widens the window of small elements only
    small = np.array([1e-3 * (1 + 2.0 ** -8)])
    assert not R.near_midpoint(small, R.flag_window(small, k)).any()
    assert R.near_midpoint(small, R.flag_window(small, k, floor=1.0) * 2.0 ** 8).all()
    # a perturbation carried into a value widens its window and adds to its charge
    x = np.array([1.0 + 2.0 ** -8 + 1e-4])
    _, fl, ch = R.rounded(x, R.flag_window(x, k), carried=np.array([2e-4]))
    assert not fl.any() and ch[0] == pytest.approx(2e-4 + 2.0 ** -7)
    # an exact tie read as it is (window 0: counts, weights, a torch cast) is never flagged
    assert not R.near_midpoint(np.array([1132.0]), np.zeros(1)).any()
