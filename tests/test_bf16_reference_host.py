"""The fp64 restatement of the folded scoring path (tests/bf16_reference.py) on the CPU: with every rounding switch off it
is the oracle on the reference-recorded fixtures; its bf16 rounding agrees bit for bit with torch's cast, the host
images (fold.to_bf16_bits) and the kernels' NaN quieting; its flip flags sit where they should."""
import numpy as np
import pytest
import torch

from lpformer_amd import fold
from oracle import lpformer_oracle as O
from tests import bf16_reference as R
from tests import f32_error_model as E
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


# ------------------------------------------------------------------------------------------------- flip bound of h_e
FLAG_FRACTION = 5e-3            # the cap of tests/test_gpu_bf16.py on the share of flagged elements
ROUNDED = dict(round_z=True, round_h=True, round_wfold=True)


@pytest.mark.parametrize("widen", [1.0, 64.0], ids=["window", "window-x64"])
@pytest.mark.parametrize("which", ["narrow", "wide"])
def test_flip_bound_covers_every_flagged_element_moved(which, widen):
    """The proof by perturbation of ``attention_ref``'s flip bound: every flagged element of h_e moved to its other bf16
    neighbour -- all up, all down, 32 random patterns -- and the restatement recomputed; the post-norm rows stay within
    d_post of the unperturbed ones, at gain 1 and at the gain that stretches the widest pair to 80 units (ds_e grows
    with the gain: a first-order charge alpha_e |k_e - out| ds_e is no bound there).  On the 600-entry pair of
    tests/test_f32_error_model_host.py; with the window as it is (54 flagged elements) and 64 x as wide (2309, 4 % of
    them).  1e-13 scale on top: the fp64 rounding of two evaluations of a row whose flagged entries weigh nothing."""
    from tests import test_f32_error_model_host as FH
    c = FH._cases()[which][0]
    args = FH._args(c)
    hw = None if widen == 1.0 else [np.full((s[1].size, FH.D), (widen - 1.0) * R.H_TERMS * R.U32) for s in c["sel"]]
    base = R.attention_ref(*args, h_window=hw, **ROUNDED)
    assert base["n_flag"] >= 50 and (base["d_post"] >= 0).all()
    floor = 1e-13 * max(1.0, float(np.abs(base["post"]).max()))
    worst = 0.0
    moved_any = False
    for to in ["up", "down"] + [np.random.default_rng(100 + i) for i in range(32)]:
        r = R.attention_ref(*args, h_window=hw, flagged_to=to, **ROUNDED)
        assert r["n_flag"] == base["n_flag"]
        diff = np.abs(r["post"] - base["post"])
        moved_any |= bool((diff > floor).any())
        worst = max(worst, float((diff / (base["d_post"] + floor)).max()))
        assert (diff <= base["d_post"] + floor).all(), (which, widen, to if isinstance(to, str) else "random")
    print(f"{which}, window x {widen:g}: {base['n_flag']} of {base['n_elem']} flagged, ds max {base['ds_max']:.3g}, worst "
          f"|moved - base| / d_post {worst:.3f}, d_post max {base['d_post'].max():.3e}")
    assert moved_any and worst > 0.05            # (the perturbation is real, and the bound within 20 x of it)
    # rows of pairs without a flagged entry carry no charge, and an unflagged run charges nothing
    plain = R.attention_ref(*args, round_z=True)
    assert not plain["d_post"].any() and plain["ds_max"] == 0.0


def _kappa_case(dim=32):
    from tests import test_unfolded_reference_host as UH
    c = UH._case(dim, "pe_diff_big")
    return c, UH._folded_f32(c)


def test_flip_flags_on_both_sides_of_a_midpoint_at_large_kappa():
    """The flag window of h_e under ``pe_diff_big``: an entry with pa ~ pb where the closed-form variance cancels
    (kappa >= 1e4).  Its fp32 error is b_h = u (sqrt(kappa) |r u| + m) + u |beta| (f32_error_model.h_bound), several
    times H_TERMS 2^-24 mag.  pa is moved (in fp64; pb stays) until one element of h_e sits at 0.9 / 1.1 windows on
    either side of a bf16 midpoint: inside it is flagged and charged one spacing, outside it is not -- and with the
    window that knows nothing of kappa the inside values on both sides go unflagged."""
    c, args = _kappa_case()
    sel, w = c["sel"], args[3]
    t = 0
    kap = E.h_window(sel, c["msd"])[t]                     # [E_t, D]
    from tests import unfolded_reference as U
    _, _, kappa, _ = U.pe_hidden(c["msd"], t, sel[t][1], sel[t][2])
    e = int(np.argmax(kappa.max(axis=1)))
    assert kappa[e].max() >= 1e4
    pa0, pb0 = float(sel[t][1][e]), float(sel[t][2][e])

    def h_of(pa):
        h, mag = R.pe_hidden(w["pe_tab"][t], w["pe_stat"][t], np.array([pa]), np.array([pb0]))
        return h[0], mag[0]

    def window(pa, widened):
        _, mag = h_of(pa)
        extra = E.h_window([(sel[t][0][:, :1], np.array([pa]), np.array([pb0]))], c["msd"])[0][0] if widened else 0.0
        return R.H_TERMS * R.U32 * mag + extra

    h0, _ = h_of(pa0)
    j = int(np.argmax(np.where(h0 > 0.05, kap[e] / (R.H_TERMS * R.U32 * np.maximum(h0, 1e-30)), 0.0)))
    assert h0[j] > 0.05
    wide_w, plain_w = window(pa0, True)[j], window(pa0, False)[j]
    print(f"entry {e}: kappa {kappa[e].max():.3g}, h[{j}] = {h0[j]:.6f}, window {wide_w:.3e} = {wide_w / plain_w:.1f} x "
          f"H_TERMS 2^-24 mag, bf16 spacing {R.bf16_spacing(h0[j]):.3e}")
    assert wide_w >= 2.0 * plain_w and wide_w < 0.25 * R.bf16_spacing(h0[j])
    # h_j as a function of pa around pa0: find a bracket of a midpoint target, then bisect
    sp = float(R.bf16_spacing(h0[j]))
    step = 1e-7
    grid = pa0 + step * np.arange(-4000, 4001)
    hs = np.array([h_of(p)[0][j] for p in grid])
    seen = {}
    for side in (-1.0, 1.0):
        for frac, want_flag in ((0.9, True), (1.1, False)):
            done = False
            for mid in (np.floor(h0[j] / sp) + np.array([0.5, -0.5, 1.5, -1.5])) * sp:
                target = mid + side * frac * wide_w
                s = np.flatnonzero((hs[:-1] - target) * (hs[1:] - target) <= 0)
                if not s.size:
                    continue
                lo, hi = grid[s[0]], grid[s[0] + 1]
                for _ in range(60):
                    m = 0.5 * (lo + hi)
                    if (h_of(lo)[0][j] - target) * (h_of(m)[0][j] - target) <= 0:
                        hi = m
                    else:
                        lo = m
                pa = 0.5 * (lo + hi)
                hv = h_of(pa)[0][j]
                assert abs(hv - target) <= 1e-3 * wide_w
                one = [None] * 3
                one[t] = (sel[t][0][:, e:e + 1], np.array([pa]), np.array([pb0]))
                a1 = (one,) + tuple(args[1:])
                ref = R.attention_ref(*a1, round_h=True, detail=True,
                                      h_window=E.h_window(one, c["msd"]))
                old = R.attention_ref(*a1, round_h=True)
                fl = R.near_midpoint(hv, window(pa, True)[j])
                assert bool(fl) == want_flag, (side, frac)
                if want_flag:
                    assert ref["n_flag"] >= 1 and ref["d_post"].max() > 0
                    assert not R.near_midpoint(hv, window(pa, False)[j])      # (the old window misses it)
                    assert ref["n_flag"] > old["n_flag"] or frac * wide_w <= window(pa, False)[j]
                seen[(side, frac)] = float(hv - mid)
                done = True
                break
            assert done, f"no midpoint of h[{j}] within reach of pa on side {side}"
    assert len(seen) == 4 and seen[(-1.0, 0.9)] < 0 < seen[(1.0, 0.9)]


@pytest.mark.parametrize("dim", [32, 64, 128, 256])
def test_flagged_fraction_cap_with_the_widened_window(dim):
    """The condition of tests/test_gpu_bf16_regimes.py (b), on the reference alone: with the flag window of h_e widened
    by b_h the matrix-core kernel's restatement flags fewer than FLAG_FRACTION of its elements in every one of the six
    regimes (CPU model and synthetic selection of tests/test_unfolded_reference_host.py, pa == pb on a tenth of the
    entries: more cancellation than the harness batch has).  Measured: 1.8e-4 ... 6.2e-4 (init, ln_*), 1.1e-3 ... 1.6e-3
    (pe_steep), 2.0e-3 ... 2.9e-3 (pe_diff, pe_diff_big; 6e-4 ... 1.4e-3 with the window that ignores kappa): no regime
    loses its ``mfma`` knob."""
    from tests import param_regimes as PR
    from tests import test_unfolded_reference_host as UH
    for regime in PR.REGIMES:
        c = UH._case(dim, regime)
        args = UH._folded_f32(c)
        ref, bnd = E.attention_bf16(*args, fused=True, b_h=E.h_window(c["sel"], c["msd"]))
        plain = R.attention_ref(*args, factor=True, **ROUNDED)
        frac = ref["n_flag"] / ref["n_elem"]
        print(f"D = {dim} {regime}: flagged {frac:.2e} (window without b_h: {plain['n_flag'] / plain['n_elem']:.2e}), "
              f"ds max {ref['ds_max']:.3g}")
        assert ref["n_flag"] >= plain["n_flag"] and frac < FLAG_FRACTION, (regime, frac)
        assert (bnd["b_post_h"] >= 0).all() and np.isfinite(ref["d_post"]).all()
