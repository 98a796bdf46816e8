"""The unfolded fp64 reference (tests/unfolded_reference.py), the parameter regimes (tests/param_regimes.py) and the
conditioning term of the error model (tests/f32_error_model.py) on the CPU, on a model built on the CPU and a synthetic
selection: agreement with the fp32 oracle function by function, agreement with the folded restatement at random
initialisation, the regimes' conditions that need no device, and the four near-misses, each of which must lie outside
the bound at the committed constants for at least one pair of its regime."""
import numpy as np
import pytest
import torch

import lpformer_amd
from lpformer_amd import data as D
from lpformer_amd import fold
from oracle import lpformer_oracle as O
from tests import bf16_reference as R
from tests import f32_error_model as E
from tests import param_regimes as PR
from tests import unfolded_reference as U
from tests.test_gpu_f32_reference import C_ATT
from tests.test_gpu_param_regimes import C_H

N, F_IN, BS = 300, 40, 48
TAGS = ("cn", "onehop", "non1hop")
_memo = {}


def _selection(rng):
    """Ragged pairs: pair 0 with 240 entries, pairs with 1 .. 20, pair 39 with exactly one, pairs 40 .. 47 empty; PPR-like
    values in [0, 0.3] with pa == pb on a tenth of the entries (all of pairs 1 and 2: a == b) and pb == 0 on another; pair 2
    and the single entry of pair 39 have pa == pb in [0.15, 0.3]."""
    sizes = np.concatenate([[240], rng.integers(3, 21, 38), [1], np.zeros(BS - 40, np.int64)])
    sel = []
    for t in range(3):
        cnt = sizes // 3 + (np.arange(BS) % 3 == t) * (sizes % 3)
        pair = np.repeat(np.arange(BS), cnt)
        node = rng.integers(0, N, pair.size)
        pa, pb = (0.3 * rng.random((2, pair.size)) ** 3).astype(np.float32)
        eq = (rng.random(pair.size) < 0.1) | (pair == 1) | (pair == 2)
        pb[eq] = pa[eq]
        pb[(rng.random(pair.size) < 0.1) & ~eq] = 0.0
        big = (pair == 2) | (pair == 39)      # where the variance's quadratic form cancels most: pa == pb, and large
        pa[big] = pb[big] = (0.15 + 0.15 * rng.random(int(big.sum()))).astype(np.float32)
        sel.append((np.stack([pair, node]), pa, pb))
    return sel, sizes


def _case(dim, regime, seed=0):
    key = (dim, regime, seed)
    if key in _memo:
        return _memo[key]
    rng = np.random.default_rng(seed + dim)
    data = {"x": torch.from_numpy(rng.standard_normal((N, F_IN)).astype(np.float32)), "num_nodes": N}
    args = D.train_args_for(dict(thresholds=(0.0, 0.0, 1e-3), dim=dim, gnn_layers=1, residual=False))
    torch.manual_seed(seed + dim)
    model = lpformer_amd.LinkTransformer(args, data, device="cpu").eval()
    score = lpformer_amd.mlp_score(2 * dim, 2 * dim, 1, 2).eval()
    with torch.no_grad():
        for p in list(model.parameters()) + list(score.parameters()):
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    PR.apply(model, score, regime, seed)
    sel, sizes = _selection(rng)
    x_node = rng.standard_normal((N, dim)).astype(np.float32)
    batch = rng.integers(0, N, (2, BS))
    batch[1, 1:3] = batch[0, 1:3]
    msd, ssd = U.state64(model), U.state64(score)
    ref = U.scoring(sel, x_node, batch, msd, ssd, model.count_dim)
    bnd = E.unfolded_bounds(ref, x_node, batch, msd, ssd)
    c = {"model": model, "score": score, "sel": sel, "sizes": sizes, "x": x_node, "batch": batch, "msd": msd, "ssd": ssd,
         "ref": ref, "bnd": bnd, "dim": dim, "n_counts": model.count_dim}
    _memo[key] = c
    return c


def _c_att(dim):
    return max(v[dim] for v in C_ATT.values() if dim in v)


def _rows_bound(c, bnd=None):
    return E.row_bound(bnd or c["bnd"], _c_att(c["dim"]), C_H[c["dim"]])


def _folded_f32(c):
    """The fp32 fold tables, Z and q of a case, as the product derives them from the state dict."""
    sd = {k: v for k, v in c["model"].state_dict().items()}
    dim = c["dim"]
    w = fold.fold_attention(sd, dim, 3)
    w["pe_tab"], w["pe_stat"] = fold.pe_tables(sd, dim, 3)
    x = c["x"]
    z = (x @ w["w_rx"].T + w["b_r"]).astype(np.float32)
    q = (x[c["batch"][0]] @ w["w_l"].T + w["b_l"] + x[c["batch"][1]] @ w["w_l"].T + w["b_l"]).astype(np.float32)
    ln = tuple(np.float32(c["msd"][f"att_layers.0.post_att_norm.{k}"]) for k in ("weight", "bias"))
    return (c["sel"], z, q, w, np.float32(c["msd"]["att_layers.0.att.bias"]), *ln, BS)


# ------------------------------------------------------------------------------------------------- agreement
@pytest.mark.parametrize("dim", [32, 128])
def test_unfolded_reference_matches_the_oracle(dim):
    """pos_encodings, link_attention, calc_pairwise and mlp_score of the fp32 oracle against the unfolded fp64 reference
    on the synthetic selection, at 1e-5 max(1, max|ref|): the oracle's own fp32 error (it is pinned to the reference's
    outputs at 2e-5, observed ~1e-6)."""
    c = _case(dim, "init")
    ref, msd = c["ref"], c["msd"]
    P = {f"model.{k}": np.float32(v) for k, v in msd.items()}
    P.update({f"score.{k}": np.float32(v) for k, v in c["ssd"].items()})
    sel = {tag: (s[0], s[1], s[2]) for tag, s in zip(TAGS, c["sel"])}
    ent = ref["ent"]
    pes = O.pos_encodings(sel, P)
    want = np.concatenate([ent["h"][ent["type"] == t] @ msd[f"{k}.linears.1.weight"].T + 2 * msd[f"{k}.linears.1.bias"]
                           for t, k in enumerate(U.PE_KEYS)])

    def close(name, got, want):
        err, tol = np.abs(got - want).max(), 1e-5 * max(1.0, np.abs(want).max())
        print(f"D = {dim} {name}: max |oracle - unfolded| {err:.3e} (tolerance {tol:.3e})")
        assert err <= tol, name
    close("pos_encodings", pes, want)
    ix = np.concatenate([s[0] for s in c["sel"]], axis=1)
    pre, alpha = O.link_attention(ix, c["x"], c["batch"], pes, P, BS)
    close("link_attention", pre, ref["pre"])
    close("alpha", alpha, ent["alpha"])
    pw, parts = O.calc_pairwise(c["batch"], c["x"], sel, P, want_parts=True)
    close("post_att_norm", parts["att_post_ln"], ref["post"])
    close("calc_pairwise", pw, ref["pw"])
    ew = O.mlp2((c["x"][c["batch"][0]] * c["x"][c["batch"][1]]).astype(np.float32), P, "model.elementwise_lin")
    close("elementwise_lin", ew, ref["ew"])
    _, logit = O.mlp_score(np.concatenate([ew, pw], axis=1), P)
    close("mlp_score", logit, ref["logit"])
    assert (ref["counts"].sum(axis=1) == c["sizes"]).all() and (c["sizes"] == 0).sum() == 8
    empty = c["sizes"] == 0
    assert np.ptp(ref["post"][empty], axis=0).max() == 0.0             # (no entries: LN(0 / 1e-16 + bias))


@pytest.mark.parametrize("dim", [32, 128])
def test_unfolded_reference_matches_the_folded_restatement_at_init(dim):
    """``attention_ref`` + ``tail_ref`` on the product's fp32 fold tables against the unfolded reference at random
    initialisation: within 4 x the C = 1 bound (the tables' fp32 storage, a few u x magnitude); kappa = 1 there, and the
    fp64 fold of the tail's tables reproduces the layer-by-layer logits to 1e-12."""
    c = _case(dim, "init")
    ref, bnd = c["ref"], c["bnd"]
    args = _folded_f32(c)
    got = E.attention(*args)
    b1 = E.row_bound(bnd, 1.0, 1.0)
    r = np.abs(got["post"] - ref["post"]) / b1
    print(f"D = {dim}: folded fp64 on fp32 tables vs unfolded, worst |diff| / bound(C = 1) {r.max():.3f}")
    assert r.max() <= 4.0
    assert np.array_equal(got["counts"], ref["counts"])
    kap = ref["ent"]["kappa"]
    assert kap.min() >= 0.99 and kap.max() <= 2.0, (kap.min(), kap.max())    # (below 1 by the epsilon in its denominator)
    tabs32 = {k: np.float32(v) for k, v in bnd["tabs"].items()}
    t = R.tail_ref(got["post"], ref["feats"], ref["r_e"], tabs32)
    lb = E.logit_bound(ref, bnd, b1, 1.0)
    rl = np.abs(t["logit"] - ref["logit"]) / lb
    print(f"D = {dim}: folded logits vs unfolded, worst |diff| / bound(C = 1) {rl.max():.3f}")
    assert rl.max() <= 4.0
    t64 = R.tail_ref(ref["post"], ref["feats"], ref["r_e"], bnd["tabs"])
    assert np.abs(t64["logit"] - ref["logit"]).max() <= 1e-12 * max(1.0, np.abs(ref["logit"]).max())


# ------------------------------------------------------------------------------------------------- regimes
def _points(rng, n=6000):
    pa, pb = 0.3 * rng.random((2, n)) ** 3
    pb[:n // 10] = pa[:n // 10]
    pb[n // 10:n // 5] = 0.0
    return pa, pb


@pytest.mark.parametrize("dim", [32, 128])
def test_pe_regimes_lose_digits_in_the_closed_form(dim):
    """The closed-form h_e (``bf16_reference.pe_hidden`` on the factor rows of ``fold.pe_tables``, fp64 on the fp32
    tables) against the direct LayerNorm on 6000 (pa, pb) points with pa == pb and pb == 0 among them: at ``init`` and
    ``pe_steep`` kappa is 1 and the closed form is good to 1e-6; in ``pe_diff`` / ``pe_diff_big`` kappa reaches 1e3 / 1e4
    and the stored tables alone lose digits -- 1e-5, within the u sqrt(kappa) that b_h charges for the sum of squares (the
    six moments in fp32 lost 1e-4 ... 3e-4 at the same points)."""
    pa, pb = _points(np.random.default_rng(dim))
    for regime in ("init", "pe_steep", "pe_diff", "pe_diff_big"):
        c = _case(dim, regime)
        sd = {k: v for k, v in c["model"].state_dict().items()}
        tab, stat = fold.pe_tables(sd, dim, 3)
        worst_k = worst_e = worst_r = 0.0
        for t in range(3):
            h, ru, kap, _ = U.pe_hidden(c["msd"], t, pa, pb)
            got, _ = R.pe_hidden(tab[t], stat[3 + t], pa, pb, factor=True)
            err = np.abs(got - h) / np.maximum(1.0, np.abs(h))
            ent = {"kappa": kap, "ru0": ru[0][0], "ru1": ru[1][0], "rm0": ru[0][1], "rm1": ru[1][1], "h": h,
                   "type": np.full(pa.size, t)}
            b_h = E.h_bound(ent, c["msd"])
            worst_k, worst_e = max(worst_k, float(kap.max())), max(worst_e, float(err.max()))
            worst_r = max(worst_r, float((np.abs(got - h) / b_h).max()))
        print(f"D = {dim} {regime}: kappa max {worst_k:.3g}, fp64 closed form on fp32 tables {worst_e:.2e}, "
              f"/ b_h {worst_r:.3f}")
        assert worst_r <= 1.0                       # (storage alone: inside b_h)
        if regime in ("init", "pe_steep"):
            assert worst_k <= 2.0 and worst_e <= (1e-6 if regime == "init" else 1e-5)
        else:
            assert worst_k >= (1e3 if regime == "pe_diff" else 1e4)


@pytest.mark.parametrize("dim", [32, 128])
def test_regime_conditions_on_the_synthetic_case(dim):
    """The conditions of tests/param_regimes.py that need no device, on the synthetic selection: kappa of the pe_diff
    regimes, flipped units and the no-flip radius of pe_steep, ln_offset's exact invariance, ln_flat's row variance; and
    ``init`` is the control (``apply`` leaves every parameter bitwise alone)."""
    init = _case(dim, "init")
    for regime in PR.REGIMES[1:]:
        c = _case(dim, regime)
        sd = {k: v for k, v in c["model"].state_dict().items()}
        plain = None
        if regime == "ln_offset":
            plain = U.scoring(c["sel"], c["x"], c["batch"], PR.without_offset(c["msd"]), c["ssd"], c["n_counts"])
        fig = PR.conditions(regime, c["ref"], init_ref=init["ref"], plain_ref=plain, sel=c["sel"],
                            radius=PR.radii(sd, dim))
        print(f"D = {dim} {regime}: {fig}")
    before = {k: v.clone() for k, v in init["model"].state_dict().items()}
    PR.apply(init["model"], init["score"], "init")
    assert all(torch.equal(v, before[k]) for k, v in init["model"].state_dict().items())


# ------------------------------------------------------------------------------------------------- teeth
def _outside(name, near, c, bnd=None):
    """Largest |near - ref| / bound over the rows at the committed constants; asserts that some pair is outside."""
    r = np.abs(np.asarray(near, np.float64) - c["ref"]["post"]) / _rows_bound(c, bnd)
    print(f"D = {c['dim']} teeth {name}: worst |near-miss - ref| / bound {r.max():.2f}; pairs outside "
          f"{int((r.max(axis=1) > 1.0).sum())} of {BS}")
    assert (r.max(axis=1) > 1.0).any(), name
    return r


@pytest.mark.parametrize("dim", [32, 128])
def test_teeth_epsilon_left_out(dim):
    """(a) post_att_norm without its epsilon in ``ln_flat`` (row variances of the order of the epsilon), and the PE
    LayerNorms without theirs in ``pe_diff`` (at pa == pb the hidden layer's variance is 1e-4)."""
    c = _case(dim, "ln_flat")
    near = U.scoring(c["sel"], c["x"], c["batch"], c["msd"], ln_eps=0.0)
    _outside("(a) post_att_norm eps = 0 [ln_flat]", near["post"], c)
    c = _case(dim, "pe_diff")
    near = U.scoring(c["sel"], c["x"], c["batch"], c["msd"], pe_eps=0.0)
    _outside("(a) PE eps = 0 [pe_diff]", near["post"], c)


@pytest.mark.parametrize("dim", [32, 128])
def test_teeth_pattern_of_the_origin_everywhere(dim):
    """(b) every entry evaluated with the ReLU states of (0, 0) -- a no-flip radius of infinity -- in ``pe_steep``."""
    c = _case(dim, "pe_steep")
    near = U.scoring(c["sel"], c["x"], c["batch"], c["msd"], origin_only=True)
    _outside("(b) origin pattern [pe_steep]", near["post"], c)


@pytest.mark.parametrize("dim", [32, 128])
def test_teeth_variance_from_raw_moments(dim):
    """(c) post_att_norm in fp32 with its variance as E[x^2] - E[x]^2 in ``ln_offset`` (rows at 30 +- 1); the two-pass
    fp32 LayerNorm of the same rows stays inside."""
    c = _case(dim, "ln_offset")
    ln = tuple(c["msd"][f"att_layers.0.post_att_norm.{k}"] for k in ("weight", "bias"))
    _outside("(c) E[x^2] - E[x]^2 [ln_offset]", E.layer_norm_moments_f32(c["ref"]["pre"], *ln), c)
    two_pass = O.layer_norm(np.float32(c["ref"]["pre"]), np.float32(ln[0]), np.float32(ln[1]))
    assert (np.abs(two_pass - c["ref"]["post"]) <= _rows_bound(c)).all()


@pytest.mark.parametrize("dim", [32, 128])
def test_teeth_kappa_dropped_from_the_bound(dim):
    """(d) in ``pe_diff_big`` the plain fp32 evaluation of the variance from the six moments written out (``attention_f32``
    as it stands, on rows 0-2 of ``pe_stat``: the form the kernels evaluated before they read the triangular factor)
    is outside the bound whose b_h has
    the conditioning dropped (an h_e good to u |h_e|) for at least one pair: the term does work.  The evaluation on the
    factor rows (the sum of squares, ``factor``) is inside the committed bound, sqrt(kappa) in b_h; the ratios of both
    evaluations to both bounds are printed (written out: 2.2 / 0.97 x the committed bound at D = 32 / 128, sum of squares
    0.07 / 0.09; the sum of squares is 1.3 / 0.5 x the bound without the term).  At ``init`` the evaluation is inside
    both."""
    c = _case(dim, "pe_diff_big")
    args = _folded_f32(c)
    dropped = E.unfolded_bounds(c["ref"], c["x"], c["batch"], c["msd"], None, kappa="none")
    old = E.attention_f32(*args)
    _outside("(d) six moments written out, kappa dropped [pe_diff_big]", old["post"], c, dropped)
    r_old = (np.abs(old["post"].astype(np.float64) - c["ref"]["post"]) / _rows_bound(c)).max()
    got = E.attention_f32(*args, factor=True)
    err = np.abs(got["post"].astype(np.float64) - c["ref"]["post"])
    print(f"D = {dim}: six moments written out / committed bound {r_old:.3f}; sum of squares / committed bound "
          f"{(err / _rows_bound(c)).max():.3f}, "
          f"/ bound with kappa dropped {(err / _rows_bound(c, dropped)).max():.3f}")
    assert (err <= _rows_bound(c)).all()
    c0 = _case(dim, "init")
    d0 = E.unfolded_bounds(c0["ref"], c0["x"], c0["batch"], c0["msd"], None, kappa="none")
    for got0 in (E.attention_f32(*_folded_f32(c0), factor=True), E.attention_f32(*_folded_f32(c0))):
        err0 = np.abs(got0["post"].astype(np.float64) - c0["ref"]["post"])
        assert (err0 <= _rows_bound(c0, d0)).all() and (err0 <= _rows_bound(c0)).all()
