"""The fp32 error model (tests/f32_error_model.py) on the CPU, on synthetic selections and fold tables: a plain float32
evaluation of the attention algebra stays inside the bound with a single-digit constant at a narrow and at a wide score
range, near-misses are rejected at both, the closed form of the lost-entry near-miss is exact, and ``layer_norm``'s
new ``eps`` argument leaves the default result bitwise unchanged."""
import numpy as np
import pytest

from tests import bf16_reference as R
from tests import f32_error_model as E

D, N, BS = 32, 400, 48
C_HOST = 8.0            # the plain fp32 evaluation must fit C = 1 ... 8
OFFSET = 3.0            # common offset of the keys
WIDE_RANGE = 80.0       # largest score range of a pair at the wide gain (exp(+-80) is finite in fp32)


def _pe_tables(rng):
    """pe_tab [3, D, 4] / pe_stat [3, 6] of a first PE layer W1 [D, 2], b1 + LayerNorm (gamma, beta), as
    ``fold.pe_tables`` lays them out: u = gamma (a x + b y + c) with (a, b, c) centred over D, var the quadratic form."""
    tab, stat = np.zeros((3, D, 4)), np.zeros((3, 6))
    for t in range(3):
        a, b, c = (v - v.mean() for v in rng.standard_normal((3, D)))
        gamma, beta = 1.0 + 0.1 * rng.standard_normal(D), 0.1 * rng.standard_normal(D)
        tab[t] = np.stack([gamma * a, gamma * b, gamma * c, beta], axis=1)
        stat[t] = [(a * a).mean(), (b * b).mean(), (c * c).mean(), (a * b).mean(), (a * c).mean(), (b * c).mean()]
    return tab.astype(np.float32), stat.astype(np.float32)


def _case(seed=0):
    """Ragged pairs: pair 0 with 600 entries (200 of each type), pairs with 1 .. 60 entries, pairs 40 .. 47 empty,
    pair 39 with exactly one entry."""
    rng = np.random.default_rng(seed)
    sizes = np.concatenate([[600], rng.integers(6, 61, 38), [1], np.zeros(BS - 40, np.int64)])
    sel = []
    for t in range(3):
        cnt = sizes // 3 + (np.arange(BS) % 3 == t) * (sizes % 3 > 0) * (sizes % 3)   # the remainder goes to one type
        cnt[39] = 1 if t == 1 else 0
        pair = np.repeat(np.arange(BS), cnt)
        node = rng.integers(0, N, pair.size)
        ppr = rng.random((2, pair.size)).astype(np.float32) ** 3
        sel.append((np.stack([pair, node]), ppr[0], ppr[1]))
    tab, stat = _pe_tables(rng)
    w = {"wfold": (rng.standard_normal((3, D, D)) / np.sqrt(D)).astype(np.float32),
         "bfold": (OFFSET + 0.1 * rng.standard_normal((3, D))).astype(np.float32),
         "att": (rng.standard_normal(D) / np.sqrt(D)).astype(np.float32), "pe_tab": tab, "pe_stat": stat}
    z = rng.standard_normal((N, D)).astype(np.float32)
    # q carries the sign of att, so the keys' common offset (bfold) moves every score up by OFFSET sum_j |att_j q_pj|:
    # large scores as well as wide ranges (a softmax without its maximum shift then overflows at the wide gain)
    q = (np.abs(rng.standard_normal((BS, D))) * np.sign(w["att"])).astype(np.float32)
    bias = (0.1 * rng.standard_normal(D)).astype(np.float32)
    ln = ((1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32), (0.1 * rng.standard_normal(D)).astype(np.float32))
    return {"sel": sel, "z": z, "q": q, "w": w, "att_bias": bias, "ln": ln, "bs": BS, "sizes": sizes}


def _args(c):
    return c["sel"], c["z"], c["q"], c["w"], c["att_bias"], *c["ln"], c["bs"]


def _gained(c, gain):
    out = dict(c)
    out["w"] = dict(c["w"], att=(c["w"]["att"] * np.float32(gain)).astype(np.float32))
    return out


_memo = {}


def _cases():
    """(narrow, wide) with their references and bounds, built once."""
    if not _memo:
        c1 = _case()
        r1 = E.attention(*_args(c1))
        gain = WIDE_RANGE / E.score_ranges(r1, BS).max()
        for name, c in (("narrow", c1), ("wide", _gained(c1, gain))):
            ref = E.attention(*_args(c))
            bnd = E.attention_bound(ref, c["z"], c["w"], c["q"], c["att_bias"], *c["ln"])
            _memo[name] = (c, ref, bnd)
    return _memo


def _ratio(got, ref, bnd):
    with np.errstate(invalid="ignore"):
        r = np.abs(got["post"].astype(np.float64) - ref["post"]) / bnd["b_post"]
    return np.where(np.isnan(r), np.inf, r)


def test_wide_gain_range_conditions():
    """At the wide gain the 600-entry pair spans >= 30 score units, a quarter of the non-empty pairs >= 10, and exp of
    the largest difference is finite in fp32; the gain scales every range by the same factor and nothing else."""
    cs = _cases()
    rn, rw = (E.score_ranges(cs[k][1], BS) for k in ("narrow", "wide"))
    nonempty = cs["wide"][0]["sizes"] > 0
    print(f"ranges: narrow max {rn.max():.2f}, wide max {rw.max():.2f}, hub {rw[0]:.2f}, "
          f"share >= 10: {(rw[nonempty] >= 10).mean():.2f}")
    assert rw[0] >= 30 and (rw[nonempty] >= 10).mean() >= 0.25
    assert np.isfinite(np.exp(np.float32(rw.max()))) and np.exp(np.float32(-rw.max())) > 0
    gain = rw.max() / rn.max()
    np.testing.assert_allclose(rw, gain * rn, rtol=1e-5)
    assert rn.max() < 10 and (rw[~nonempty] == 0).all() and rw[39] == 0


@pytest.mark.parametrize("which", ["narrow", "wide"])
def test_plain_f32_evaluation_is_inside_the_bound(which):
    c, ref, bnd = _cases()[which]
    got = E.attention_f32(*_args(c))
    r = _ratio(got, ref, bnd)
    print(f"{which}: plain fp32 evaluation, worst |got - ref| / bound(C = 1) = {r.max():.3f} "
          f"(pre-norm: {(np.abs(got['pre'] - ref['pre']) / bnd['b_pre']).max():.3f}); bound / (1e-5 scale): "
          f"{(bnd['b_post'] / (1e-5 * max(1.0, np.abs(ref['post']).max()))).max():.3f}")
    assert r.max() <= C_HOST
    assert (bnd["b_post"] <= bnd["b_post_worst"]).all() and (bnd["M"] <= bnd["M1"]).all()   # (never above the worst case)
    assert (np.abs(got["pre"] - ref["pre"]) <= C_HOST * bnd["b_pre"]).all()
    assert (got["post"][c["sizes"] == 0] == got["post"][-1]).all()          # empty pairs: LN(bias)


@pytest.mark.parametrize("which", ["narrow", "wide"])
def test_near_miss_evaluations_are_rejected(which):
    """Scores rounded to bf16 before the softmax: outside C = 8 at both gains -- the sensitivity term grows with the
    gain because M_e does, not because the bound is loose.  Without the maximum shift the wide case overflows."""
    c, ref, bnd = _cases()[which]
    got = E.attention_f32(*_args(c), score_rounder=R.rne_bf16)
    r = _ratio(got, ref, bnd)
    multi = c["sizes"] > 1
    print(f"{which}: bf16 scores, worst ratio {r.max():.1f}; rows outside C = {C_HOST}: "
          f"{(r.max(axis=1) > C_HOST).sum()} of {multi.sum()} pairs with more than one entry")
    # (a wide pair whose softmax has saturated on one entry does not feel its other scores: not every pair, most)
    assert (r.max(axis=1) > C_HOST)[multi].mean() > 0.5 and r[0].max() > C_HOST
    assert (r[~multi] <= C_HOST).all()                                   # (one entry or none: alpha does not matter)
    noshift = E.attention_f32(*_args(c), shift=False)
    r = _ratio(noshift, ref, bnd)
    print(f"{which}: no maximum shift, worst ratio {r.max():.3g}")
    if which == "wide":
        assert (r.max(axis=1) > C_HOST).any()
    else:
        assert r.max() <= C_HOST                                         # (narrow scores: the shift is not needed)


@pytest.mark.parametrize("which", ["narrow", "wide"])
def test_drop_closed_form_matches_two_reference_runs(which):
    c, ref, _ = _cases()[which]
    eff = E.drop_effect(ref, c["att_bias"])
    ent = ref["ent"]
    ofs = np.cumsum([0] + [s[0].shape[1] for s in c["sel"]])
    rng = np.random.default_rng(1)
    # (alpha_e / (1 - alpha_e) is ill-conditioned for an entry that holds nearly all of its pair's weight: the two
    #  fp64 runs then differ by their own rounding -- entries up to alpha = 0.9 are compared)
    ok = (ent["pair"] != 39) & (ent["alpha"] <= 0.9)
    picks = [int(np.flatnonzero(ent["pair"] == 0)[0]), int(np.argmax(np.where(ok, ent["alpha"], 0)))]
    picks += [int(i) for i in rng.choice(np.flatnonzero(ok), 6, replace=False)]
    for e in picks:
        t = int(ent["type"][e])
        dropped = E.attention(*_args(c), drop=(t, e - int(ofs[t])))
        p = int(ent["pair"][e])
        diff = dropped["pre"][p] - ref["pre"][p]
        err = np.abs(diff - eff[e]).max()
        assert err <= 1e-12 * max(1.0, np.abs(eff[e]).max()), (e, err)
        others = np.arange(BS) != p
        assert np.array_equal(dropped["pre"][others], ref["pre"][others])


def test_layer_norm_eps_default_is_bitwise_the_old_result():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((50, D)) * 10.0 ** rng.integers(-4, 3, (50, 1))
    g, b = rng.standard_normal(D), rng.standard_normal(D)

    def old(x, g, b):
        mu = x.mean(axis=-1, keepdims=True)
        xc = x - mu
        sd = np.sqrt((xc * xc).mean(axis=-1, keepdims=True) + R.LN_EPS)
        return xc / sd * g + b, xc / sd, sd
    for got, want in zip(R.layer_norm(x, g, b), old(x, g, b)):
        assert got.tobytes() == want.tobytes()
    for got, want in zip(R.layer_norm(x, g, b, eps=R.LN_EPS), old(x, g, b)):
        assert got.tobytes() == want.tobytes()
    y0 = R.layer_norm(x, g, b, eps=0.0)[0]
    assert not np.array_equal(y0, R.layer_norm(x, g, b)[0])
    assert np.abs(y0 - R.layer_norm(x, g, b)[0]).max() > 1e-3        # (rows of scale 1e-4: the epsilon matters there)


@pytest.mark.parametrize("which", ["narrow", "wide"])
def test_bf16_bound_holds_a_plain_f32_evaluation_on_the_rounded_table(which):
    """``attention_bf16`` (the per-row bound of a *_zbf16 kernel: the restatement with Z rounded, K_e from the rounded
    Z): the plain fp32 evaluation on the bf16 image of Z -- what such a kernel computes -- is inside C = 1 ... 8 at both
    gains, on rows with one entry and with 600; the unrounded reference and the one that truncates Z are outside for
    most pairs; and with nothing rounded the helper returns ``attention_bound`` itself."""
    c, ref, bnd = _cases()[which]
    ref16, b16 = E.attention_bf16(*_args(c), fused=False)
    z16 = R.rne_bf16(c["z"]).astype(np.float32)
    assert np.array_equal(z16.astype(np.float64), R.rne_bf16(c["z"]))              # (bf16 values are fp32 values)
    got = E.attention_f32(c["sel"], z16, *_args(c)[2:])
    r = _ratio(got, ref16, b16)
    multi = c["sizes"] > 0
    r_plain = _ratio({"post": ref["post"]}, ref16, b16)
    trunc = E.attention(*_args(c), round_z=True, rounder=R.trunc_bf16)
    r_trunc = _ratio({"post": trunc["post"]}, ref16, b16)
    print(f"{which}: fp32 on bf16(Z) vs ref16, worst ratio {r.max():.3f}; unrounded reference {r_plain.max():.0f}, "
          f"truncating reference {r_trunc.max():.0f}")
    assert r.max() <= C_HOST and not b16["b_post_h"].any() and not ref16["d_post"].any()
    assert (r_plain.max(axis=1) > C_HOST)[multi].mean() > 0.9 and (r_trunc.max(axis=1) > C_HOST)[multi].mean() > 0.9
    same, b_same = E.attention_bf16(*_args(c), fused=False, round_z=False)
    assert np.array_equal(same["post"], ref["post"]) and np.array_equal(b_same["b_post"], bnd["b_post"])
