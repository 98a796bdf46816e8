"""Error model of the fp32 scoring kernels, stated per pair and per feature from the fp64 restatement
(tests/bf16_reference.py with every rounding switch off).  Test helper; everything here is fp64.

Why not C 2^-23 max|ref|.  An fp32 score s_e = sum_j att_j LeakyReLU(k_ej q_pj) carries an ABSOLUTE error proportional
to the sum of the magnitudes of its terms, and that error goes straight into alpha_e = softmax(s)_e: d alpha_e =
alpha_e (ds_e - sum_f alpha_f ds_f).  With large scores (a trained ``att``) this is the dominant term, and it does not
scale with max|ref|.  So the bound is built from the reference's own quantities (u = 2^-23, one constant C per kernel
family, see tests/test_gpu_f32_reference.py):

  key magnitude      K_e = |Z[v_e]| + |Wfold_t| |h_e| + |bfold_t|                         [E, D]
                     (k_e = Z[v_e] + Wfold_t h_e + bfold_t is a D-term fp32 product: |dk_e| <= C u K_e)
  score magnitude    M_e = sqrt( sum_j (att_j q_pj K_ej)^2 )   <=   M1_e = sum_j |att_j q_pj| K_ej     [E]
                     The score is a sum of D products whose rounding errors are independent and of either sign: the
                     error of the sum grows like the root of the sum of their squares, not like the sum of their
                     magnitudes, which all D errors would have to be aligned to reach.  M1_e is the worst case; measured
                     on an MI355X it makes the bound of a many-entry row at random-init scores 1.4 (D = 32) to 2.7
                     (D = 128) times what M_e gives, for rows whose error is a tenth of it.  ``b_post_worst``,
                     the bound with M1_e, is returned as well: b_post <= b_post_worst everywhere, so nothing held to
                     b_post is held to less than the worst case would hold it to.
                     (|LeakyReLU(x)| <= |x|; |ds_e| <= C u M_e covers the products' rounding and dk_e carried into
                      the score.  The fast exponential adds an argument error u |s_e - max s| <= u (|s_e| + |max s|):
                      |s_e| <= M_e, and the magnitude sums of one pair's entries are alike, so the measured C
                      absorbs it)
  pre-norm row       out_p = sum_e alpha_e k_e + bias:
                     d out_p = sum_e alpha_e dk_e + sum_e d alpha_e k_e
                             = sum_e alpha_e dk_e + sum_e alpha_e (k_e - out_p) ds_e     (sum_e alpha_e (k_e - out_p) = 0)
                     b_pre[p] = C u ( sum_e alpha_e K_e + |bias| + sqrt( sum_e (alpha_e |k_e - out_p| M_e)^2 ) )
                     (the score errors ds_e of different entries come from different products: independent, so
                      their weighted sum adds in quadrature as well; the worst case sum_e alpha_e |k_e - out_p| M1_e
                      is what ``b_post_worst`` keeps.  With the worst case a 100-entry row at random-init scores has
                      a bound ten times its error while a one-entry row sits at a third of its own: one constant
                      cannot fit both.  In quadrature the two kinds of row sit at the same 0.3 ... 0.6.)
  post-norm row      b_post = ln_bound(b_pre, xhat, sd, g) + C u max(1, |post|)
                     (first-order LayerNorm sensitivity, 1 / sd of the row itself -- no row is excluded -- plus the
                      LayerNorm's own arithmetic on a value of size max(1, |post|))
  elementwise branch r_e = ReLU(LN(W_e0 (x_a * x_b) + b_e0)) comes from an fp32 kernel as well:
                     b_re = ln_bound(C u (|x_a x_b| |W_e0|^T + |b_e0|)) + C u max(1, |r_e|)
  logit, worst case  tail_ref(..., d_rows = b_post)["d_logit"]     (the rows' bound carried through |W_p0|, LN_B, |A|,
                     |w_dot|) + C_tail u T,  T = the magnitude sums of the two products carried the same way:
                     m1 = |[row | counts]| |W_p0|^T + |b_p0| -> b_rp = ln_bound(m1) + max(1, |r_p|),
                     m2 = |[r_e | r_p]| |A|^T + |c| + [b_re | b_rp] |A|^T,   T = (m2 + ReLU(hid)) . |w_dot| + |b_dot|
                     (a 'lite' pair -- scored without its pairwise branch -- keeps the r_e half and bC_empty only)
  logit              The worst case adds D x 2 D magnitudes as if every element's error had the sign of its
                     coefficient: 1e-3 (D = 32) to 1e-1 (D = 256) for logits whose fp32 error is 1e-7, and wider than
                     the 1e-4 it was to supersede.  ``tail_sigma`` carries the same quantities in quadrature
                     (independent errors through a linear map: variances add with the squared coefficients; the
                     LayerNorm's three first-order terms likewise, its means over D elements divided by D):
                       s_v^2 = s_x^2 (W_p0^2)^T + u^2 (x^2 (W_p0^2)^T + b_p0^2),   s_x = C_att b_post on the row part
                       s_rp^2 = (g / sd)^2 (s_v^2 + mean s_v^2 / D + xhat^2 mean(xhat^2 s_v^2) / D) + u^2 max(1, |y|)^2
                       s_h^2 = [b_re^2 | s_rp^2] (A^2)^T + u^2 ([r_e | r_p]^2 (A^2)^T + c^2)
                       s_l^2 = s_h^2 . w_dot^2 + u^2 (ReLU(hid)^2 . w_dot^2 + b_dot^2)
                     and the logit bound is C_tail s_l (never above the worst case: the tests assert it).
  encoder            per layer C_enc u (|A_hat| |X| |W|^T + |b|) added before the layer's LayerNorm and carried with
                     ln_bound as ``encoder_ref`` carries its dx, + C_enc u max(1, |out|) for the final LayerNorm.

``drop_effect`` is the closed form behind the lost-entry near-miss: without entry e the softmax of the remaining
entries is alpha_f / (1 - alpha_e), so  out' - out = (out - alpha_e k_e) / (1 - alpha_e) - out
= alpha_e / (1 - alpha_e) (out - k_e)  (the 1e-16 in the denominator aside).
"""
from __future__ import annotations

import numpy as np

from tests import bf16_reference as R

EPS23 = 2.0 ** -23
_f64 = R._f64


def pow2_ceil(x: float) -> float:
    """x rounded up to a power of two."""
    return float(2.0 ** np.ceil(np.log2(x)))


def attention(sel, z, q, w, att_bias, ln_g, ln_b, bs, **kw):
    """``attention_ref`` with every rounding off and the per-entry quantities the bound needs."""
    return R.attention_ref(sel, z, q, w, att_bias, ln_g, ln_b, bs, detail=True, **kw)


def score_ranges(ref, bs):
    """max_e s_e - min_e s_e per pair (0 for pairs without entries)."""
    ent = ref["ent"]
    hi, lo = np.full(bs, -np.inf), np.full(bs, np.inf)
    if ent is not None:
        np.maximum.at(hi, ent["pair"], ent["score"])
        np.minimum.at(lo, ent["pair"], ent["score"])
    return np.where(np.isfinite(hi), hi - lo, 0.0)


def attention_bound(ref, z, w, q, att_bias, ln_g, ln_b):
    """The bounds with C = 1 (they are linear in C): dict b_pre, b_post [bs, D], b_post_worst (M1 in place of M), and per
    entry K [E, D], M, M1 [E]."""
    z, q, g = _f64(z), _f64(q), _f64(ln_g)
    wfold, bfold, att = _f64(w["wfold"]), _f64(w["bfold"]), _f64(w["att"])
    pre = ref["pre"]
    bias = _f64(att_bias)
    acc, acc1, sens2 = np.zeros_like(pre), np.zeros_like(pre), np.zeros_like(pre)
    ent = ref["ent"]
    kmag = mmag = m1 = None
    if ent is not None:
        pair, tt = ent["pair"], ent["type"]
        kmag = np.abs(z[ent["node"]])
        for t in range(wfold.shape[0]):
            m = tt == t
            if m.any():
                kmag[m] += np.abs(ent["h"][m]) @ np.abs(wfold[t]).T + np.abs(bfold[t])
        terms = np.abs(att * q[pair]) * kmag
        mmag, m1 = np.sqrt((terms * terms).sum(axis=1)), terms.sum(axis=1)
        dev = np.abs(ent["k"] - (pre - bias)[pair])
        np.add.at(acc, pair, ent["alpha"][:, None] * kmag)
        np.add.at(sens2, pair, (ent["alpha"][:, None] * dev * mmag[:, None]) ** 2)
        np.add.at(acc1, pair, ent["alpha"][:, None] * (kmag + dev * m1[:, None]))
    post, xhat, sd = R.layer_norm(pre, g, _f64(ln_b))
    own = EPS23 * np.maximum(1.0, np.abs(post))
    b_pre, b_pre1 = EPS23 * (acc + np.abs(bias) + np.sqrt(sens2)), EPS23 * (acc1 + np.abs(bias))
    return {"b_pre": b_pre, "b_post": R.ln_bound(b_pre, xhat, sd, g) + own, "K": kmag, "M": mmag, "M1": m1,
            "b_post_worst": R.ln_bound(b_pre1, xhat, sd, g) + own, "sd": sd[:, 0]}


def drop_effect(ref, att_bias):
    """Pre-norm move of each entry's row when that entry is lost: alpha_e / (1 - alpha_e) (out_p - k_e)  [E, D]
    (entries that are alone in their pair: inf / nan -- the row becomes the bias)."""
    ent = ref["ent"]
    out = (ref["pre"] - _f64(att_bias))[ent["pair"]]
    a = ent["alpha"][:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        return a / (1.0 - a) * (out - ent["k"])


def elementwise_bound(x_node, batch, w0, b0, g, b):
    """Bound (C = 1) of r_e = ReLU(LN(W_e0 (x_a * x_b) + b_e0)) as an fp32 kernel leaves it."""
    x = _f64(x_node)
    batch = np.asarray(batch, np.int64)
    prod = x[batch[0]] * x[batch[1]]
    y, xhat, sd = R.layer_norm(prod @ _f64(w0).T + _f64(b0), _f64(g), _f64(b))
    mag = np.abs(prod) @ np.abs(_f64(w0)).T + np.abs(_f64(b0))
    return R.ln_bound(EPS23 * mag, xhat, sd, _f64(g)) + EPS23 * np.maximum(1.0, np.abs(y))


def tail_bound(rows, feats_cnt, r_e, t, b_rows, b_re, lite=None):
    """(carried, own), both [bs]: ``carried`` = the rows' bound ``b_rows`` through the tail (tail_ref's d_logit),
    ``own`` = 2^-23 T, the tail's own fp32 error with C_tail = 1.  The logit bound is carried + C_tail own (b_rows
    already scaled by its family's constant)."""
    ref = R.tail_ref(rows, feats_cnt, r_e, t, d_rows=b_rows, lite=lite)
    rows, r_e = _f64(rows), _f64(r_e)
    d = rows.shape[1]
    x = np.concatenate([rows, _f64(feats_cnt)], axis=1)
    w_p0, a, wd = _f64(t["w_p0"]), _f64(t["A"]), np.abs(_f64(t["w_dot"]))
    g = _f64(t["lnB_g"])
    y, xhat, sd = R.layer_norm(x @ w_p0.T + _f64(t["b_p0"]), g, _f64(t["lnB_b"]))
    r_p = np.maximum(y, 0.0)
    m1 = np.abs(x) @ np.abs(w_p0).T + np.abs(_f64(t["b_p0"]))
    b_rp = R.ln_bound(EPS23 * m1, xhat, sd, g) + EPS23 * np.maximum(1.0, np.abs(y))
    act = np.concatenate([r_e, r_p], axis=1)
    hid = act @ a.T + _f64(t["c"])
    m2 = EPS23 * (np.abs(act) @ np.abs(a).T + np.abs(_f64(t["c"]))) + np.concatenate([b_re, b_rp], axis=1) @ np.abs(a).T
    b_dot = abs(float(_f64(t["b_dot"]).reshape(-1)[0]))
    own = (m2 + EPS23 * np.maximum(hid, 0.0)) @ wd + EPS23 * b_dot
    if lite is not None and lite.any():
        ae = a[:, :d]
        hl = r_e[lite] @ ae.T + _f64(t["bC_empty"])
        ml = EPS23 * (np.abs(r_e[lite]) @ np.abs(ae).T + np.abs(_f64(t["bC_empty"]))) + b_re[lite] @ np.abs(ae).T
        own[lite] = (ml + EPS23 * np.maximum(hl, 0.0)) @ wd + EPS23 * b_dot
    return ref["d_logit"], own, ref["logit"]


def tail_sigma(rows, feats_cnt, r_e, t, s_rows, s_re, own=True):
    """s_l [bs]: the logit's error scale with the rows' ``s_rows`` and r_e's ``s_re`` carried in quadrature (module
    docstring); ``own=False`` leaves the tail's own roundings out.  s_l^2 is linear in (s_rows^2, s_re^2 and own^2), so
    sqrt((C s_l(s_rows, 0, own=False))^2 + s_l(0, s_re, own=True)^2) is the scale with the rows at C s_rows."""
    rows, r_e = _f64(rows), _f64(r_e)
    d = rows.shape[1]
    x = np.concatenate([rows, _f64(feats_cnt)], axis=1)
    w2, a, wd2 = _f64(t["w_p0"]) ** 2, _f64(t["A"]), _f64(t["w_dot"]) ** 2
    g = _f64(t["lnB_g"])
    u2 = EPS23 * EPS23 if own else 0.0
    sx2 = np.zeros_like(x)
    sx2[:, :d] = np.asarray(s_rows, np.float64) ** 2
    y, xhat, sd = R.layer_norm(x @ _f64(t["w_p0"]).T + _f64(t["b_p0"]), g, _f64(t["lnB_b"]))
    sv2 = sx2 @ w2.T + u2 * ((x * x) @ w2.T + _f64(t["b_p0"]) ** 2)
    n = sv2.shape[1]
    sy2 = (g / sd) ** 2 * (sv2 + sv2.mean(axis=1, keepdims=True) / n +
                           xhat ** 2 * (xhat ** 2 * sv2).mean(axis=1, keepdims=True) / n)
    sy2 = sy2 + u2 * np.maximum(1.0, np.abs(y)) ** 2
    act = np.concatenate([r_e, np.maximum(y, 0.0)], axis=1)
    hid = act @ a.T + _f64(t["c"])
    sh2 = np.concatenate([np.asarray(s_re, np.float64) ** 2, sy2], axis=1) @ (a * a).T
    sh2 = sh2 + u2 * ((act * act) @ (a * a).T + _f64(t["c"]) ** 2)
    b_dot = float(_f64(t["b_dot"]).reshape(-1)[0])
    return np.sqrt(sh2 @ wd2 + u2 * ((np.maximum(hid, 0.0) ** 2) @ wd2 + b_dot * b_dot))


def encoder_bound(x, rowptr, col, val, layers, *, residual, relu, final_ln, **kw):
    """(out, bound with C_enc = 1) of the fp32 encoder: ``encoder_ref`` carrying each layer's own fp32 error."""
    res = R.encoder_ref(x, rowptr, col, val, layers, residual=residual, relu=relu, final_ln=final_ln, round_x=False,
                        f32_unit=EPS23, **kw)
    return res["out"], res["d_out"] + EPS23 * np.maximum(1.0, np.abs(res["out"]))


# ------------------------------------------------------------------------------------------------- fp32 evaluation
def attention_f32(sel, z, q, w, att_bias, ln_g, ln_b, bs, *, shift=True, score_rounder=None):
    """The same algebra in plain float32 numpy, entries in order, np.float32 throughout (what the bound is checked
    against on the CPU).  ``shift=False``: the softmax without its maximum shift;  ``score_rounder``: the scores pass
    through it before the softmax (near-misses that the bound has to reject)."""
    f = np.float32
    z, q = np.asarray(z, f), np.asarray(q, f)
    wfold, bfold, att = (np.asarray(w[k], f) for k in ("wfold", "bfold", "att"))
    tab, stat = np.asarray(w["pe_tab"], f), np.asarray(w["pe_stat"], f)
    d = z.shape[1]
    pairs, keys = [], []
    for t, s in enumerate(sel):
        if s is None:
            continue
        pair, node = np.asarray(s[0][0], np.int64), np.asarray(s[0][1], np.int64)
        pa, pb = np.asarray(s[1], f)[:, None], np.asarray(s[2], f)[:, None]
        st = stat[t]

        def half(x, y):
            var = st[0] * x * x + st[1] * y * y + st[2] + f(2) * (st[3] * x * y + st[4] * x + st[5] * y)
            r = f(1) / np.sqrt(np.maximum(var, f(0)) + f(R.LN_EPS))
            u = tab[t][:, 0] * x + tab[t][:, 1] * y + tab[t][:, 2]
            return np.maximum(r * u + tab[t][:, 3], f(0))
        h = half(pa, pb) + half(pb, pa)
        assert h.dtype == f
        keys.append(z[node] + h @ wfold[t].T + bfold[t])
        pairs.append(pair)
    pre = np.zeros((bs, d), f)
    if pairs:
        pair, k = np.concatenate(pairs), np.concatenate(keys)
        sv = k * q[pair]
        score = (np.where(sv > 0, sv, f(0.2) * sv) * att).sum(axis=1, dtype=f)
        if score_rounder is not None:
            score = np.asarray(score_rounder(score), f)
        smax = np.full(bs, -np.inf, f)
        np.maximum.at(smax, pair, score)
        with np.errstate(over="ignore"):
            e = np.exp(score - smax[pair]) if shift else np.exp(score)
        den = np.zeros(bs, f)
        np.add.at(den, pair, e)
        with np.errstate(invalid="ignore"):
            alpha = e / (den + f(1e-16))[pair]
        np.add.at(pre, pair, k * alpha[:, None])
        assert pre.dtype == f and alpha.dtype == f
    pre = pre + np.asarray(att_bias, f)
    mu = pre.mean(axis=1, keepdims=True, dtype=f)
    xc = pre - mu
    sd = np.sqrt((xc * xc).mean(axis=1, keepdims=True, dtype=f) + f(R.LN_EPS))
    post = xc / sd * np.asarray(ln_g, f) + np.asarray(ln_b, f)
    assert post.dtype == f
    return {"pre": pre, "post": post}
