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

Against the model as defined (tests/unfolded_reference.py: no fold table) the bound gains one term, the conditioning of
the closed-form LayerNorm of the PE hidden layer: see "conditioning of h_e" below (``unfolded_bounds``).

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


def elementwise_window(x_node, batch, w0, b0, g, b):
    """``bf16_reference.bias_add_window`` of r_e's pre-activation W_e0 (x_a * x_b) + b_e0: what the flag window of a
    bf16 tail's r_e has to include beside K 2^-24 max(|r_e|, floor) (``tail_ref(win_re=...)``)."""
    x = _f64(x_node)
    batch = np.asarray(batch, np.int64)
    v = (x[batch[0]] * x[batch[1]]) @ _f64(w0).T + _f64(b0)
    _, xhat, sd = R.layer_norm(v, _f64(g), _f64(b))
    return R.bias_add_window(v, xhat, sd, _f64(g))


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


# ------------------------------------------------------------------------------------------------- conditioning of h_e
# The kernels evaluate the LayerNorm of the PE hidden layer from the closed form of its variance, the form
# (x, y, 1) M (x, y, 1)^T of the centred second moments M, held as fp32.  Its conditioning is kappa_e = (sum of the
# magnitudes of the form's six terms) / (var + eps), tests/unfolded_reference.py.  Written out in M's entries the form
# carries a RELATIVE error u kappa_e where its terms cancel (storage and arithmetic alike); as the sum of squares
# |L^T (x, y, 1)|^2 of M's triangular factor, which fold.pe_tables stores next to the moments and the kernels evaluate,
# u sqrt(kappa_e).
# r = 1 / sqrt(var + eps) takes half of it, and the element y = r u + beta of h_e an absolute error
#     b_h[e] = u (sqrt(kappa_e) |r u| + m_e) + u |beta|       per argument order, summed over the two orders,
# m_e >= |r u| the sum of the magnitudes of the three terms of r u (u (1 + sqrt(kappa_e)) |r u| + u |beta| where they do
# not cancel; where the first layer has learned pa - pb they cancel at the same entries at which the variance does, and
# m_e ~ sqrt(kappa_e) |r u| there).  K_e's term |Wfold_t| |h_e| (an h_e good to u |h|) does not hold this.  It reaches
# the key through |Wfold_t| and goes from there through the same carry as K_e (b_pre, b_post, then the tail), with a
# constant of its own, C_H[D]:    |got - ref| <= C_ATT b_post + C_H b_post_h.
# ``kappa="full"`` is the bound of the written-out form (u kappa_e |r u|): what the kernels were good to before.
# Everything below starts from the state dict in fp64 (|Wfold_t| = |W_rp W2_t|): the bound reads no fold table.
PE_KEYS = ("ppr_encoder_cn", "ppr_encoder_onehop", "ppr_encoder_non1hop")


def fold64(msd, dim):
    """wfold [3, D, D] = W_rp W2_t, bfold [3, D] = W_rp (2 b2_t) and att in fp64 from the fp64 state dict ``msd``."""
    w_rp = msd["att_layers.0.att.lin_r.weight"][:, dim:]
    wfold, bfold = np.zeros((3, dim, dim)), np.zeros((3, dim))
    for t, k in enumerate(PE_KEYS):
        if f"{k}.linears.1.weight" in msd:
            wfold[t] = w_rp @ msd[f"{k}.linears.1.weight"]
            bfold[t] = w_rp @ (2.0 * msd[f"{k}.linears.1.bias"])
    return {"wfold": wfold, "bfold": bfold, "att": msd["att_layers.0.att.att"].reshape(-1)}


def tail_fold64(msd, ssd, dim):
    """The tables ``tail_bound`` / ``tail_sigma`` take, folded in fp64 from the state dicts (for the BOUND only: the
    unfolded reference computes its logits layer by layer)."""
    we1, be1 = msd["elementwise_lin.linears.1.weight"], msd["elementwise_lin.linears.1.bias"]
    wp1, bp1 = msd["pairwise_lin.linears.1.weight"], msd["pairwise_lin.linears.1.bias"]
    ws0, bs0 = ssd["lins.0.weight"], ssd["lins.0.bias"]
    a = np.concatenate([ws0[:, :dim] @ we1, ws0[:, dim:] @ wp1], axis=1)
    return {"w_p0": msd["pairwise_lin.linears.0.weight"], "b_p0": msd["pairwise_lin.linears.0.bias"],
            "lnB_g": msd["pairwise_lin.norm.weight"], "lnB_b": msd["pairwise_lin.norm.bias"], "A": a,
            "c": bs0 + ws0[:, :dim] @ be1 + ws0[:, dim:] @ bp1, "w_dot": ssd["lins.1.weight"].reshape(-1),
            "b_dot": ssd["lins.1.bias"]}


def h_bound(ent, msd, kappa="root"):
    """b_h [E, D] with C_H = 1.  ``kappa``: "root" -- u (sqrt(kappa) |r u| + m) + u |beta| (the variance as a sum of
    squares);  "full" -- kappa in its place (the six moments written out);  "none" -- kappa dropped and m = |r u| (an h_e good
    to u |h_e|: the near-miss of a model without the term)."""
    kap = {"full": ent["kappa"], "root": np.sqrt(ent["kappa"]), "none": np.ones_like(ent["kappa"])}[kappa]
    rm0, rm1 = (ent["ru0"], ent["ru1"]) if kappa == "none" else (ent["rm0"], ent["rm1"])
    beta = np.zeros((3, ent["h"].shape[1]))
    for t, k in enumerate(PE_KEYS):
        if f"{k}.norm.bias" in msd:
            beta[t] = np.abs(msd[f"{k}.norm.bias"])
    return EPS23 * (kap[:, :1] * ent["ru0"] + rm0 + kap[:, 1:] * ent["ru1"] + rm1 + 2.0 * beta[ent["type"]])


def conditioning_bound(ref, w, qmag, att_bias, ln_g, ln_b, b_h):
    """(b_pre_h, b_post_h) [bs, D]: the key error |Wfold_t| b_h carried like K_e in ``attention_bound`` (C_H = 1)."""
    pre = ref["pre"]
    ent = ref["ent"]
    acc, sens2 = np.zeros_like(pre), np.zeros_like(pre)
    if ent is not None:
        pair, tt = ent["pair"], ent["type"]
        dk = np.zeros_like(b_h)
        for t in range(3):
            m = tt == t
            if m.any():
                dk[m] = b_h[m] @ np.abs(w["wfold"][t]).T
        terms = np.abs(w["att"] * qmag[pair]) * dk
        ds = np.sqrt((terms * terms).sum(axis=1))
        dev = np.abs(ent["k"] - (pre - _f64(att_bias))[pair])
        np.add.at(acc, pair, ent["alpha"][:, None] * dk)
        np.add.at(sens2, pair, (ent["alpha"][:, None] * dev * ds[:, None]) ** 2)
    _, xhat, sd = R.layer_norm(pre, _f64(ln_g), _f64(ln_b))
    b_pre = acc + np.sqrt(sens2)
    return b_pre, R.ln_bound(b_pre, xhat, sd, _f64(ln_g))


# ------------------------------------------------------------------------------------------------- bf16 kernels
# A bf16 attention kernel does the fp32 kernels' arithmetic on rounded inputs (a bf16 x bf16 product is exact in the
# fp32 accumulator), so it is held to the same per-row model, stated on the restatement with that kernel's roundings
# on: K_e from the ROUNDED Z (and the rounded Wfold image and the rounded h_e for the matrix-core kernel) -- what the
# kernel multiplies --, alpha, k_e and the LayerNorm of the rounded reference, the fp32 kernels' constants, plus the
# restatement's flip bound d_post for the one value a kernel rounds after computing it (h_e, matrix-core kernel):
#     |got - ref16| <= C_ATT b_post(ref16) + C_H b_post_h(ref16) + d_post.
def h_window(sel, msd, kappa="root"):
    """Per type b_h [E_t, D] (``h_bound``, C_H = 1) of a selection, from the fp64 state dict: the fp32 error of h_e
    that the flag window of ``attention_ref(round_h=True)`` has to include beside H_TERMS 2^-24 mag."""
    from tests import unfolded_reference as U
    out = []
    for t, s in enumerate(sel):
        if s is None or not len(s[1]):
            out.append(None)
            continue
        h, ru, kap, _ = U.pe_hidden(msd, t, s[1], s[2])
        ent = {"kappa": kap, "ru0": ru[0][0], "ru1": ru[1][0], "rm0": ru[0][1], "rm1": ru[1][1], "h": h,
               "type": np.full(h.shape[0], t)}
        out.append(h_bound(ent, msd, kappa))
    return out


def attention_bf16(sel, z, q, w, att_bias, ln_g, ln_b, bs, *, fused, b_h=None, rounder=R.rne_bf16, round_z=True):
    """(ref16, bnd) of one bf16 attention kernel: the restatement with Z rounded (``fused``, the matrix-core kernel:
    the Wfold image and h_e as well, flags within H_TERMS 2^-24 mag + ``b_h``) and the C = 1 bounds on it: b_post,
    b_post_worst, K, M ... of ``attention_bound`` with the rounded tables, and b_post_h, ``b_h`` carried through
    ``conditioning_bound`` (zero without ``b_h``).  ``b_h``: ``h_window``'s list.  Z is the fp32 table the kernel's
    image is cast from.  ``round_z=False`` (with ``fused=False``): nothing is rounded -- an fp32 kernel's reference and
    bound in the same form."""
    assert round_z or not fused
    factor = np.shape(w["pe_stat"])[0] >= 6         # (the factor rows, where the tables have them: the kernels' form)
    ref = attention(sel, z, q, w, att_bias, ln_g, ln_b, bs, round_z=round_z, round_h=fused, round_wfold=fused,
                    rounder=rounder, h_window=b_h if fused else None, factor=factor)
    w16 = {"wfold": rounder(w["wfold"]) if fused else _f64(w["wfold"]), "bfold": _f64(w["bfold"]), "att": _f64(w["att"])}
    bnd = attention_bound(ref, rounder(z) if round_z else z, w16, q, att_bias, ln_g, ln_b)
    bnd["b_post_h"] = np.zeros_like(bnd["b_post"])
    if b_h is not None and ref["ent"] is not None:
        flat = np.concatenate([b for b in b_h if b is not None])
        assert flat.shape == ref["ent"]["h"].shape
        bnd["b_post_h"] = conditioning_bound(ref, w16, np.abs(_f64(q)), att_bias, ln_g, ln_b, flat)[1]
    return ref, bnd


def unfolded_bounds(ref, x_node, batch, msd, ssd, kappa="root"):
    """Every C = 1 piece of the bounds of one unfolded reference (``unfolded_reference.scoring``), from the state dicts:
    ``b_post`` (``attention_bound``; Z and q are not taken from a device here, so their D-term fp32 products are charged
    too: |Z| and |q| enter with their quadrature magnitudes sqrt(x^2 (W^2)^T + b^2) added), ``b_post_h`` (above),
    ``b_re``, the tail's tables and the tail's own share ``s_own`` of the logit's scale."""
    x, batch = _f64(x_node), np.asarray(batch, np.int64)
    d = x.shape[1]
    w = fold64(msd, d)
    w_r, b_r = msd["att_layers.0.att.lin_r.weight"], msd["att_layers.0.att.lin_r.bias"]
    w_l, b_l = msd["att_layers.0.att.lin_l.weight"], msd["att_layers.0.att.lin_l.bias"]
    bias = msd["att_layers.0.att.bias"]
    ln = (msd["att_layers.0.post_att_norm.weight"], msd["att_layers.0.post_att_norm.bias"])
    zmag = np.abs(x @ w_r[:, :d].T + b_r) + np.sqrt((x * x) @ (w_r[:, :d] ** 2).T + b_r ** 2)
    x2 = x[batch[0]] ** 2 + x[batch[1]] ** 2
    qmag = np.abs(ref["q"]) + np.sqrt(x2 @ (w_l ** 2).T + 2.0 * b_l ** 2)
    out = attention_bound(ref, zmag, w, qmag, bias, *ln)
    if ref["ent"] is not None:
        b_h = h_bound(ref["ent"], msd, kappa)
    else:
        b_h = None
    out["b_pre_h"], out["b_post_h"] = conditioning_bound(ref, w, qmag, bias, *ln, b_h)
    if ssd is not None:
        out["tabs"] = tail_fold64(msd, ssd, d)
        out["b_re"] = elementwise_bound(x, batch, msd["elementwise_lin.linears.0.weight"],
                                        msd["elementwise_lin.linears.0.bias"], msd["elementwise_lin.norm.weight"],
                                        msd["elementwise_lin.norm.bias"])
        out["s_own"] = tail_sigma(ref["post"], ref["feats"], ref["r_e"], out["tabs"], np.zeros_like(ref["post"]),
                                  out["b_re"])
    return out


def row_bound(bnd, c_att, c_h):
    return c_att * bnd["b_post"] + c_h * bnd["b_post_h"]


def logit_bound(ref, bnd, rows_b, c_tail):
    """c_tail s_l with the rows at ``rows_b`` (``row_bound``), in quadrature with the tail's own roundings."""
    s_rows = tail_sigma(ref["post"], ref["feats"], ref["r_e"], bnd["tabs"], rows_b, np.zeros_like(bnd["b_re"]), own=False)
    return c_tail * np.sqrt(s_rows ** 2 + bnd["s_own"] ** 2)


def layer_norm_moments_f32(pre, ln_g, ln_b):
    """Near-miss: LayerNorm in float32 with the variance taken as E[x^2] - E[x]^2."""
    f = np.float32
    x = np.asarray(pre, f)
    n = f(x.shape[1])
    mu = x.sum(axis=1, keepdims=True, dtype=f) / n
    var = (x * x).sum(axis=1, keepdims=True, dtype=f) / n - mu * mu
    return (x - mu) / np.sqrt(np.maximum(var, f(0)) + f(R.LN_EPS)) * np.asarray(ln_g, f) + np.asarray(ln_b, f)


# ------------------------------------------------------------------------------------------------- fp32 evaluation
def attention_f32(sel, z, q, w, att_bias, ln_g, ln_b, bs, *, shift=True, score_rounder=None, factor=False):
    """The same algebra in plain float32 numpy, entries in order, np.float32 throughout (what the bound is checked
    against on the CPU).  ``shift=False``: the softmax without its maximum shift;  ``score_rounder``: the scores pass
    through it before the softmax (near-misses that the bound has to reject).  The variance is the quadratic form of the
    six centred second moments (rows 0-2 of ``pe_stat``) written out;  ``factor``: the sum of squares of the moment
    matrix's triangular factor (rows 3-5), which is what the kernels evaluate."""
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
        st = stat[3 + t] if factor else stat[t]

        def half(x, y):
            if not factor:
                var = st[0] * x * x + st[1] * y * y + st[2] + f(2) * (st[3] * x * y + st[4] * x + st[5] * y)
                r = f(1) / np.sqrt(np.maximum(var, f(0)) + f(R.LN_EPS))
            else:
                a, b = st[0] * x + st[1] * y + st[2], st[3] * y + st[4]
                r = f(1) / np.sqrt(a * a + b * b + st[5] * st[5] + f(R.LN_EPS))
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
