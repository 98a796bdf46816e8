"""fp64 restatement of the folded scoring path with switches for the roundings of the bf16 kernels (test helper).

The bf16 entry points round at a few documented points and keep everything else in fp32:
  * ``*_zbf16`` attention kernels: the node table Z (a torch cast, round to nearest even);
  * ``lpf_pair_attention_fused_bf16``: Z, the Wfold image (host RNE) and h_e = h_ab + h_ba (the SUM, in the kernel);
  * tail ``*_bf16`` kernels: the wB / wC weight images and every activation as it enters one of the two GEMMs;
  * ``lpf_gcn_layer_fused_bf16``: the layer INPUT X that the aggregation gathers (aggregate, then transform: the
    fused layer computes epilogue((A_hat bf16(X)) W^T)); layer 0 gathers a torch cast of the features, later layers the
    permuted image the previous layer wrote of its own fp32 output.
Everything here is fp64; a switch turns one rounding on.  Nothing is taken from a bf16 kernel's output.

Flip accounting.  A value that the kernel produces itself from fp32 arithmetic (h_e, tail activations, encoder layer
outputs) and then rounds may land on the other bf16 neighbour than the fp64 value when it lies within the fp32 error of
a rounding midpoint.  ``near_midpoint`` flags such elements: |x - mid| <= K 2^-24 max(|x|, floor) with K the length of
the producing dot product (fp32 accumulation of K terms: relative error K 2^-24 in the worst case); ``floor`` is the
row's RMS / sqrt(K) for LayerNorm outputs, whose error is absolute (that of the pre-activation, ~sqrt(K) 2^-24 times the
row's scale) rather than relative to the element.  Each flagged element is charged one bf16 spacing, carried to every
output through the absolute values of the downstream coefficients (``ln_bound`` for a LayerNorm, 1-Lipschitz ReLUs):
that is the ``flip`` bound every function returns next to its result.  A perturbation already carried into a value is
added to its flagging window and to its charge, so roundings further down that it may tip are covered as well.
Where a value's fp32 error is not of that form the caller widens the window: h_e by the conditioning of the closed-form
PE variance (``attention_ref(h_window=...)``), the tail's activations by the rounding of the bias add in front of their
LayerNorm (``bias_add_window``).  The charge of h_e goes through the softmax in a form that holds for any size of the
score change (``attention_ref``), proved by perturbation in tests/test_bf16_reference_host.py.
"""
from __future__ import annotations

import numpy as np
import torch

U32 = 2.0 ** -24          # unit roundoff of fp32
BF16_MAX = float(np.float32(3.3895313892515355e38))   # largest finite bf16 (0x7f7f)
LN_EPS = 1e-5


def _f64(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().double().numpy()
    with np.errstate(invalid="ignore"):        # (signalling NaN inputs of the bit tests)
        return np.asarray(x, np.float64)


def bf16_spacing(x) -> np.ndarray:
    """Distance between the two bf16 values around |x| (8 significant bits; subnormal spacing 2^-133)."""
    x = _f64(x)
    _, e = np.frexp(np.where(np.isfinite(x), x, 0.0))      # x = m 2^e, 0.5 <= |m| < 1
    return np.ldexp(1.0, np.maximum(e, -125) - 8)


def rne_bf16(x) -> np.ndarray:
    """x (any float) rounded to bf16, to nearest, ties to even -- returned as fp64 values.  Written from the format,
    not from the bit trick: the value is scaled by its bf16 spacing (a power of two, so exactly) and rounded to an
    integer with numpy's round-half-even.  Overflow goes to +-inf, NaN stays NaN."""
    x = _f64(x)
    s = bf16_spacing(x)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.round(x / s) * s
        r = np.where(np.abs(r) > BF16_MAX, np.copysign(np.inf, x), r)
    return np.where(np.isfinite(x), r, x)


def trunc_bf16(x) -> np.ndarray:
    """x rounded to bf16 towards zero (what a kernel that drops the low 16 bits computes; tests' near-miss)."""
    x = _f64(x)
    s = bf16_spacing(x)
    return np.where(np.isfinite(x), np.trunc(x / s) * s, x)


def rne_bf16_bits(x32) -> np.ndarray:
    """bf16 bit patterns (uint16) of an fp32 array: ``rne_bf16`` for numbers, the kernels' quieting for NaN
    (csrc/lpf_common.h lpf_f32_to_bf16: the high half with the quiet bit set)."""
    x32 = np.ascontiguousarray(x32, np.float32)
    u = x32.view(np.uint32)
    v = rne_bf16(x32).astype(np.float32)
    bits = (v.view(np.uint32) >> 16).astype(np.uint16)
    nan = np.isnan(x32)
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), bits)


def near_midpoint(x, window) -> np.ndarray:
    """True where x lies within ``window`` (absolute) of a midpoint between two neighbouring bf16 values."""
    x = _f64(x)
    s = bf16_spacing(x)
    frac = np.abs(x) / s - np.floor(np.abs(x) / s)
    return (np.abs(frac - 0.5) * s <= window) & (window > 0)     # (a value read exactly -- window 0 -- never flips)


def flag_window(x, k: int, floor=0.0) -> np.ndarray:
    """The fp32 error window of a value produced by a K-term fp32 dot product: K 2^-24 max(|x|, floor)."""
    return k * U32 * np.maximum(np.abs(_f64(x)), floor)


def rounded(x, window, rounder=rne_bf16, carried=None):
    """(rounded x, flags, charge): ``charge`` = what the kernel's rounding of x may differ by from ours -- one bf16
    spacing where x lies within ``window`` + ``carried`` of a midpoint, plus the perturbation ``carried`` already
    carried into x.  ``flags``: the elements flagged by the fp32 window alone (the statistic the tests bound)."""
    x = _f64(x)
    c = np.zeros_like(x) if carried is None else carried
    charge = c + np.where(near_midpoint(x, window + c), bf16_spacing(x), 0.0)
    return rounder(x), near_midpoint(x, window), charge


def layer_norm(x, g, b, eps=LN_EPS):
    mu = x.mean(axis=-1, keepdims=True)
    xc = x - mu
    sd = np.sqrt((xc * xc).mean(axis=-1, keepdims=True) + eps)
    return xc / sd * g + b, xc / sd, sd


def ln_bound(dx, xhat, sd, g):
    """|dy| of y = LayerNorm(x) for |dx| <= dx, first order: dy = g / sd (dx - mean dx - xhat mean(xhat dx))."""
    return np.abs(g) / sd * (dx + dx.mean(axis=-1, keepdims=True) +
                              np.abs(xhat) * (np.abs(xhat) * dx).mean(axis=-1, keepdims=True))


def bias_add_window(v, xhat, sd, g, unit=U32):
    """|dy| of y = LayerNorm(v) from the one fp32 rounding of every element of v as the bias is added to the finished
    product (the kernels' epilogues: tail_chain.hip, dense_chain.hip): |dv| <= unit |v| for the element itself, a hard
    bound; through the row's mean and variance the n roundings are independent and add in quadrature."""
    dv = unit * np.abs(v)
    n = v.shape[-1]
    return np.abs(g) / sd * (dv + np.sqrt((dv * dv).mean(axis=-1, keepdims=True) / n) +
                             np.abs(xhat) * np.sqrt((xhat * xhat * dv * dv).mean(axis=-1, keepdims=True) / n))


def row_floor(x, k: int):
    """The absolute floor of the flag window of a LayerNorm output: row RMS / sqrt(K)."""
    return np.sqrt((x * x).mean(axis=-1, keepdims=True)) / np.sqrt(k)


# ------------------------------------------------------------------------------------------------- attention
def pe_hidden(tab, stat, pa, pb, factor=False):
    """h = ReLU(LN(W1 [pa,pb] + b1)) + ReLU(LN(W1 [pb,pa] + b1)) from ``fold.pe_tables``' rows of one type: [E, D],
    and the magnitude of its terms (the scale of its fp32 error).  ``stat``: the type's six moments (row t of
    ``pe_stat``), or with ``factor`` its factor row (3 + t) and the variance as the sum of squares."""
    tab, st = _f64(tab), _f64(stat)
    pa, pb = _f64(pa)[:, None], _f64(pb)[:, None]

    def half(x, y):
        if factor:
            a, b = st[0] * x + st[1] * y + st[2], st[3] * y + st[4]
            var = a * a + b * b + st[5] * st[5]
        else:
            var = st[0] * x * x + st[1] * y * y + st[2] + 2.0 * (st[3] * x * y + st[4] * x + st[5] * y)
        r = 1.0 / np.sqrt(np.maximum(var, 0.0) + LN_EPS)
        u = tab[:, 0] * x + tab[:, 1] * y + tab[:, 2]
        return np.maximum(r * u + tab[:, 3], 0.0), np.abs(r * u) + np.abs(tab[:, 3])
    (h1, m1), (h2, m2) = half(pa, pb), half(pb, pa)
    return h1 + h2, m1 + m2


H_TERMS = 16   # fp32 operations behind an element of h_e: 3-term u, 6-term variance, rsqrt, fma with beta, ReLU, sum


def attention_ref(sel, z, q, w, att_bias, ln_g, ln_b, bs, *, round_z=False, round_h=False, round_wfold=False,
                  drop=None, rounder=rne_bf16, ln_eps=LN_EPS, detail=False, h_window=None, flagged_to=None,
                  factor=False):
    """LinkAttention + post_att_norm on the folded tables:  k_e = Z[v] + Wfold_t h_e + bfold_t,  s_e = att .
    LeakyReLU_0.2(k_e * q[pair]),  PyG softmax per pair (max-shifted, + 1e-16), out = sum_e alpha_e k_e + bias -> LN.

    sel: per type (ix int [2, E] = (pair, node), pa, pb) or None;  z [N, D], q [bs, D] fp32;  w: ``model._fold()``
    (numpy or tensors: wfold, bfold, att, pe_tab, pe_stat).  ``drop``: (type, entry) left out (near-miss of a kernel
    that loses one entry).  Returns dict pre, post, counts [bs, 3], and the flip bound ``d_post`` of ``round_h``
    (h_e is rounded inside the kernel) with its flag statistics.  ``ln_eps``: the epsilon of post_att_norm (near-miss:
    0).  ``detail``: also ``ent``, the per-entry quantities (pair, type, node, h, k, score, alpha) in type order.
    ``h_window``: per type an absolute window [E_t, D] (or None) added to the flag window of h_e -- the fp32 error of
    h_e beyond H_TERMS 2^-24 mag, f32_error_model.h_bound: the conditioning of the closed-form variance.
    ``factor``: the variance of the PE LayerNorm as the sum of squares of the moment matrix's triangular factor (rows
    3-5 of ``pe_stat``), which is what the kernels evaluate, instead of the six moments written out (rows 0-2): the
    same function of the exact tables, but where the form cancels (kappa large) the fp32 STORAGE of the six moments
    alone moves h_e by u kappa, 1e-4 ... 3e-4 under ``pe_diff_big`` -- far outside the flag window.
    ``flagged_to``: "up", "down" or a numpy Generator -- every FLAGGED element of h_e goes to its upper / lower / a
    randomly chosen bf16 neighbour instead of the nearest (the perturbation the flip bound ``d_post`` has to cover).

    The flip bound holds for any size of the score change.  Flagged elements move k_e by at most dk_e and s_e by at
    most ds_e; the pair's weights become alpha'_e = alpha_e exp(+-ds_e) / Z, Z = sum_f alpha_f exp(+-ds_f), so
    |log Z| <= L = max(log(1 + sum_f alpha_f (e^ds_f - 1)), -log(1 - sum_f alpha_f (1 - e^-ds_f))) and
    |alpha'_e / alpha_e - 1| <= exp(ds_e + L) - 1 for EVERY entry of the pair (ds_e = 0 where nothing is flagged).  With
    out' - out = sum_e alpha'_e dk_e + sum_e (alpha'_e - alpha_e) (k_e - out):
        d_pre = sum_e alpha_e (exp(ds_e + L) dk_e + (exp(ds_e + L) - 1) |k_e - out|).
    ``ds_max``: the largest ds_e (0 without flags)."""
    z, q = _f64(z), _f64(q)
    wfold, bfold, att = _f64(w["wfold"]), _f64(w["bfold"]), _f64(w["att"])
    tab, stat = _f64(w["pe_tab"]), _f64(w["pe_stat"])
    d = z.shape[1]
    if round_z:
        z = rounder(z)
    if round_wfold:
        wfold = rounder(wfold)
    pairs, keys, hs, charges, types, nodes = [], [], [], [], [], []
    counts = np.zeros((bs, 3))
    n_flag = n_elem = 0
    for t, s in enumerate(sel):
        if s is None:
            continue
        ix, pa, pb = (_f64(a) for a in s)
        pair, node = ix[0].astype(np.int64), ix[1].astype(np.int64)
        keep = np.ones(pair.size, bool)
        if drop is not None and drop[0] == t:
            keep[drop[1]] = False
        pair, node, pa, pb = pair[keep], node[keep], pa[keep], pb[keep]
        counts[:, t] = np.bincount(pair, minlength=bs)[:bs]
        h, mag = pe_hidden(tab[t], stat[3 + t], pa, pb, factor=True) if factor else pe_hidden(tab[t], stat[t], pa, pb)
        ch = np.zeros_like(h)
        if round_h:
            win = H_TERMS * U32 * mag
            if h_window is not None and h_window[t] is not None:
                win = win + _f64(h_window[t])[keep]
            h0 = h
            h, fl, ch = rounded(h0, win, rounder)
            if flagged_to is not None:
                sp = bf16_spacing(h0)
                lo, hi = np.floor(h0 / sp) * sp, np.ceil(h0 / sp) * sp
                to = hi if flagged_to == "up" else lo if flagged_to == "down" else \
                    np.where(flagged_to.random(h0.shape) < 0.5, hi, lo)
                h = np.where(fl, to, h)
            n_flag += int(fl.sum())
            n_elem += fl.size
        keys.append(z[node] + h @ wfold[t].T + bfold[t])
        pairs.append(pair)
        hs.append(h)
        charges.append(ch)
        types.append(np.full(pair.size, t))
        nodes.append(node)
    pre = np.zeros((bs, d))
    d_pre = np.zeros((bs, d))
    ent = None
    ds_max = 0.0
    if pairs:
        pair = np.concatenate(pairs)
        k = np.concatenate(keys)
        ch = np.concatenate(charges)
        tt = np.concatenate(types)
        qe = q[pair]
        sv = k * qe
        score = (np.where(sv > 0, sv, 0.2 * sv) * att).sum(axis=1)
        smax = np.full(bs, -np.inf)
        np.maximum.at(smax, pair, score)
        e = np.exp(score - smax[pair])
        den = np.zeros(bs)
        np.add.at(den, pair, e)
        alpha = e / (den + 1e-16)[pair]
        np.add.at(pre, pair, k * alpha[:, None])
        if detail:
            ent = {"pair": pair, "type": tt, "node": np.concatenate(nodes), "h": np.concatenate(hs), "k": k,
                   "score": score, "alpha": alpha}
        hit = np.flatnonzero(ch.any(axis=1))
        if hit.size:
            # one flipped h element moves k_e by Wfold[:, k] delta and s_e by (att q) . Wfold[:, k] delta (LeakyReLU is
            # 1-Lipschitz); the weights and the output follow as the docstring says, for any size of ds_e
            dk = np.zeros((hit.size, d))
            ds = np.zeros(hit.size)
            for t in range(3):
                m = tt[hit] == t
                if m.any():
                    wa = np.abs(wfold[t])
                    dk[m] = ch[hit[m]] @ wa.T
                    ds[m] = ((np.abs(att * qe[hit[m]]) @ wa) * ch[hit[m]]).sum(axis=1)
            ph = pair[hit]
            up, dn = np.zeros(bs), np.zeros(bs)
            np.add.at(up, ph, alpha[hit] * np.expm1(ds))
            np.add.at(dn, ph, alpha[hit] * -np.expm1(-ds))
            lz = np.maximum(np.log1p(up), -np.log1p(-np.minimum(dn, 1.0 - 2.0 ** -52)))
            dev = np.abs(k - pre[pair])
            np.add.at(d_pre, pair, (alpha * np.expm1(lz)[pair])[:, None] * dev)
            grow = np.exp(ds + lz[ph])
            contrib = alpha[hit, None] * (grow[:, None] * dk + (grow - np.exp(lz[ph]))[:, None] * dev[hit])
            np.add.at(d_pre, ph, contrib)
            ds_max = float(ds.max())
    pre = pre + _f64(att_bias)
    post, xhat, sd = layer_norm(pre, _f64(ln_g), _f64(ln_b), ln_eps)
    d_post = ln_bound(d_pre, xhat, sd, _f64(ln_g))
    out = {"pre": pre, "post": post, "counts": counts, "d_post": d_post, "n_flag": n_flag, "n_elem": n_elem,
           "d_pre": d_pre, "ds_max": ds_max}
    if detail:
        out["ent"] = ent
    return out


def count_features(counts, n_counts):
    """get_structure_cnts (link_transformer.py:340-356): n_cn, n_1hop, [n_non1hop,] n_cn + n_1hop."""
    c = counts
    if n_counts == 1:
        return c[:, :1]
    if n_counts == 3:
        return np.stack([c[:, 0], c[:, 1], c[:, 0] + c[:, 1]], axis=1)
    return np.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 0] + c[:, 1]], axis=1)


# ------------------------------------------------------------------------------------------------- dense tail
def elementwise_hidden(x_node, batch, w0, b0, g, b):
    """r_e = ReLU(LN(W_e0 (x_a * x_b) + b_e0)): the elementwise branch's hidden activation."""
    x = _f64(x_node)
    batch = np.asarray(batch, np.int64)
    y, _, _ = layer_norm((x[batch[0]] * x[batch[1]]) @ _f64(w0).T + _f64(b0), _f64(g), _f64(b))
    return np.maximum(y, 0.0)


def tail_ref(rows, feats_cnt, r_e, t, *, round_act=False, round_w=False, lite=None, d_rows=None, rounder=rne_bf16,
             ln_eps=LN_EPS, f32_unit=None, win_re=None):
    """pairwise_lin's first layer + LN + ReLU, then the folded score head (``LinkTransformer._score_fold``):
        r_p = ReLU(LN_B(W_p0 [row | counts] + b_p0)),  logit = w_dot . ReLU(A [r_e | r_p] + c) + b_dot.
    t: dict w_p0 [pd, pd], b_p0, lnB_g, lnB_b, A [2D, D + pd], c [2D], w_dot [2D], b_dot, and bC_empty (lite rows).
    ``round_w`` rounds W_p0 and A (the wB / wC images), ``round_act`` the GEMM inputs [row | counts], r_e and r_p.
    ``lite`` (bool [bs]): pairs the tail takes without a pairwise branch -- w_dot . ReLU(A_e r_e + bC_empty) + b_dot
    (lpf_tail_chain_rows_perm_*: a workgroup of pairs without selected nodes).  ``d_rows``: a bound on the rows'
    error carried in (a bf16 attention upstream).  ``ln_eps``: the epsilon of LN_B (near-miss: 0).
    ``f32_unit`` / ``win_re``: the flag windows of r_p and r_e widened (windows only, nothing is charged: the tests'
    error model holds the fp32 error itself) by ``bias_add_window`` of the pre-activation behind them -- computed here
    for r_p (``f32_unit`` = 2^-24), given as ``win_re`` [bs, D] for r_e (the elementwise kernel's).
    K 2^-24 max(|x|, floor) knows nothing of a bias that the LayerNorm removes again (param_regimes' ``ln_offset``: +30
    on b_p0 and b_e0 -- the pre-activation then carries 30 2^-24 whatever its deviation from the mean is).
    Returns dict logit, r_p, d_logit (flip bound), n_flag, n_elem."""
    rows, r_e = _f64(rows), _f64(r_e)
    x = np.concatenate([rows, _f64(feats_cnt)], axis=1)
    d = rows.shape[1]
    w_p0, a = _f64(t["w_p0"]), _f64(t["A"])
    if round_w:
        w_p0, a = rounder(w_p0), rounder(a)
    kb, kc = x.shape[1], a.shape[1]
    dx = np.zeros_like(x)
    if d_rows is not None:
        dx[:, :d] = d_rows
    n_flag = n_elem = 0
    if round_act:
        win = np.zeros_like(x)
        win[:, :d] = flag_window(rows, d, row_floor(rows, d))     # post-LN rows: D-term products upstream
        x, fl, dx = rounded(x, win, rounder, dx)
        w_re = flag_window(r_e, d, row_floor(r_e, d))
        if win_re is not None:
            w_re = w_re + np.where(r_e > 0.0, _f64(win_re), 0.0)       # (a unit that is off is read as an exact 0)
        re_, fl2, dre = rounded(r_e, w_re, rounder)
        n_flag += int(fl[:, :d].sum() + fl2.sum())
        n_elem += fl[:, :d].size + fl2.size
    else:
        re_, dre = r_e, np.zeros_like(r_e)
    v = x @ w_p0.T + _f64(t["b_p0"])
    y, xhat, sd = layer_norm(v, _f64(t["lnB_g"]), _f64(t["lnB_b"]), ln_eps)
    r_p = np.maximum(y, 0.0)
    drp = ln_bound(np.abs(dx) @ np.abs(w_p0).T, xhat, sd, _f64(t["lnB_g"]))
    if round_act:
        w_rp = flag_window(r_p, kb, row_floor(r_p, kb))
        if f32_unit is not None:     # (a unit that is off is read as an exact 0)
            w_rp = w_rp + np.where(r_p > 0.0, bias_add_window(v, xhat, sd, _f64(t["lnB_g"]), f32_unit), 0.0)
        rp_, fl3, drp = rounded(r_p, w_rp, rounder, drp)
        n_flag += int(fl3.sum())
        n_elem += fl3.size
    else:
        rp_ = r_p
    hid = np.concatenate([re_, rp_], axis=1) @ a.T + _f64(t["c"])
    dh = np.concatenate([dre, drp], axis=1) @ np.abs(a).T
    wd = _f64(t["w_dot"])
    logit = np.maximum(hid, 0.0) @ wd + float(_f64(t["b_dot"]).reshape(-1)[0])
    d_logit = dh @ np.abs(wd)
    if lite is not None and lite.any():
        hl = re_[lite] @ a[:, :d].T + _f64(t["bC_empty"])
        logit[lite] = np.maximum(hl, 0.0) @ wd + float(_f64(t["b_dot"]).reshape(-1)[0])
        d_logit[lite] = (dre[lite] @ np.abs(a[:, :d]).T) @ np.abs(wd)
    return {"logit": logit, "r_p": r_p, "d_logit": d_logit, "n_flag": n_flag, "n_elem": n_elem, "kc": kc}


# ------------------------------------------------------------------------------------------------- encoder
def encoder_ref(x, rowptr, col, val, layers, *, residual, relu, final_ln, round_x=False, rounder=rne_bf16,
                dup_part=None, f32_unit=None):
    """GCN encoder as the fused layer kernel computes it:  y = LN(ReLU?)(A_hat g(X) W^T + b), X <- X + y (residual),
    gnn_norm after the last layer; g = bf16 rounding of the gathered layer input with ``round_x`` (layer 0: the
    features, a torch cast -- no flips; later layers: the kernel rounds its own fp32 output -- flagged, window
    D 2^-24 max(|x|, row RMS / sqrt(D))).  layers: list of (W [D, D], bias, ln_g or None, ln_b or None);
    final_ln: (g, b).  ``dup_part``: (layer, row, lo, hi) -- entries [lo, hi) of that row counted twice (near-miss of a
    hub-part bug).  ``f32_unit``: a layer's own fp32 error, f32_unit (|A_hat| |X| |W|^T + |b|), is added to the bound
    before its LayerNorm and carried like the rest (tests/f32_error_model.py).  Returns dict out, d_out (flip bound),
    n_flag, n_elem."""
    x = _f64(x)
    rowptr, col, val = (np.asarray(a) for a in (rowptr, col, val))
    n = rowptr.size - 1
    row_of = np.repeat(np.arange(n), np.diff(rowptr))
    col = col.astype(np.int64)
    val = _f64(val)
    a_abs = torch.sparse_coo_tensor(torch.from_numpy(np.stack([row_of, col])), torch.from_numpy(np.abs(val)), (n, n))
    a_abs = a_abs.coalesce()
    dx = np.zeros_like(x)
    n_flag = n_elem = 0
    for i, (w, b, g, be) in enumerate(layers):
        w = _f64(w)
        if round_x:
            floor = row_floor(x, x.shape[1]) if i > 0 else 0.0
            win = flag_window(x, x.shape[1], floor) if i > 0 else np.zeros_like(x)
            xr, fl, dg = rounded(x, win, rounder, dx)
            if i > 0:
                n_flag += int(fl.sum())
                n_elem += fl.size
        else:
            xr, dg = x, dx
        agg = np.zeros_like(x)
        np.add.at(agg, row_of, xr[col] * val[:, None])
        if dup_part is not None and dup_part[0] == i:
            _, r, lo, hi = dup_part
            agg[r] += (xr[col[lo:hi]] * val[lo:hi, None]).sum(axis=0)
        dagg = (a_abs @ torch.from_numpy(dg)).numpy()
        v = agg @ w.T + _f64(b)
        dv = dagg @ np.abs(w).T
        if f32_unit is not None:
            dv = dv + f32_unit * ((a_abs @ torch.from_numpy(np.abs(xr))).numpy() @ np.abs(w).T + np.abs(_f64(b)))
        if g is not None:
            v, xhat, sd = layer_norm(v, _f64(g), _f64(be))
            dv = ln_bound(dv, xhat, sd, _f64(g))
        if relu:
            v = np.maximum(v, 0.0)
        if residual and v.shape == x.shape:
            x, dx = x + v, dx + dv
        else:
            x, dx = v, dv
    x, xhat, sd = layer_norm(x, _f64(final_ln[0]), _f64(final_ln[1]))
    dx = ln_bound(dx, xhat, sd, _f64(final_ln[0]))
    return {"out": x, "d_out": dx, "n_flag": n_flag, "n_elem": n_elem}
