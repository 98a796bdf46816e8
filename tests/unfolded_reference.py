"""The scoring path as the model defines it, in fp64, from the state dict (test helper, plain numpy, not collected).

Nothing here reads a fold table: no ``fold.pe_tables`` closed-form variance, no Wfold / bfold, no ``_score_fold`` A / c, no
constant row for pairs without entries.  Per selected entry e of type t (reference link_transformer.py:182-211,
layers.py:161-224):

    h_e  = ReLU(LN_t(W1_t [pa, pb] + b1_t)) + ReLU(LN_t(W1_t [pb, pa] + b1_t))     LayerNorm over the D pre-activations
    pe_e = W2_t h_e + 2 b2_t
    k_e  = W_r [x_v ; pe_e] + b_r,     q_p = W_l x_a + b_l + W_l x_b + b_l
    s_e  = att . LeakyReLU_0.2(k_e * q_p),  alpha = PyG softmax per pair (max-shifted, + 1e-16)
    pre  = sum_e alpha_e k_e + bias,   post = post_att_norm(pre)
    pw   = pairwise_lin([post | counts]),  ew = elementwise_lin(x_a * x_b),  logit = score([ew | pw])  layer by layer

A pair without entries takes the same code: its sum is empty, 0 / (0 + 1e-16) + bias.

``scoring`` returns what ``bf16_reference.attention_ref(detail=True)`` returns (pre, post, counts, ent with pair, type,
node, h, k, score, alpha) plus ``logit`` and what the error model needs: per entry and argument order the conditioning
kappa of the LayerNorm's variance when it is written as the quadratic form of the centred second moments,

    var(x, y) = s0 x^2 + s1 y^2 + s2 + 2 (s3 x y + s4 x + s5 y),
    kappa     = (s0 x^2 + s1 y^2 + s2 + 2 (|s3 x y| + |s4 x| + |s5 y|)) / (var + 1e-5)      (moments in fp64)

|r u|, the LN output before beta, of both orders (the value the conditioning error multiplies), and next to it the sum of
the magnitudes of the numerator's three terms, r gamma (|w0c x| + |w1c y| + |bc|) with w0c, w1c, bc the centred columns:
what an fp32 evaluation of r u itself is good to.  It equals |r u| where the terms do not cancel and exceeds it where they
do (a first layer that has learned pa - pb, at pa ~ pb).
"""
from __future__ import annotations

import numpy as np

from tests import bf16_reference as R

PE_KEYS = ("ppr_encoder_cn", "ppr_encoder_onehop", "ppr_encoder_non1hop")
ATT = "att_layers.0.att"
LN_EPS = R.LN_EPS
_f64 = R._f64


def state64(module_or_dict) -> dict:
    """name -> fp64 array of a module's ``state_dict()`` (or of a dict of tensors / arrays)."""
    sd = module_or_dict.state_dict() if hasattr(module_or_dict, "state_dict") else module_or_dict
    return {k: _f64(v) for k, v in sd.items()}


def _ln(x, g, b, eps=LN_EPS):
    """LayerNorm over the last axis, directly: (y, xhat, var)."""
    mu = x.mean(axis=-1, keepdims=True)
    xc = x - mu
    var = (xc * xc).mean(axis=-1, keepdims=True)
    xhat = xc / np.sqrt(var + eps)
    return xhat * g + b, xhat, var[..., 0]


def moments(w1, b1):
    """The six centred second moments of (W1[:, 0], W1[:, 1], b1) over the D units, fp64."""
    a, b, c = w1[:, 0] - w1[:, 0].mean(), w1[:, 1] - w1[:, 1].mean(), b1 - b1.mean()
    return np.array([(a * a).mean(), (b * b).mean(), (c * c).mean(), (a * b).mean(), (a * c).mean(), (b * c).mean()])


def kappa(st, x, y, eps=LN_EPS):
    """Conditioning of the quadratic form of the variance at (x, y): sum of the magnitudes of its terms / (var + eps)."""
    var = st[0] * x * x + st[1] * y * y + st[2] + 2.0 * (st[3] * x * y + st[4] * x + st[5] * y)
    mag = st[0] * x * x + st[1] * y * y + st[2] + 2.0 * (np.abs(st[3] * x * y) + np.abs(st[4] * x) + np.abs(st[5] * y))
    return mag / (np.maximum(var, 0.0) + eps)


def pe_hidden(sd, t, pa, pb, eps=LN_EPS):
    """h [E, D] of one type, LayerNorm taken over the D pre-activations of each argument order; also ``ru`` (per order
    (|r u|, magnitude sum of r u), module docstring, each [E, D]), ``kappa`` [E, 2] and ``on`` (ReLU states of the two orders, bool)."""
    k = PE_KEYS[t]
    w1, b1 = sd[f"{k}.linears.0.weight"], sd[f"{k}.linears.0.bias"]
    g, be = sd[f"{k}.norm.weight"], sd[f"{k}.norm.bias"]
    pa, pb = _f64(pa), _f64(pb)
    st = moments(w1, b1)
    h, ru, on = 0.0, [], []
    for x, y in ((pa, pb), (pb, pa)):
        v = np.stack([x, y], axis=1) @ w1.T + b1
        yv, xhat, var = _ln(v, g, be, eps)
        h = h + np.maximum(yv, 0.0)
        a, b, c = w1[:, 0] - w1[:, 0].mean(), w1[:, 1] - w1[:, 1].mean(), b1 - b1.mean()
        mag = np.abs(x)[:, None] * np.abs(a) + np.abs(y)[:, None] * np.abs(b) + np.abs(c)
        ru.append((np.abs(xhat * g), mag * np.abs(g) / np.sqrt(var + eps)[:, None]))
        on.append(yv > 0.0)
    return h, ru, np.stack([kappa(st, pa, pb, eps), kappa(st, pb, pa, eps)], axis=1), on


def origin_pattern(sd, t, eps=LN_EPS):
    """ReLU states of the D hidden units of one PE MLP at (pa, pb) = (0, 0)."""
    k = PE_KEYS[t]
    y, _, _ = _ln(sd[f"{k}.linears.0.bias"][None], sd[f"{k}.norm.weight"], sd[f"{k}.norm.bias"], eps)
    return y[0] > 0.0


def mlp2(x, sd, prefix, eps=LN_EPS):
    """Linear -> LayerNorm -> ReLU -> Linear; returns (output, hidden activation, pre-norm variance)."""
    y, _, var = _ln(x @ sd[f"{prefix}.linears.0.weight"].T + sd[f"{prefix}.linears.0.bias"],
                    sd[f"{prefix}.norm.weight"], sd[f"{prefix}.norm.bias"], eps)
    hid = np.maximum(y, 0.0)
    return hid @ sd[f"{prefix}.linears.1.weight"].T + sd[f"{prefix}.linears.1.bias"], hid, var


def scoring(sel, x_node, batch, msd, ssd=None, n_counts=4, *, ln_eps=LN_EPS, pe_eps=LN_EPS, origin_only=False):
    """The whole scoring path of one batch.  sel: per type (ix [2, E] = (pair, node), pa, pb) or None; x_node [N, D] (the
    fp32 encoder output, taken as exact); batch [2, bs]; msd / ssd: ``state64`` of the model / the score head (``ssd``
    None: no tail).  Near-misses: ``ln_eps`` the epsilon of post_att_norm, ``pe_eps`` that of the PE LayerNorms,
    ``origin_only`` every hidden unit held at its ReLU state of (0, 0)."""
    x = _f64(x_node)
    batch = np.asarray(batch, np.int64)
    bs, d = batch.shape[1], x.shape[1]
    w_r, b_r = msd[f"{ATT}.lin_r.weight"], msd[f"{ATT}.lin_r.bias"]
    w_l, b_l = msd[f"{ATT}.lin_l.weight"], msd[f"{ATT}.lin_l.bias"]
    att, bias = msd[f"{ATT}.att"].reshape(-1), msd[f"{ATT}.bias"]
    q = (x[batch[0]] @ w_l.T + b_l) + (x[batch[1]] @ w_l.T + b_l)
    counts = np.zeros((bs, 3))
    parts = {k: [] for k in ("pair", "type", "node", "h", "k", "ru0", "ru1", "rm0", "rm1", "kappa", "flipped")}
    for t, s in enumerate(sel):
        if s is None:
            continue
        ix = np.asarray(s[0], np.int64)
        pair, node = ix[0], ix[1]
        counts[:, t] = np.bincount(pair, minlength=bs)[:bs]
        h, ru, kap, on = pe_hidden(msd, t, s[1], s[2], pe_eps)
        on0 = origin_pattern(msd, t, pe_eps)
        if origin_only:
            pk = PE_KEYS[t]
            h = 0.0
            for xx, yy in ((_f64(s[1]), _f64(s[2])), (_f64(s[2]), _f64(s[1]))):
                v = np.stack([xx, yy], axis=1) @ msd[f"{pk}.linears.0.weight"].T + msd[f"{pk}.linears.0.bias"]
                h = h + np.where(on0, _ln(v, msd[f"{pk}.norm.weight"], msd[f"{pk}.norm.bias"], pe_eps)[0], 0.0)
        pe = h @ msd[f"{PE_KEYS[t]}.linears.1.weight"].T + 2.0 * msd[f"{PE_KEYS[t]}.linears.1.bias"]
        parts["k"].append(np.concatenate([x[node], pe], axis=1) @ w_r.T + b_r)
        parts["pair"].append(pair)
        parts["node"].append(node)
        parts["type"].append(np.full(pair.size, t))
        parts["h"].append(h)
        for o in (0, 1):
            parts[f"ru{o}"].append(ru[o][0])
            parts[f"rm{o}"].append(ru[o][1])
        parts["kappa"].append(kap)
        parts["flipped"].append(((on[0] != on0) | (on[1] != on0)).any(axis=1))
    pre = np.zeros((bs, d))
    ent = None
    if parts["pair"]:
        ent = {k: np.concatenate(v) for k, v in parts.items()}
        pair, k = ent["pair"], ent["k"]
        sv = k * q[pair]
        score = (np.where(sv > 0, sv, 0.2 * sv) * att).sum(axis=1)
        smax = np.full(bs, -np.inf)
        np.maximum.at(smax, pair, score)
        e = np.exp(score - smax[pair])
        den = np.zeros(bs)
        np.add.at(den, pair, e)
        alpha = e / (den + 1e-16)[pair]
        np.add.at(pre, pair, k * alpha[:, None])
        ent["score"], ent["alpha"] = score, alpha
    pre = pre + bias
    post, _, var = _ln(pre, msd["att_layers.0.post_att_norm.weight"], msd["att_layers.0.post_att_norm.bias"], ln_eps)
    out = {"pre": pre, "post": post, "counts": counts, "ent": ent, "q": q, "pre_var": var}
    if ssd is not None:
        feats = R.count_features(counts, n_counts)
        pw, _, _ = mlp2(np.concatenate([post, feats], axis=1), msd, "pairwise_lin")
        ew, r_e, _ = mlp2(x[batch[0]] * x[batch[1]], msd, "elementwise_lin")
        hid = np.concatenate([ew, pw], axis=1)
        n_lin = len([k for k in ssd if k.startswith("lins.") and k.endswith(".weight")])
        for i in range(n_lin - 1):
            hid = np.maximum(hid @ ssd[f"lins.{i}.weight"].T + ssd[f"lins.{i}.bias"], 0.0)
        out["logit"] = (hid @ ssd[f"lins.{n_lin - 1}.weight"].T + ssd[f"lins.{n_lin - 1}.bias"]).reshape(-1)
        out["feats"], out["r_e"], out["pw"], out["ew"] = feats, r_e, pw, ew
    return out
