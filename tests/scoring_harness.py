"""What the GPU tests of the scoring path share (test helper, not collected): the heavy-tailed graph with its two
hubs, a model + score head + batch on it with the batch's edge cases, the inputs the fp64 restatement
(tests/bf16_reference.py) may take, the reach map over the C entry points, and the knob sets that select each
attention kernel."""
import collections

import numpy as np
import torch

import lpformer_amd
from lpformer_amd import _lib
from lpformer_amd import data as D
from tests import bf16_reference as R
from tests import param_regimes

DEV = "cuda:0"
N_ISO = 20


class Reach:
    """Call counts of the watched C entry points (wrappers on the ``_lib.hip()`` object) and, in ``log``, their names in
    the order the host called them."""

    def __init__(self, monkeypatch, names):
        self.calls = collections.Counter()
        self.log = []
        lib = _lib.hip()
        for nm in names:
            fn = getattr(lib, nm)

            def wrap(*a, _fn=fn, _nm=nm):
                self.calls[_nm] += 1
                self.log.append(_nm)
                return _fn(*a)
            monkeypatch.setattr(lib, nm, wrap)

    def ran(self, fn):
        before = dict(self.calls)
        out = fn()
        torch.cuda.synchronize()
        return out, {k for k, v in self.calls.items() if v > before.get(k, 0)}


def _graph(seed, n=2000, weighted=False):
    """Heavy-tailed graph with two hubs (700 / 650 neighbours: their pair selects > 512 nodes, the hub rows of the
    encoder are cut into parts) and N_ISO isolated nodes (their pairs select nothing)."""
    rng = np.random.default_rng(seed)
    ei, w = D.chung_lu_graph(n, 11000, gamma=2.1, seed=seed, max_weight=5 if weighted else 0)
    star = np.concatenate([np.stack([np.zeros(700, np.int64), rng.choice(np.arange(2, n - N_ISO), 700, replace=False)]),
                           np.stack([np.ones(650, np.int64), rng.choice(np.arange(2, n - N_ISO), 650, replace=False)])], 1)
    allp = np.concatenate([ei, star, star[::-1]], axis=1)
    allw = None if w is None else np.concatenate([w, np.ones(2 * star.shape[1], np.float32)])
    keep = (allp[0] < n - N_ISO) & (allp[1] < n - N_ISO)
    allp, allw = allp[:, keep], (None if allw is None else allw[keep])
    _, u = np.unique(allp[0] * n + allp[1], return_index=True)
    return allp[:, u], (None if allw is None else allw[u])


def _setup(dim, mode, seed=0, layers=1, residual=False, weighted=False, f_in=40, bs=700, att_gain=1.0, regime=None):
    """``att_gain`` multiplies the attention vector ``att`` in place: scores are linear in it, so every pair's score
    range is scaled by the gain and nothing else changes.  ``regime``: a rewrite of tests/param_regimes.py applied after
    the initialisation (None: none)."""
    n = 2000
    ei, w = _graph(seed, n, weighted)
    rng = np.random.default_rng(seed + 1)
    x = rng.standard_normal((n, f_in)).astype(np.float32)
    th = {"all": (0.0, 0.0, 1e-3), "1-hop": (0.0, 0.0, 1.0), "cn": (0.0, 1.0, 1.0)}[mode]
    data = D.build_data(ei, x, n, edge_weight=w, ppr=lpformer_amd.calc_ppr(ei, n, 0.15, 1e-4))
    args = D.train_args_for(dict(thresholds=th, dim=dim, gnn_layers=layers, residual=residual))
    torch.manual_seed(seed)
    model = lpformer_amd.LinkTransformer(args, data, device=DEV).to(DEV).eval()
    score = lpformer_amd.mlp_score(2 * dim, 2 * dim, 1, 2).to(DEV).eval()
    with torch.no_grad():
        for p in list(model.parameters()) + list(score.parameters()):
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
        if att_gain != 1.0:
            model.att_layers[0].att.att.mul_(att_gain)
    if regime is not None:
        param_regimes.apply(model, score, regime, seed)
    batch = D.sample_pairs(ei, n, bs, seed=seed + 2, frac_edges=0.3)
    iso = np.arange(n - N_ISO, n)
    batch[:, :8] = np.array([[0, 1, 0, 5, 7, 7, 0, iso[0]],
                             [1, 0, 0, 5, 9, 9, 3, iso[0]]])       # hubs, a == b, duplicates
    batch[:, 8:110] = rng.choice(iso, (2, 102))                     # pairs that select nothing: > 64 of them
    return model, score, data, torch.from_numpy(batch).to(DEV)


def _np(t):
    return t.detach().float().cpu().numpy()


def _inputs(model, score, tb, h):
    """What the restatement may take: selection records, x_node, fp32 Z and q, the fp32 fold tables."""
    model._fold_memo = None
    w = model._fold()
    z = model._node_keys(h, w)
    q = model._pair_q(tb, h, w)
    sel = [None if s is None else tuple(_np(a) if a.dtype.is_floating_point else a.cpu().numpy() for a in s)
           for s in model.compute_node_mask(tb)]
    layer, pw, ew = model.att_layers[0], model.pairwise_lin, model.elementwise_lin
    a, c, _ = model._score_fold(score)
    tt = model._tail_tables(score, a, c)
    d, pd = model.dim, model.dim + model.count_dim
    tabs = {"w_p0": pw.linears[0].weight, "b_p0": pw.linears[0].bias, "lnB_g": pw.norm.weight, "lnB_b": pw.norm.bias,
            "A": a[:, :d + pd], "c": c, "w_dot": score.lins[1].weight.reshape(-1), "b_dot": score.lins[1].bias,
            "bC_empty": tt["bC_empty"]}
    r_e = R.elementwise_hidden(_np(h), tb.cpu().numpy(), ew.linears[0].weight, ew.linears[0].bias, ew.norm.weight,
                               ew.norm.bias)
    return {"w": {k: _np(v) for k, v in w.items() if k in ("wfold", "bfold", "att", "pe_tab", "pe_stat")},
            "z": _np(z), "q": _np(q), "sel": sel, "tabs": {k: _np(v) for k, v in tabs.items()}, "r_e": r_e,
            "att_bias": _np(layer.att.bias), "ln": (_np(layer.post_att_norm.weight), _np(layer.post_att_norm.bias)),
            "bs": tb.shape[1]}


def _lite(counts, bs):
    """Pairs a lpf_tail_chain_rows_perm_* launch scores without their pairwise branch: pairs without selected nodes sit
    at positions bs - 1 - i of its order (i-th of them ascending); a 64-pair workgroup is 'lite' when it starts at or
    behind the number of pairs with selected nodes."""
    empty = counts.sum(axis=1) == 0
    n_full = int((~empty).sum())
    lite = np.zeros(bs, bool)
    pos = bs - 1 - np.arange(int(empty.sum()))
    lite[np.flatnonzero(empty)] = (pos // 64) * 64 >= n_full
    return lite


_DEFAULTS = dict(attention_impl="auto", use_select_index=True, tail_skip_empty=True, attention_rows=True,
                 use_fused_attention=True)

# name -> (model settings, stem of the entry point calc_pairwise reaches, stem of the one score_pairs reaches); the
# precision suffix (_f32, or _zbf16 / _bf16 for the matrix-core kernel) is added by ``knobs``
_KNOB_STEMS = {
    "rows4": (dict(attention_impl="flip"), "rows4", "rows4"),
    "rows": (dict(attention_impl="flip", use_select_index=False, tail_skip_empty=False), "rows", "rows"),
    "rows_perm": (dict(attention_impl="flip", use_select_index=False), "rows", "rows_perm"),
    "flip": (dict(attention_impl="flip", attention_rows=False), "flip", "flip"),
    "mfma": (dict(attention_impl="mfma"), "fused", "fused"),
}


def knobs(precision):
    """KNOBS of one attention precision ("f32" or "bf16"): name -> (model settings, entry point of calc_pairwise,
    entry points of score_pairs)."""
    def entry(stem):
        sfx = "_f32" if precision == "f32" else ("_bf16" if stem == "fused" else "_zbf16")
        return "lpf_pair_attention_" + stem + sfx
    return {name: (kn, entry(cp), {entry(sp)}) for name, (kn, cp, sp) in _KNOB_STEMS.items()}
