"""The bf16 entry points against the fp64 restatement with their roundings emulated (tests/bf16_reference.py).

Reach map -- entry point: knobs that select it (D covered here):
  lpf_pair_attention_rows4_zbf16     precision "bf16", select4 (default: walk indexes, no adj_mask), attention kernel
                                     "flip", attention_rows; calc_pairwise, and score_pairs with an order
                                     (tail_skip_empty)                                    D 64, 128, 256
  lpf_pair_attention_rows_zbf16      the same with use_select_index = False; calc_pairwise, or score_pairs with
                                     tail_skip_empty = False                               D 64, 128, 256
  lpf_pair_attention_rows_perm_zbf16 use_select_index = False, score_pairs, tail_skip_empty D 64, 128, 256
  lpf_pair_attention_flip_zbf16      attention kernel "flip", attention_rows = False       D 64, 128, 256
  lpf_pair_attention_fused_bf16      attention_impl "mfma" (the "auto" choice below D 128) D 64, 128, 256
  lpf_tail_chain_rows_perm_bf16      tail_precision "bf16", rows attention, tail_skip_empty D 64, 128, 256
  lpf_tail_chain_rows_bf16           the same with tail_skip_empty = False                 D 64, 128, 256
  lpf_tail_chain_merge_bf16          tail_precision "bf16", attention_rows = False (records + merge) D 64, 128
  lpf_gcn_layer_fused_bf16           encoder_precision "bf16", square layers (f_in = D)    D 64, 128
  lpf_spmm_row_parts_bf16p           the same on a graph with rows of more than 64 entries D 64, 128
(D = 256 with tail_precision "bf16" runs the bf16 tail: lpf_tail_chain_rows*_bf16 has a D = 256 instantiation.)

Tolerances: |got - ref| <= C 2^-23 scale + flip, scale = max(1, max |ref|), flip = the restatement's bound for
values the kernel rounds after computing them in fp32 (none for the *_zbf16 kernels: Z is read, not computed).  C is
fp32 re-association over the producing chain: C_ATT = 4 D (D-term products for k_e and for the LayerNorm statistics,
times 4 for the LayerNorm's 1 / sigma on rows whose sigma is >= 1/4 of their largest element), C_LOGIT = 16 D (two
chained products of <= 2 D + 4 terms and two LayerNorms behind the rows), C_ENC = 4 D per layer.
"""
import numpy as np
import pytest
import torch

from tests import bf16_reference as R
from tests.scoring_harness import DEV, Reach, _DEFAULTS, _inputs, _lite, _np, _setup, knobs

pytestmark = pytest.mark.gpu
EPS23 = 2.0 ** -23
OLD_ATT_TOL, OLD_ENC_TOL = 5e-3, 3e-2          # what the bf16 modes were held to against the fp32 path
FLAG_FRACTION = 5e-3

ATT_ENTRIES = ("lpf_pair_attention_rows4_zbf16", "lpf_pair_attention_rows_zbf16", "lpf_pair_attention_rows_perm_zbf16",
               "lpf_pair_attention_flip_zbf16", "lpf_pair_attention_fused_bf16")
TAIL_ENTRIES = ("lpf_tail_chain_rows_bf16", "lpf_tail_chain_rows_perm_bf16", "lpf_tail_chain_merge_bf16")
ENC_ENTRIES = ("lpf_gcn_layer_fused_bf16", "lpf_spmm_row_parts_bf16p")


def _att(inp, fused, **kw):
    return R.attention_ref(inp["sel"], inp["z"], inp["q"], inp["w"], inp["att_bias"], *inp["ln"], inp["bs"],
                           round_z=True, round_h=fused, round_wfold=fused, **kw)


def _check(name, got, ref, bound, c, d):
    """Assert |got - ref| <= c 2^-23 scale + bound; returns (max err, max err / tolerance)."""
    scale = max(1.0, float(np.abs(ref).max()))
    tol = c * EPS23 * scale + bound
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / tol).max())
    print(f"{name}: max |got - ref| {err.max():.3e}, max ratio to bound {worst:.3f} (c = {c}, D = {d})")
    assert np.isfinite(got).all() and worst <= 1.0, f"{name}: {err.max():.3e} beyond the bound"
    return float(err.max()), worst


# ------------------------------------------------------------------------------------------------- attention
KNOBS = knobs("bf16")   # name -> (model settings, entry point of calc_pairwise, entry points of score_pairs)


@pytest.mark.parametrize("dim,mode", [(64, "all"), (128, "all"), (256, "all"), (128, "1-hop"), (64, "cn")])
def test_bf16_attention_matches_rounded_reference(dim, mode, monkeypatch):
    """Every bf16 attention kernel: post-LN rows (calc_pairwise) and logits (score_pairs, fp32 tail) against the fp64
    restatement with Z rounded (and, for the matrix-core kernel, the Wfold image and h_e).  Teeth: the same reference
    with one entry of the largest pair left out is rejected for that pair."""
    model, score, data, tb = _setup(dim, mode, seed=dim + len(mode))
    reach = Reach(monkeypatch, ATT_ENTRIES + TAIL_ENTRIES)
    h = model.propagate()
    inp = _inputs(model, score, tb, h)
    bs = tb.shape[1]
    refs = {f: _att(inp, f) for f in (False, True)}
    cnt = refs[False]["counts"].sum(axis=1)
    assert cnt.max() > (512 if mode != "cn" else 96) and (cnt == 0).sum() >= 3 and (cnt == 1).any() and bs % 64
    nc = model.count_dim
    logit_ref = {}
    for f, r in refs.items():
        t = R.tail_ref(r["post"], R.count_features(r["counts"], nc), inp["r_e"], inp["tabs"], d_rows=r["d_post"])
        logit_ref[f] = t
    model.precision = "bf16"
    seen = set()
    for name, (knobs, cp_entry, sp_entries) in KNOBS.items():
        for k, v in knobs.items():
            setattr(model, k, v)
        fused = name == "mfma"
        r = refs[fused]
        _, ran = reach.ran(lambda: model.calc_pairwise(tb, h))
        got_rows = _np(model._last_att)
        assert cp_entry in ran and model.check_selection(), (name, ran)
        _check(f"{name} rows", got_rows, r["post"], r["d_post"], 4 * dim, dim)
        lg, ran2 = reach.ran(lambda: model.score_pairs(tb, h, score, logits=True))
        assert sp_entries <= ran2 and model.check_selection(), (name, ran2)
        _check(f"{name} logits", _np(lg), logit_ref[fused]["logit"], logit_ref[fused]["d_logit"], 16 * dim, dim)
        seen |= ran | ran2
        if fused:
            frac = r["n_flag"] / max(1, r["n_elem"])
            print(f"h_e flagged fraction {frac:.2e} ({r['n_flag']} of {r['n_elem']})")
            assert frac < FLAG_FRACTION
        if name == "rows4" and mode == "all":
            # bs = 1: the hub pair alone
            one = tb[:, :1].contiguous()
            i1 = _inputs(model, score, one, h)
            r1 = _att(i1, False)
            model.calc_pairwise(one, h)
            _check("bs = 1 rows", _np(model._last_att), r1["post"], r1["d_post"], 4 * dim, dim)
            # teeth: one entry of the largest pair dropped
            big = int(np.argmax(cnt))
            t_big = next(t for t, s in enumerate(inp["sel"]) if s is not None and (s[0][0] == big).any())
            e_big = int(np.flatnonzero(inp["sel"][t_big][0][0] == big)[0])
            rd = _att(inp, False, drop=(t_big, e_big))
            err = np.abs(got_rows[big] - rd["post"][big]).max()
            tol = 4 * dim * EPS23 * max(1.0, float(np.abs(r["post"]).max()))
            print(f"teeth (attention, one of {int(cnt[big])} entries dropped): |got - ref_drop| {err:.3e} = "
                  f"{err / tol:.1f} x the bound, {err / OLD_ATT_TOL:.3f} x the old 5e-3")
            assert err > tol + r["d_post"][big].max()
        for k in knobs:
            setattr(model, k, _DEFAULTS[k])
    assert seen >= set(ATT_ENTRIES)
    assert not seen & set(TAIL_ENTRIES)          # (tail_precision stayed fp32)


# ------------------------------------------------------------------------------------------------- tail
@pytest.mark.parametrize("dim,mode", [(64, "all"), (128, "1-hop"), (256, "all")])
def test_bf16_tail_matches_rounded_reference(dim, mode, monkeypatch):
    """tail_precision = "bf16" behind the fp32 attention: logits against the restatement with the wB / wC images and
    every GEMM input rounded (pairs that a perm launch scores without their pairwise branch taken as it does).  At
    D = 256 the bf16 tail runs too (rows kernels).  Teeth: the same reference rounding by truncation is rejected."""
    model, score, data, tb = _setup(dim, mode, seed=3 * dim)
    reach = Reach(monkeypatch, ATT_ENTRIES + TAIL_ENTRIES)
    h = model.propagate()
    inp = _inputs(model, score, tb, h)
    bs = tb.shape[1]
    att = R.attention_ref(inp["sel"], inp["z"], inp["q"], inp["w"], inp["att_bias"], *inp["ln"], bs)
    feats = R.count_features(att["counts"], model.count_dim)
    lite = _lite(att["counts"], bs)
    assert lite.any()
    model.tail_precision = "bf16"
    runs = {"rows_perm": (dict(attention_impl="flip"), "lpf_tail_chain_rows_perm_bf16", lite),
            "rows": (dict(attention_impl="flip", tail_skip_empty=False), "lpf_tail_chain_rows_bf16", None)}
    if dim <= 128:
        runs["merge"] = (dict(attention_impl="flip", attention_rows=False), "lpf_tail_chain_merge_bf16", None)
    seen = set()
    for name, (knobs, entry, lt) in runs.items():
        for k, v in knobs.items():
            setattr(model, k, v)
        lg, ran = reach.ran(lambda: model.score_pairs(tb, h, score, logits=True))
        assert entry in ran and model.check_selection(), (name, ran)
        seen |= ran
        ref = R.tail_ref(att["post"], feats, inp["r_e"], inp["tabs"], round_act=True, round_w=True, lite=lt)
        frac = ref["n_flag"] / ref["n_elem"]
        print(f"tail {name}: flagged fraction {frac:.2e}")
        assert frac < FLAG_FRACTION
        got = _np(lg)
        _check(f"tail {name}", got, ref["logit"], ref["d_logit"], 16 * dim, dim)
        if name == "rows_perm":
            tr = R.tail_ref(att["post"], feats, inp["r_e"], inp["tabs"], round_act=True, round_w=True, lite=lt,
                            rounder=R.trunc_bf16)
            scale = max(1.0, float(np.abs(ref["logit"]).max()))
            tol = 16 * dim * EPS23 * scale + ref["d_logit"]
            gap = np.abs(got - tr["logit"])
            out = gap > tol
            print(f"teeth (tail, truncation): max |got - ref_trunc| {gap.max():.3e} = {(gap / tol).max():.1f} x the "
                  f"bound, {gap.max() / OLD_ATT_TOL:.3f} x the old 5e-3; {out.mean():.1%} of logits outside")
            assert out.any()
        for k in knobs:
            setattr(model, k, _DEFAULTS[k])
    assert seen & set(TAIL_ENTRIES) == {e for _, e, _ in runs.values()}
    assert not seen & set(ATT_ENTRIES)           # (precision stayed fp32)


# ------------------------------------------------------------------------------------------------- encoder
def _enc_ref(model, dup_part=None, x=None):
    enc = model.node_encoder.gnn_encoder
    a_hat = model._device_graph("prop", model._data_obj("adj", False))
    layers = [(c.lin.weight, c.bias, None if enc.lns is None else enc.lns[i].weight,
               None if enc.lns is None else enc.lns[i].bias) for i, c in enumerate(enc.convs)]
    layers = [tuple(None if t is None else _np(t) for t in l) for l in layers]
    x = _np(model._features()) if x is None else x
    return R.encoder_ref(x, a_hat.rowptr.cpu().numpy(), a_hat.col.cpu().numpy(), a_hat.val.cpu().numpy(), layers,
                         residual=enc.residual, relu=enc.relu, final_ln=(_np(model.gnn_norm.weight),
                                                                         _np(model.gnn_norm.bias)),
                         round_x=True, dup_part=dup_part), a_hat


@pytest.mark.parametrize("dim,layers,residual,weighted", [(64, 1, False, True), (64, 2, True, False),
                                                          (128, 3, True, True), (128, 2, False, False)])
def test_bf16_encoder_matches_rounded_reference(dim, layers, residual, weighted, monkeypatch):
    """encoder_precision = "bf16", every layer fused (f_in = D): node embeddings against the restatement that gathers
    the bf16 image of each layer input (2 and 3 layers: the image the previous layer wrote, out_bf16p).  Teeth: the
    same reference with one part of the largest hub row added twice (first or last layer) is rejected for that row."""
    model, score, data, tb = _setup(dim, "all", seed=dim + layers, layers=layers, residual=residual,
                                    weighted=weighted, f_in=dim)
    reach = Reach(monkeypatch, ENC_ENTRIES)
    model.encoder_precision = "bf16"
    got, ran = reach.ran(lambda: _np(model.propagate()))
    assert ran == set(ENC_ENTRIES) and reach.calls["lpf_gcn_layer_fused_bf16"] == layers
    ref, a_hat = _enc_ref(model)
    if layers > 1:
        frac = ref["n_flag"] / ref["n_elem"]
        print(f"encoder: flagged fraction {frac:.2e}")
        assert frac < FLAG_FRACTION
    _check(f"encoder L = {layers}", got, ref["out"], ref["d_out"], 4 * dim * layers, dim)
    rp = a_hat.rowptr.cpu().numpy()
    hub = int(np.argmax(np.diff(rp)))
    assert rp[hub + 1] - rp[hub] > 256
    tol = 4 * dim * layers * EPS23 * max(1.0, float(np.abs(ref["out"]).max())) + ref["d_out"][hub]
    ratios = []
    for layer in sorted({0, layers - 1}):      # (first layer: the residual carries it; last: straight into the row)
        rd, _ = _enc_ref(model, dup_part=(layer, hub, int(rp[hub]), int(rp[hub]) + 256))
        err = np.abs(got[hub] - rd["out"][hub])
        ratios.append(float((err / tol).max()))
        print(f"teeth (encoder, hub part of layer {layer} added twice): |got - ref_dup| {err.max():.3e} = "
              f"{ratios[-1]:.1f} x the bound, {err.max() / OLD_ENC_TOL:.3f} x the old 3e-2")
    assert max(ratios) > 1.0


# ------------------------------------------------------------------------------------------------- freshness
def test_bf16_modes_follow_in_place_updates(monkeypatch):
    """In-place updates of lin_r, one PE MLP, pairwise_lin, the score head and a node-feature Parameter (ddi-style x)
    reach the bf16 images (wfold_packed_bf16, wB / wC bf16, the bf16 Z copy, the permuted feature image): the bf16
    modes match the restatement built from the new values and not the one built from the old."""
    dim = 128
    model, score, data, tb = _setup(dim, "all", seed=5, layers=2, residual=True, f_in=dim)
    model.data["x"] = torch.nn.Parameter(model.data["x"].to(DEV).clone(), requires_grad=False)
    reach = Reach(monkeypatch, ATT_ENTRIES + TAIL_ENTRIES + ENC_ENTRIES)

    def run_all():
        model.encoder_precision = "bf16"
        model.precision = model.tail_precision = "f32"
        h16 = _np(model.propagate())
        model.encoder_precision = "f32"
        h = model.propagate()
        model.precision = model.tail_precision = "bf16"
        model.attention_impl = "flip"
        lg = _np(model.score_pairs(tb, h, score, logits=True))
        model.attention_impl = "mfma"
        lgm = _np(model.score_pairs(tb, h, score, logits=True))
        model.precision = model.tail_precision = "f32"
        model.attention_impl = "auto"
        return h16, h, lg, lgm

    def refs(h):
        inp = _inputs(model, score, tb, h)
        out = []
        for fused in (False, True):
            a = _att(inp, fused)
            lt = _lite(a["counts"], tb.shape[1]) if not fused else None
            out.append(R.tail_ref(a["post"], R.count_features(a["counts"], model.count_dim), inp["r_e"], inp["tabs"],
                                  round_act=True, round_w=True, lite=lt, d_rows=a["d_post"]))
        return out, _enc_ref(model)[0]

    h16, h, lg, lgm = run_all()
    (old_f, old_m), old_e = refs(h)
    _check("fresh: logits before (flip)", lg, old_f["logit"], old_f["d_logit"], 16 * dim, dim)
    with torch.no_grad():
        g = torch.Generator(device="cpu").manual_seed(9)
        for p in (model.att_layers[0].att.lin_r.weight, model.ppr_encoder_onehop.linears[0].weight,
                  model.pairwise_lin.linears[0].weight, score.lins[0].weight, model.data["x"]):
            p.mul_(1.0 + 0.05 * torch.randn(p.shape, generator=g).to(p.device))
    h16n, hn, lgn, lgmn = run_all()
    (new_f, new_m), new_e = refs(hn)
    assert {"lpf_pair_attention_rows4_zbf16", "lpf_pair_attention_fused_bf16", "lpf_tail_chain_rows_perm_bf16",
            "lpf_tail_chain_merge_bf16", "lpf_gcn_layer_fused_bf16"} <= set(reach.calls)
    for name, got, new, old, c in (("flip logits", lgn, new_f["logit"], old_f["logit"], 16 * dim),
                                   ("mfma logits", lgmn, new_m["logit"], old_m["logit"], 16 * dim),
                                   ("encoder", h16n, new_e["out"], old_e["out"], 8 * dim)):
        bound = {"flip logits": new_f["d_logit"], "mfma logits": new_m["d_logit"], "encoder": new_e["d_out"]}[name]
        _check(f"fresh: {name}", got, new, bound, c, dim)
        scale = max(1.0, float(np.abs(new).max()))
        assert (np.abs(got - old) > c * EPS23 * scale + bound).any(), f"{name} still matches the old values"
