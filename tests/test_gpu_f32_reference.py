"""The fp32 scoring kernels against the fp64 restatement (tests/bf16_reference.py, every rounding switch off) within
the per-pair, per-feature error model of tests/f32_error_model.py -- at random-init scores (att_gain = 1) and at a wide
gain that stretches the widest pair's score range to 80 units, where the online-softmax rescales do real work.

Reach map -- entry point: knobs that select it (every D of 32, 64, 128, 256 unless noted):
  lpf_pair_attention_rows4_f32       attention_impl "flip" (select4); calc_pairwise and score_pairs       ["rows4"]
  lpf_pair_attention_rows_f32        "flip", use_select_index = False; calc_pairwise, and score_pairs with
                                     tail_skip_empty = False                                    ["rows", "rows_perm"]
  lpf_pair_attention_rows_perm_f32   "flip", use_select_index = False, score_pairs                       ["rows_perm"]
  lpf_pair_attention_flip_f32        "flip", attention_rows = False (+ lpf_pair_attention_merge_f32)      ["flip"]
  lpf_pair_attention_fused_f32       attention_impl "mfma" (+ the merge)                                   ["mfma"]
  lpf_tail_chain_rows_perm_f32       score_pairs of "rows4" and "rows_perm"
  lpf_tail_chain_rows_f32            score_pairs of "rows"; of "flip" and "mfma" at D = 256
  lpf_tail_chain_merge_f32           score_pairs of "flip" and "mfma" at D <= 128
  lpf_tail_chain_f32                 use_fused_attention = False, D <= 128 (behind lpf_pair_scores_f32 +
                                     lpf_pair_softmax_gather_f32: family "gather")                         ["chain"]
  lpf_gcn_layer_fused_f32            square encoder layers, D in 32, 64, 128 (no D = 256 instantiation: that case runs
  lpf_spmm_row_parts_f32             transform + aggregate and is held to the same bound)

Bounds (f32_error_model, u = 2^-23): rows |got - ref| <= C_ATT[family] b_post;  logits <= C_TAIL s_l, the rows' bound
(at its family's C_ATT) and the tail's own roundings carried in quadrature;  encoder <= C_ENC bound.  b_post and s_l add
independent rounding errors in quadrature where the worst case adds magnitudes; both are asserted to lie below their
worst-case forms (b_post_worst; the rows' bound carried through tail_ref's d_logit), which are 1.3 ... 10 x 1e-5 scale
for a benign row and 1e-3 ... 1e-1 for a logit -- wider than the 1e-4 they were to supersede.  Every check prints
err / bound at C = 1.  The constants are 4 x the worst ratio measured on an MI355X over every case below with three
seeds (the case's own seed, + 1000, + 2000), rounded up to a power of two:

  worst err / bound(C = 1)      D = 32          D = 64          D = 128         D = 256
  rows  (rows4, rows, _perm)    0.880 -> 4      0.595 -> 4      0.536 -> 4      0.490 -> 2
  flip + merge                  0.780 -> 4      0.588 -> 4      0.536 -> 4      0.573 -> 4
  matrix core + merge           0.780 -> 4      0.608 -> 4      0.655 -> 4      0.580 -> 4
  gather (module by module)     0.540 -> 4      0.927 -> 4      0.795 -> 4      --
  tails (the four, logits)      0.380 -> 2      0.417 -> 2      0.361 -> 2      0.415 -> 2
  encoder                       0.022 -> 2^-3   0.157 -> 1      0.005 -> 2^-5   0.010 -> 2^-4

Rows without entries, with one entry and with hundreds sit at the same 0.3 ... 0.9 at both gains, and so do the logits:
the model has the right shape (at the wide gain the rows' errors grow five-fold, to 1.3e-6 scale, and the bound with
them).  The matrix-core kernel (v_mfma_f32_32x32x2_f32: fp32 products) behaves like the other families.  The encoder's
small ratios say that its bound, which adds magnitudes in the worst case over hub rows of 700 entries, is far from the
kernel's error; its constants take that slack back as far as one constant can.
"""
import collections

import numpy as np
import pytest

from tests import bf16_reference as R
from tests import f32_error_model as E
from tests.scoring_harness import Reach, _DEFAULTS, _inputs, _np, _setup, knobs

pytestmark = pytest.mark.gpu

_W = (32, 64, 128, 256)
C_ATT = {"rows": dict(zip(_W, (4.0, 4.0, 4.0, 2.0))), "flip": dict(zip(_W, (4.0, 4.0, 4.0, 4.0))),
         "mfma": dict(zip(_W, (4.0, 4.0, 4.0, 4.0))), "gather": dict(zip(_W, (4.0, 4.0, 4.0)))}
C_TAIL = dict(zip(_W, (2.0, 2.0, 2.0, 2.0)))
C_ENC = dict(zip(_W, (2.0 ** -3, 1.0, 2.0 ** -5, 2.0 ** -4)))

WIDE_RANGE = 80.0            # the widest pair's score range at the wide gain: exp(+-80) is finite (and normal) in fp32
OLD_TOL = 1e-4               # x max(1, max|ref|): what the fp32 path was held to before
BENIGN_SD, BENIGN_TOL = 0.25, 1e-5

ATT_ENTRIES = tuple("lpf_pair_attention_" + s + "_f32" for s in ("rows4", "rows", "rows_perm", "flip", "fused"))
TAIL_ENTRIES = ("lpf_tail_chain_f32", "lpf_tail_chain_rows_f32", "lpf_tail_chain_rows_perm_f32",
                "lpf_tail_chain_merge_f32")
ENC_ENTRIES = ("lpf_gcn_layer_fused_f32", "lpf_spmm_row_parts_f32")
GATHER_ENTRIES = ("lpf_pair_scores_f32", "lpf_pair_softmax_gather_f32")
BF16_ENTRIES = ("lpf_pair_attention_rows4_zbf16", "lpf_pair_attention_rows_zbf16", "lpf_pair_attention_rows_perm_zbf16",
                "lpf_pair_attention_flip_zbf16", "lpf_pair_attention_fused_bf16", "lpf_tail_chain_rows_bf16",
                "lpf_tail_chain_rows_perm_bf16", "lpf_tail_chain_merge_bf16", "lpf_gcn_layer_fused_bf16",
                "lpf_spmm_row_parts_bf16p")
WATCHED = ATT_ENTRIES + TAIL_ENTRIES + GATHER_ENTRIES + BF16_ENTRIES

FAMILY = {"rows4": "rows", "rows": "rows", "rows_perm": "rows", "flip": "flip", "mfma": "mfma", "chain": "gather"}
KNOBS = dict(knobs("f32"))
KNOBS["chain"] = (dict(use_fused_attention=False), "lpf_pair_softmax_gather_f32", {"lpf_tail_chain_f32"})
CASES = [(32, "all"), (64, "all"), (128, "all"), (256, "all"), (128, "1-hop"), (64, "cn")]

RATIOS = collections.defaultdict(list)      # (family, D) -> ratios at C = 1, in the order measured
TAIL_LOG = []                               # (knob, D, wide, err, rows' bound carried at C = 1, own) per logits check
_seen = set()
_cases = {}


def _tail_entry(name, dim):
    if name in ("rows4", "rows_perm"):
        return "lpf_tail_chain_rows_perm_f32"
    if name == "rows" or (name in ("flip", "mfma") and dim == 256):
        return "lpf_tail_chain_rows_f32"
    return "lpf_tail_chain_f32" if name == "chain" else "lpf_tail_chain_merge_f32"


def _reference(model, score, tb, h):
    """fp64 rows and logits of one batch with their C = 1 bounds (arrays read-only)."""
    inp = _inputs(model, score, tb, h)
    bs = inp["bs"]
    ref = E.attention(inp["sel"], inp["z"], inp["q"], inp["w"], inp["att_bias"], *inp["ln"], bs)
    bnd = E.attention_bound(ref, inp["z"], inp["w"], inp["q"], inp["att_bias"], *inp["ln"])
    feats = R.count_features(ref["counts"], model.count_dim)
    ew = model.elementwise_lin
    b_re = E.elementwise_bound(_np(h), tb.cpu().numpy(), *(_np(p) for p in (
        ew.linears[0].weight, ew.linears[0].bias, ew.norm.weight, ew.norm.bias)))
    carried, own, logit = E.tail_bound(ref["post"], feats, inp["r_e"], inp["tabs"], bnd["b_post"], b_re)
    tail = (ref["post"], feats, inp["r_e"], inp["tabs"])
    s_rows = E.tail_sigma(*tail, bnd["b_post"], np.zeros_like(b_re), own=False)
    s_own = E.tail_sigma(*tail, np.zeros_like(bnd["b_post"]), b_re)
    assert (bnd["b_post"] <= bnd["b_post_worst"]).all()
    out = {"inp": inp, "ref": ref, "bnd": bnd, "feats": feats, "b_re": b_re, "carried": carried, "own": own,
           "s_rows": s_rows, "s_own": s_own, "logit": logit, "range": E.score_ranges(ref, bs)}
    for a in (ref["post"], ref["pre"], bnd["b_post"], carried, own, s_rows, s_own, logit):
        a.setflags(write=False)
    return out


def _case(dim, mode, wide, seed_shift=0):
    """Model, batch, fp64 reference and bounds of one (dim, mode, gain), built once and left unchanged.  The wide gain
    is WIDE_RANGE / (the widest pair's score range of the same case at gain 1): scores are linear in ``att``."""
    key = (dim, mode, wide, seed_shift)
    if key not in _cases:
        seed = dim + len(mode) + seed_shift
        gain = 1.0
        if wide:
            gain = WIDE_RANGE / float(_case(dim, mode, False, seed_shift)["range"].max())
        model, score, data, tb = _setup(dim, mode, seed=seed, att_gain=gain)
        h = model.propagate()
        c = {"model": model, "score": score, "tb": tb, "h": h, "gain": gain, "dim": dim}
        c.update(_reference(model, score, tb, h))
        one = tb[:, :1].contiguous()                       # the hub pair alone
        c["one"] = dict(_reference(model, score, one, h), tb=one)
        _cases[key] = c
    return _cases[key]


def _ratio(name, fam, dim, got, ref, bound, c):
    """Assert |got - ref| <= c bound elementwise; prints and records the worst ratio at C = 1."""
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / bound).max())
    RATIOS[(fam, dim)].append(worst)
    print(f"{name}: max |got - ref| {err.max():.3e}, worst err / bound(C = 1) {worst:.3f}, / bound(C = {c:g}) "
          f"{worst / c:.3f} (D = {dim})")
    assert np.isfinite(got).all() and worst <= c, f"{name}: {err.max():.3e} beyond the bound ({worst:.2f} > {c:g})"
    return worst


def _logit_bound(ref, fam, dim, c_tail):
    """c_tail s_l with the rows at their family's constant -- and never above the worst-case carry."""
    bound = c_tail * np.sqrt((C_ATT[fam][dim] * ref["s_rows"]) ** 2 + ref["s_own"] ** 2)
    assert (bound <= C_ATT[fam][dim] * ref["carried"] + ref["own"]).all()
    return bound


def _logits(name, knob, dim, wide, got, ref, fam):
    err = np.abs(got.astype(np.float64) - ref["logit"])
    worst = float((err / _logit_bound(ref, fam, dim, 1.0)).max())
    RATIOS[("tail", dim)].append(worst)
    TAIL_LOG.append((knob, fam, dim, wide, err, np.array(ref["s_rows"]), np.array(ref["s_own"])))
    print(f"{name}: max |got - ref| {err.max():.3e}, worst err / bound(C_TAIL = 1) {worst:.3f}, / bound(C_TAIL = "
          f"{C_TAIL[dim]:g}) {worst / C_TAIL[dim]:.3f} (D = {dim}, rows' share at C_ATT = {C_ATT[fam][dim]:g})")
    assert np.isfinite(got).all() and worst <= C_TAIL[dim], f"{name}: {err.max():.3e} beyond the bound"


def _set(model, settings):
    for k, v in settings.items():
        setattr(model, k, v)


def _run_knob(c, name, reach):
    """calc_pairwise rows and score_pairs logits of one knob set (model left at its defaults): (rows, logits, ran)."""
    model, tb, h, score = c["model"], c["tb"], c["h"], c["score"]
    settings, cp_entry, sp_entries = KNOBS[name]
    _set(model, settings)
    try:
        _, ran = reach.ran(lambda: model.calc_pairwise(tb, h))
        rows = _np(model._last_att).copy()
        assert cp_entry in ran and model.check_selection(), (name, ran)
        lg, ran2 = reach.ran(lambda: model.score_pairs(tb, h, score, logits=True))
        assert sp_entries <= ran2 and _tail_entry(name, c["dim"]) in ran2 and model.check_selection(), (name, ran2)
        one = c["one"]["tb"]
        model.calc_pairwise(one, h)
        rows1 = _np(model._last_att).copy()
        lg1 = _np(model.score_pairs(one, h, score, logits=True))
        assert model.check_selection()
    finally:
        _set(model, {k: _DEFAULTS[k] for k in settings})
    return rows, _np(lg), rows1, lg1, ran | ran2


def _knob_names(dim):
    return [k for k in KNOBS if not (k == "chain" and dim == 256)]   # (no lpf_tail_chain_f32 at D = 256)


def run_attention_case(dim, mode, wide, monkeypatch, seed_shift=0):
    """Every knob set of one case against the reference; returns the entry points seen."""
    c = _case(dim, mode, wide, seed_shift)
    ref, bnd, rng_ = c["ref"], c["bnd"], c["range"]
    cnt = ref["counts"].sum(axis=1)
    bs = c["tb"].shape[1]
    assert cnt.max() > (512 if mode != "cn" else 96) and (cnt == 0).sum() > 64 and (cnt == 1).any() and bs % 64
    nonempty = cnt > 0
    print(f"D = {dim}, {mode}, gain {c['gain']:.3f}: score range of the hub pair {rng_[0]:.2f}, widest {rng_.max():.2f}, "
          f"share of non-empty pairs with range >= 10: {(rng_[nonempty] >= 10).mean():.3f}; "
          f"{int(cnt.sum())} entries, largest pair {int(cnt.max())}")
    reach = Reach(monkeypatch, WATCHED)
    seen = set()
    tag = f"[{dim} {mode} {'wide' if wide else 'gain 1'}]"
    for name in _knob_names(dim):
        fam = FAMILY[name]
        rows, lg, rows1, lg1, ran = _run_knob(c, name, reach)
        seen |= ran
        _ratio(f"{tag} {name} rows", fam, dim, rows, ref["post"], bnd["b_post"], C_ATT[fam][dim])
        _logits(f"{tag} {name} logits", name, dim, wide, lg, c, fam)
        _ratio(f"{tag} {name} rows, bs = 1", fam, dim, rows1, c["one"]["ref"]["post"], c["one"]["bnd"]["b_post"],
               C_ATT[fam][dim])
        _logits(f"{tag} {name} logit, bs = 1", name, dim, wide, lg1, c["one"], fam)
    assert not seen & set(BF16_ENTRIES), seen
    if wide:    # the wide gain did its work: the conditions on the reference's score ranges
        assert rng_[0] >= 30 and (rng_[nonempty] >= 10).mean() >= 0.25
        top = np.float32(rng_.max())
        assert np.isfinite(np.exp(top)) and np.exp(-top) > 0
    _seen.update(seen)
    return seen


@pytest.mark.parametrize("wide", [False, True], ids=["gain1", "wide"])
@pytest.mark.parametrize("dim,mode", CASES)
def test_f32_attention_and_logits_match_fp64(dim, mode, wide, monkeypatch):
    """Post-norm rows (calc_pairwise) and logits (score_pairs) of every fp32 attention kernel and the tail behind it,
    on the whole batch and on the hub pair alone, within the error model; the named _f32 entry point ran and no bf16
    one did."""
    seen = run_attention_case(dim, mode, wide, monkeypatch)
    want = set(ATT_ENTRIES) | {_tail_entry(k, dim) for k in _knob_names(dim)}
    assert seen >= want, want - seen


# ------------------------------------------------------------------------------------------------- teeth
def _post_effect(c):
    """Post-norm move of every entry's row when that entry is lost (closed form, fp64): [E, D]."""
    ref, inp = c["ref"], c["inp"]
    eff = E.drop_effect(ref, inp["att_bias"])
    ok = np.isfinite(eff).all(axis=1) & (ref["ent"]["alpha"] < 0.5)
    g, b = (np.asarray(a, np.float64) for a in inp["ln"])
    moved = R.layer_norm(ref["pre"][ref["ent"]["pair"]] + np.where(ok[:, None], eff, 0.0), g, b)[0]
    return np.abs(moved - ref["post"][ref["ent"]["pair"]]), ok


TEETH_CASES = [(32, False), (64, False), (128, False), (256, False), (128, True)]
_inside_old = {}            # (dim, wide) -> the old tolerance accepted near-miss (a) or (b) from every entry point


@pytest.mark.parametrize("dim,wide", TEETH_CASES)
def test_f32_teeth_near_miss_references_are_rejected(dim, wide, monkeypatch):
    """(a) the reference without ONE entry -- the one whose loss moves its row least while still 8 x that row's bound
    (entries with alpha < 1/2: the closed form is well conditioned there) -- and (b) the reference with eps = 0 in
    post_att_norm are rejected for every entry point.  Whether the old 1e-4 max(1, max|ref|) accepted one of them is
    recorded for test_f32_entry_points_all_reached (at D = 256 the smallest loss worth 8 bounds is 1.7 x the old
    tolerance; at the other widths 0.1 ... 0.8 x)."""
    run_teeth(dim, wide, monkeypatch)


def run_teeth(dim, wide, monkeypatch):
    c = _case(dim, "all", wide)
    ref, bnd, inp = c["ref"], c["bnd"], c["inp"]
    ent = ref["ent"]
    c_max = max(C_ATT[FAMILY[k]][dim] for k in _knob_names(dim))
    effect, ok = _post_effect(c)
    margin = (effect / (c_max * bnd["b_post"][ent["pair"]])).max(axis=1)
    cand = np.flatnonzero(ok & (margin >= 8.0))
    assert cand.size
    e = int(cand[np.argmin(effect[cand].max(axis=1))])
    p, t = int(ent["pair"][e]), int(ent["type"][e])
    ofs = np.cumsum([0] + [0 if s is None else s[0].shape[1] for s in inp["sel"]])
    args = (inp["sel"], inp["z"], inp["q"], inp["w"], inp["att_bias"], *inp["ln"], inp["bs"])
    rd = E.attention(*args, drop=(t, e - int(ofs[t])))
    assert np.abs(np.abs(rd["post"][p] - ref["post"][p]) - effect[e]).max() <= 1e-9      # (the closed form)
    scale = max(1.0, float(np.abs(ref["post"]).max()))
    print(f"teeth (a): entry {e} of pair {p} ({int(ref['counts'][p].sum())} entries, alpha {ent['alpha'][e]:.2e}) lost: "
          f"row moves by {effect[e].max():.3e} = {margin[e]:.1f} x its bound = {effect[e].max() / (OLD_TOL * scale):.4f} "
          f"x the old 1e-4 scale")
    r0 = E.attention(*args, ln_eps=0.0)
    reach = Reach(monkeypatch, WATCHED)
    inside_old = []
    for name in _knob_names(dim):
        fam = FAMILY[name]
        rows, lg, _, _, _ = _run_knob(c, name, reach)
        # (a)
        gap = np.abs(rows[p] - rd["post"][p])
        out_a = float((gap / (C_ATT[fam][dim] * bnd["b_post"][p])).max())
        # (b) post_att_norm without its epsilon: some row outside
        gap0 = np.abs(rows - r0["post"])
        out_b = float((gap0 / (C_ATT[fam][dim] * bnd["b_post"])).max())
        whole_a = np.abs(rows - rd["post"]).max()
        print(f"teeth {name}: (a) {out_a:.1f} x the bound, max gap {whole_a / (OLD_TOL * scale):.4f} x old; (b) eps = 0 in "
              f"post_att_norm {out_b:.1f} x, max gap {gap0.max() / (OLD_TOL * scale):.3f} x old")
        assert out_a > 1.0 and out_b > 1.0, (name, out_a, out_b)
        inside_old.append(whole_a <= OLD_TOL * scale or gap0.max() <= OLD_TOL * scale)
    _inside_old[(dim, wide)] = all(inside_old)


def test_f32_teeth_tail_norm_epsilon_is_rejected(monkeypatch):
    """(b), tail: the reference with eps = 0 in the tail's LN_B must lie outside the logit bound of every entry point
    on at least one logit, at every D.

    eps = 0 in LN_B moves the logits by 1.5e-6 ... 2.5e-6 at most, the kernels' own logit error is about 1e-7: only
    the quadrature carry of the logit bound can tell them apart (the worst-case carry is 1e-3 ... 1e-1)."""
    reach = Reach(monkeypatch, WATCHED)
    worst = {}
    for dim in _W:
        c = _case(dim, "all", False)
        t0 = R.tail_ref(c["ref"]["post"], c["feats"], c["inp"]["r_e"], c["inp"]["tabs"], ln_eps=0.0)
        lscale = max(1.0, float(np.abs(c["logit"]).max()))
        for name in _knob_names(dim):
            fam = FAMILY[name]
            _, lg, _, _, _ = _run_knob(c, name, reach)
            gap = np.abs(lg - t0["logit"])
            bound = _logit_bound(c, fam, dim, C_TAIL[dim])
            worst[(dim, name)] = float((gap / bound).max())
            print(f"teeth (tail, eps = 0 in LN_B) D = {dim} {name}: max gap {gap.max():.3e} = {worst[(dim, name)]:.4f} x "
                  f"the bound (largest bound {bound.max():.3e}, median {np.median(bound):.3e}), "
                  f"{gap.max() / (OLD_TOL * lscale):.4f} x the old 1e-4 scale")
    inside = {k: v for k, v in worst.items() if v <= 1.0}
    assert not inside, f"eps = 0 in LN_B is inside the logit bound: {inside}"


def test_f32_benign_bound_is_a_tenth_of_the_old_tolerance():
    """Condition on the bound itself: with the chosen constants, the asserted bound of every benign row (att_gain = 1,
    row standard deviation >= 0.25) is below 1e-5 max(1, max|ref|), a tenth of the tolerance it supersedes, at every D.

    With the score-sensitivity term in its worst-case form (b_post_worst) this does not hold in any family: the largest
    benign bound is then 0.7 (D = 32) to 2.6 (D = 256) x 1e-5 scale at C = 1 already, because that form adds D magnitudes
    per score and then the entries' magnitudes, while C is set by rows without the term."""
    fails = []
    for dim, mode in CASES:
        c = _case(dim, mode, False)
        ref, bnd = c["ref"], c["bnd"]
        scale = max(1.0, float(np.abs(ref["post"]).max()))
        benign = bnd["sd"] >= BENIGN_SD
        assert benign.sum() > 200
        for fam in ("rows", "flip", "mfma"):
            top = C_ATT[fam][dim] * float(bnd["b_post"][benign].max())
            print(f"[{dim} {mode}] {fam}: largest bound of a benign row {top:.3e} = {top / (BENIGN_TOL * scale):.3f} x 1e-5 "
                  f"scale (C = {C_ATT[fam][dim]:g}, {int(benign.sum())} rows benign; median row "
                  f"{C_ATT[fam][dim] * float(np.median(bnd['b_post'][benign].max(axis=1))) / (BENIGN_TOL * scale):.3f})")
            if not top < BENIGN_TOL * scale:
                fails.append((dim, mode, fam, round(top / (BENIGN_TOL * scale), 2)))
    assert not fails, f"benign bound above 1e-5 scale: {fails}"


# ------------------------------------------------------------------------------------------------- encoder
def _enc_ref(model, dup_part=None):
    enc = model.node_encoder.gnn_encoder
    a_hat = model._device_graph("prop", model._data_obj("adj", False))
    layers = [(c.lin.weight, c.bias, None if enc.lns is None else enc.lns[i].weight,
               None if enc.lns is None else enc.lns[i].bias) for i, c in enumerate(enc.convs)]
    layers = [tuple(None if t is None else _np(t) for t in l) for l in layers]
    out, bound = E.encoder_bound(_np(model._features()), a_hat.rowptr.cpu().numpy(), a_hat.col.cpu().numpy(),
                                 a_hat.val.cpu().numpy(), layers, residual=enc.residual, relu=enc.relu,
                                 final_ln=(_np(model.gnn_norm.weight), _np(model.gnn_norm.bias)), dup_part=dup_part)
    return out, bound, a_hat


ENC_CASES = [(64, 1, False, True), (64, 2, True, False), (128, 3, True, True), (128, 2, False, False),
             (256, 2, True, False), (32, 2, True, True)]


def run_encoder_case(dim, layers, residual, weighted, monkeypatch, seed_shift=0):
    model, score, data, tb = _setup(dim, "all", seed=dim + layers + seed_shift, layers=layers, residual=residual,
                                    weighted=weighted, f_in=dim)
    reach = Reach(monkeypatch, ENC_ENTRIES + BF16_ENTRIES)
    got, ran = reach.ran(lambda: _np(model.propagate()))
    if dim <= 128:
        assert ran == set(ENC_ENTRIES) and reach.calls["lpf_gcn_layer_fused_f32"] == layers, (ran, reach.calls)
    else:       # (no fused layer that wide: transform + aggregate)
        assert "lpf_gcn_layer_fused_f32" not in ran and not ran & set(BF16_ENTRIES), ran
    ref, bound, a_hat = _enc_ref(model)
    _ratio(f"encoder D = {dim}, L = {layers}", "encoder", dim, got, ref, bound, C_ENC[dim])
    scale = max(1.0, float(np.abs(ref).max()))
    print(f"encoder: largest bound {C_ENC[dim] * bound.max():.3e} = {C_ENC[dim] * bound.max() / (BENIGN_TOL * scale):.3f} x 1e-5 "
          f"scale")
    # teeth: ONE entry of the largest hub row counted twice (first or last layer) is rejected for that row
    rp = a_hat.rowptr.cpu().numpy()
    hub = int(np.argmax(np.diff(rp)))
    assert rp[hub + 1] - rp[hub] > 256
    worst = []
    for layer in sorted({0, layers - 1}):
        rd, _, _ = _enc_ref(model, dup_part=(layer, hub, int(rp[hub]), int(rp[hub]) + 1))
        gap = np.abs(got[hub] - rd[hub])
        worst.append(float((gap / (C_ENC[dim] * bound[hub])).max()))
        print(f"teeth (encoder, one of {int(rp[hub + 1] - rp[hub])} entries of the hub row added twice in layer {layer}): "
              f"{worst[-1]:.1f} x the bound, {gap.max() / (OLD_TOL * scale):.3f} x the old 1e-4 scale")
    assert max(worst) > 1.0
    _seen.update(ran)
    return ran


@pytest.mark.parametrize("dim,layers,residual,weighted", ENC_CASES)
def test_f32_encoder_matches_fp64(dim, layers, residual, weighted, monkeypatch):
    """model.propagate() against the fp64 encoder within the encoder bound; one launch of the fused layer per layer
    and the hub rows' part sums (D <= 128)."""
    run_encoder_case(dim, layers, residual, weighted, monkeypatch)


# ------------------------------------------------------------------------------------------------- coverage
def test_f32_entry_points_all_reached(monkeypatch):
    """The union of the entry points the tests of this module saw covers the nine fp32 attention and tail entry points
    and the two of the encoder, and the old tolerance accepted at least one of the near-misses the teeth test rejects.
    (Run on its own, it runs one D = 64 case of each kind first.)"""
    if not _seen & set(ATT_ENTRIES):
        run_attention_case(64, "all", False, monkeypatch)
    if not _seen & set(ENC_ENTRIES):
        run_encoder_case(64, 1, False, True, monkeypatch)
    if not _inside_old:
        run_teeth(64, False, monkeypatch)
    # a near-miss that every entry point now rejects sat inside the old 1e-4 max(1, max|ref|): the gap is closed
    print(f"near-miss inside the old tolerance: {_inside_old}")
    assert any(_inside_old.values())
    missing = (set(ATT_ENTRIES) | set(TAIL_ENTRIES) | set(ENC_ENTRIES)) - _seen
    assert not missing, missing
    assert not _seen & set(BF16_ENTRIES)
