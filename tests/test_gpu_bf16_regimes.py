"""The bf16 scoring kernels at wide gains and at trained-like parameters, held to the per-row error model of the fp32
kernels (tests/f32_error_model.py) on the restatement with each kernel's roundings on (tests/bf16_reference.py).

Harness of tests/scoring_harness.py as it is (n = 2000, bs = 700: hub pair above 512 entries, > 64 empty pairs, a == b
pairs, duplicates); one case per key, built once.  D = 32 goes through the model: ``precision = "bf16"`` is not refused
at any D, the launchers have D = 32 instantiations.

Bounds (C_ATT, C_TAIL of test_gpu_f32_reference, C_H of test_gpu_param_regimes, imported, not re-fitted: a bf16 kernel
does the fp32 arithmetic on rounded inputs, a bf16 x bf16 product is exact in the fp32 accumulator):
  rows    |got - ref16| <= C_ATT[family][D] b_post(ref16) + C_H[D] b_post_h(ref16) + d_post
          ref16: Z rounded (a torch cast of the model's own fp32 table; the reference rounds that table), for the
          matrix-core kernel also the Wfold image and h_e; K_e of b_post from the rounded Z / Wfold / h_e; d_post the
          flip bound of the h_e elements within their fp32 error of a rounding midpoint (valid for any score change:
          bf16_reference.attention_ref), b_post_h the conditioning of the closed-form PE variance (regimes only).
  logits  fp32 tail: C_TAIL[D] s_l (rows at the bound above and the tail's own roundings, in quadrature) + d_logit, the
          flip bound carried through the tail.  bf16 tail: the same on tail_ref(round_act, round_w, lite, d_rows = the
          rows' bound), whose d_logit charges every activation that the rows' bound may tip over a midpoint.

Tests:
  a  attention, gain 1 and wide (the gain that stretches the widest pair of the rounded reference to 80 units):
     D 32 / 64 / 128 / 256 "all", (128, "1-hop"), (64, "cn") x the five knob sets; batch and hub pair alone (bs = 1)
  b  attention at the six regimes of tests/param_regimes.py: D 64, 128 x five knobs, D 32, 256 x rows4.  No regime loses
     its ``mfma`` knob: with the flag window widened by b_h the flagged fraction stays below 5e-3 everywhere
     (tests/test_bf16_reference_host.py::test_flagged_fraction_cap_with_the_widened_window: at most 2.9e-3, pe_diff_big;
     on the harness batch 1e-4 ... 1.0e-3)
  c  precision = tail_precision = "bf16" (what bench.py times): D 32 ... 256, gain 1 and wide; rows4, rows_perm (perm
     tail, lite pairs), rows, and flip (merge tail) at D <= 128
  d  the bf16 tail behind the fp32 attention under init, ln_offset, ln_flat: D 64, 128, the three tail entry points
  e  teeth, every (D, mode, gain) of (a) and every knob: the unrounded fp64 reference, the reference rounding by
     truncation and the reference without one entry of the largest pair must each lie outside the bound
  f  what the mode costs: max |bf16 logits - unrounded fp64 logits| per (D, gain / regime), printed next to the figure
     the reference alone predicts; 5e-3 asserted at (gain 1, init) only, where it is stated today

The reference.  The restatement evaluates the PE LayerNorm's variance from the triangular factor (rows 3-5 of pe_stat,
``attention_ref(factor=True)``), as the kernels do.  With the six moments written out (rows 0-2, the restatement's form
until now) the fp32 STORAGE of the moments alone moves h_e by 1e-4 ... 3e-4 under pe_diff_big: measured with that form,
the *_zbf16 kernels sat at 0.72 ... 0.89 of a bound that C_H b_post_h dominated, and the matrix-core kernel at D = 128
pe_diff_big at 2.9 x its bound (1.5e-3: elements of h_e rounded the other way that no window of the size of the
kernel's error could flag).  That was the reference, not a kernel.  No kernel and no host image was changed.

Measured on an AMD Instinct MI355X, worst err / bound at EVERY C = 1 over the case's seed, + 1000 and + 2000 (the
committed constants are 2 ... 4): rows per kernel family, logits behind the fp32 tail per family, logits of attention
and tail both bf16 (c; regimes: the record-only runs of f), logits of the bf16 tail behind the fp32 attention (d).

  D    case          rows    flip    mfma  |  logits  rows    flip    mfma  |  both bf16  rows    flip  |  bf16 tail  rows    flip
  32   gain 1        0.446   0.451   0.320  |          0.378   0.404   0.348  |             0.161   0.115  |                 --      --
  32   wide          0.611   0.585   0.472  |          0.381   0.381   0.446  |             0.161   0.026  |                 --      --
  32   init          0.327      --      --  |          0.366      --      --  |             0.161      --  |                 --      --
  32   pe_diff       0.327      --      --  |          0.408      --      --  |             0.161      --  |                 --      --
  32   pe_diff_big   0.327      --      --  |          0.436      --      --  |             0.161      --  |                 --      --
  32   pe_steep      0.327      --      --  |          0.442      --      --  |             0.161      --  |                 --      --
  32   ln_offset     0.304      --      --  |          0.261      --      --  |             0.147      --  |                 --      --
  32   ln_flat       0.261      --      --  |          0.398      --      --  |             0.101      --  |                 --      --
  64   gain 1        0.482   0.452   0.402  |          0.430   0.481   0.481  |             0.142   0.016  |                 --      --
  64   wide          0.538   0.590   0.485  |          0.430   0.481   0.481  |             0.142   0.023  |                 --      --
  64   init          0.269   0.269   0.269  |          0.416   0.390   0.401  |             0.142      --  |              0.142   0.006
  64   pe_diff       0.269   0.269   0.269  |          0.352   0.352   0.276  |             0.142      --  |                 --      --
  64   pe_diff_big   0.269   0.269   0.269  |          0.398   0.398   0.276  |             0.142      --  |                 --      --
  64   pe_steep      0.280   0.280   0.269  |          0.321   0.280   0.276  |             0.142      --  |                 --      --
  64   ln_offset     0.299   0.273   0.262  |          0.261   0.261   0.305  |             0.136      --  |              0.136   0.085
  64   ln_flat       0.146   0.288   0.727  |          0.444   0.444   0.321  |             0.098      --  |              0.181   0.181
  128  gain 1        0.435   0.431   0.363  |          0.474   0.474   0.396  |             0.107   0.017  |                 --      --
  128  wide          0.572   0.572   0.446  |          0.534   0.486   0.396  |             0.107   0.004  |                 --      --
  128  init          0.363   0.363   0.363  |          0.397   0.397   0.335  |             0.107      --  |              0.107   0.002
  128  pe_diff       0.363   0.363   0.363  |          0.475   0.335   0.335  |             0.107      --  |                 --      --
  128  pe_diff_big   0.363   0.363   0.363  |          0.351   0.335   0.335  |             0.107      --  |                 --      --
  128  pe_steep      0.363   0.363   0.699  |          0.351   0.335   0.335  |             0.107      --  |                 --      --
  128  ln_offset     0.280   0.273   0.255  |          0.290   0.306   0.257  |             0.054      --  |              0.054   0.017
  128  ln_flat       0.138   0.202   0.724  |          0.396   0.396   0.368  |             0.086      --  |              0.086   0.025
  256  gain 1        0.489   0.535   0.371  |          0.467   0.467   0.284  |             0.102      --  |                 --      --
  256  wide          0.489   0.535   0.734  |          0.413   0.399   0.369  |             0.102      --  |                 --      --
  256  init          0.351      --      --  |          0.465      --      --  |             0.102      --  |                 --      --
  256  pe_diff       0.351      --      --  |          0.477      --      --  |             0.102      --  |                 --      --
  256  pe_diff_big   0.351      --      --  |          0.456      --      --  |             0.102      --  |                 --      --
  256  pe_steep      0.351      --      --  |          0.318      --      --  |             0.102      --  |                 --      --
  256  ln_offset     0.237      --      --  |          0.188      --      --  |             0.047      --  |                 --      --
  256  ln_flat       0.387      --      --  |          0.410      --      --  |             0.064      --  |                 --      --

No bf16 kernel exceeds a constant its fp32 sibling meets: the worst ratio is 0.73 at C = 1 (fp32 siblings: 0.49 ... 0.93),
the same at both gains and in every regime; the regimes' repeated figures (0.269, 0.363, 0.351) belong to the same rows
in every regime, rows that b_post alone holds.  The matrix-core kernel's rows differ from ref16 by 5e-5 ... 3e-3 where an
element of h_e was flagged (d_post covers it) and by 1e-6 elsewhere.  The logits of a bf16 tail sit far below their
bound wherever an activation is flagged (d_logit ~ 1e-2: one bf16 spacing through |A| |w_dot|, most logits at D >= 128)
and at 0.1 ... 0.2 of C_TAIL s_l where none is.

Teeth (e), smallest factor by which a near-miss lies outside the committed bound over the five knob sets, case's seed:
(i) unrounded reference 660 ... 1600 x, (ii) truncation 1500 ... 3100 x, (iii) one entry of the largest pair lost 19 ...
6000 x; the truncating tail of (c) 1200 ... 2100 x on 7 % (D = 256) ... 74 % (D = 32) of the logits, those without a
flagged activation.  At seed + 1000, (256, all, wide), (iii) lies INSIDE the matrix-core kernel's bound (0.017): the
entries of the hub pair share small PPR values, so one element of h_e near a midpoint is flagged in hundreds of them,
and d_post of that row exceeds the loss of one entry.  A weakness of the flip bound on such rows, not met at the
committed seed.  For the same reason the hub pair alone reaches a flagged fraction of 4.9e-3 at (32, all, wide, seed +
1000); and the bf16 tail's fraction at D = 256 is 4.6e-3 ... 4.9e-3 (test_gpu_bf16's tail test: 4.65e-3), close to the cap.

What the mode costs (f): max |logits with attention and tail in bf16 - unrounded fp64 logits|, rows4, worst of the
three seeds.  The figure that the reference alone predicts (computed on the CPU before the kernel output is read)
agrees with the card's to three digits, so one column serves both -- but for (256, ln_offset, seed + 2000), 7.04e-4 on
the card against 6.74e-4 predicted: a tail activation rounded the other way.  max |logit| is 0.15 ... 0.36: the cost is
2e-3 ... 5e-3 of the largest logit.

  D     gain 1    wide      init      pe_diff   pe_diff_big  pe_steep  ln_offset  ln_flat
  32    7.86e-04  7.86e-04  7.86e-04  7.86e-04  7.86e-04     7.86e-04  7.86e-04   6.84e-04
  64    8.81e-04  1.09e-03  8.81e-04  9.11e-04  8.79e-04     9.22e-04  8.81e-04   8.52e-04
  128   8.66e-04  1.64e-03  8.66e-04  7.41e-04  8.23e-04     7.75e-04  8.66e-04   7.57e-04
  256   8.87e-04  4.39e-03  8.87e-04  8.97e-04  9.92e-04     9.40e-04  8.87e-04   8.87e-04

At random init and in every regime the 5e-3 of test_gpu_configs has a margin of 5; at the wide gain the cost grows with
D to 4.4e-3 (D = 256): rounding Z moves a score by ~2^-9 M_e, which the gain multiplies.  5e-3 is asserted at gain 1 and
init only, as it is stated today.
"""
import collections

import numpy as np
import pytest

from tests import bf16_reference as R
from tests import f32_error_model as E
from tests import param_regimes as PR
from tests import test_gpu_f32_reference as F32
from tests import test_gpu_param_regimes as PRG
from tests import unfolded_reference as U
from tests.scoring_harness import Reach, _DEFAULTS, _inputs, _lite, _np, _setup, knobs
from tests.test_gpu_bf16 import ATT_ENTRIES, FLAG_FRACTION, OLD_ATT_TOL, TAIL_ENTRIES
from tests.test_gpu_f32_reference import C_ATT, C_TAIL, FAMILY, WIDE_RANGE, _set
from tests.test_gpu_param_regimes import C_H

pytestmark = pytest.mark.gpu

KNOBS = knobs("bf16")
F32_ATT = F32.ATT_ENTRIES + F32.GATHER_ENTRIES
WATCHED = ATT_ENTRIES + TAIL_ENTRIES + F32_ATT + F32.TAIL_ENTRIES
GAIN_CASES = [(32, "all"), (64, "all"), (128, "all"), (256, "all"), (128, "1-hop"), (64, "cn")]
REGIME_CASES = [(d, r, k) for d in (64, 128) for r in PR.REGIMES for k in KNOBS] + \
               [(d, r, "rows4") for d in (32, 256) for r in PR.REGIMES]
TAIL_REGIMES = ("init", "ln_offset", "ln_flat")
# knob -> (bf16 tail entry point, pairs scored without their pairwise branch?)
TAIL_KNOBS = {"rows4": ("lpf_tail_chain_rows_perm_bf16", True), "rows_perm": ("lpf_tail_chain_rows_perm_bf16", True),
              "rows": ("lpf_tail_chain_rows_bf16", False), "flip": ("lpf_tail_chain_merge_bf16", False)}

RATIOS = collections.defaultdict(list)      # (kind, D, gain / regime, family) -> err / bound at C = 1
COST = {}                                   # (D, gain / regime) -> (measured, predicted)
_seen = collections.defaultdict(set)        # D -> bf16 entry points reached
_cases = {}
SEED_SHIFT = 0                              # (+ 1000, + 2000: the other two seeds of the measured tables)


def _tag(wide):
    return "wide" if wide else "gain1"


def _references(model, score, tb, h, msd=None):
    """Everything one batch's checks share, from the reference alone (arrays read-only): per ``fused`` the rounded
    restatement with its C = 1 bounds; the unrounded one (``f32``: the fp32 kernels' reference and bound); the tail's
    inputs.  ``msd`` (regimes): the fp64 state dict -- b_h widens the flag window and is carried as b_post_h."""
    inp = _inputs(model, score, tb, h)
    args = (inp["sel"], inp["z"], inp["q"], inp["w"], inp["att_bias"], *inp["ln"], inp["bs"])
    b_h = None if msd is None else E.h_window(inp["sel"], msd)
    ew = model.elementwise_lin
    ew_args = (_np(h), tb.cpu().numpy(), *(_np(p) for p in (ew.linears[0].weight, ew.linears[0].bias, ew.norm.weight,
                                                           ew.norm.bias)))
    out = {"inp": inp, "args": args, "b_re": E.elementwise_bound(*ew_args), "win_re": E.elementwise_window(*ew_args)}
    for key, kw in (("f32", dict(fused=False, round_z=False)), (False, dict(fused=False)), (True, dict(fused=True))):
        ref, bnd = E.attention_bf16(*args, b_h=b_h, **kw)
        assert (bnd["b_post"] <= bnd["b_post_worst"]).all()
        for a in (ref["post"], ref["d_post"], bnd["b_post"], bnd["b_post_h"]):
            a.setflags(write=False)
        if key is False:
            out["range"] = E.score_ranges(ref, inp["bs"])
        # (the per-entry arrays are not kept: [E, D] fp64 each, three references per case)
        out[key] = {"ref": {k: ref[k] for k in ("post", "counts", "d_post", "n_flag", "n_elem", "ds_max")},
                    "bnd": {k: bnd[k] for k in ("b_post", "b_post_h")},
                    "feats": R.count_features(ref["counts"], model.count_dim)}
    return out


def _case(dim, mode, wide):
    """Model, batch and references of one (D, mode, gain) with the hub pair alone beside them.  The wide gain is
    WIDE_RANGE / (the widest pair's range of the rounded reference of the same case at gain 1)."""
    key = (dim, mode, wide, SEED_SHIFT)
    if key not in _cases:
        gain = WIDE_RANGE / float(_case(dim, mode, False)["range"].max()) if wide else 1.0
        model, score, data, tb = _setup(dim, mode, seed=dim + len(mode) + SEED_SHIFT, att_gain=gain)
        h = model.propagate()
        c = {"model": model, "score": score, "tb": tb, "h": h, "gain": gain, "dim": dim, "mode": mode, "wide": wide}
        c.update(_references(model, score, tb, h))
        one = tb[:, :1].contiguous()
        c["one"] = dict(_references(model, score, one, h), tb=one)
        _cases[key] = c
    return _cases[key]


def _regime_case(dim, regime):
    """test_gpu_param_regimes' case (it asserts the regime's condition on the unfolded fp64 reference, and the batch
    conditions) with the folded references on ``_inputs`` beside it."""
    key = (dim, regime, SEED_SHIFT)
    if key not in _cases:
        c0 = PRG._case(dim, regime, SEED_SHIFT)
        c = {k: c0[k] for k in ("model", "score", "tb", "h", "dim")}
        c.update(mode="all", wide=False, regime=regime)
        c.update(_references(c["model"], c["score"], c["tb"], c["h"], U.state64(c["model"])))
        _cases[key] = c
    return _cases[key]


def _conditions(c):
    """The batch conditions (and at the wide gain those on the reference's ranges), before any kernel output."""
    cnt = c[False]["ref"]["counts"].sum(axis=1)
    bs = c["tb"].shape[1]
    assert cnt.max() > (512 if c["mode"] != "cn" else 96) and (cnt == 0).sum() > 64 and (cnt == 1).any() and bs % 64
    rng_ = c["range"]
    if c["wide"]:
        nonempty = cnt > 0
        assert rng_[0] >= 30 and (rng_[nonempty] >= 10).mean() >= 0.25
        top = np.float32(rng_.max())
        assert np.isfinite(np.exp(top)) and np.exp(-top) > 0
    return cnt


def _flag_cap(r, what, record_only=False):
    frac = r["n_flag"] / max(1, r["n_elem"])
    print(f"{what}: flagged fraction {frac:.2e} ({r['n_flag']} of {r['n_elem']})")
    assert record_only or frac < FLAG_FRACTION, (what, frac)


def _run(c, name, reach, tb=None, precision="bf16", tail="f32"):
    """calc_pairwise rows and score_pairs logits of one knob set at the given precisions; the model is left as found."""
    model, h, score = c["model"], c["h"], c["score"]
    tb = c["tb"] if tb is None else tb
    settings = KNOBS[name][0]
    _set(model, settings)
    model.precision, model.tail_precision = precision, tail
    try:
        _, ran = reach.ran(lambda: model.calc_pairwise(tb, h))
        rows = _np(model._last_att).copy()
        assert model.check_selection()
        lg, ran2 = reach.ran(lambda: model.score_pairs(tb, h, score, logits=True))
        assert model.check_selection()
    finally:
        model.precision = model.tail_precision = "f32"
        _set(model, {k: _DEFAULTS[k] for k in settings})
    return rows, _np(lg), ran, ran2


def _row_bound(r, fam, dim, c_att=None, c_h=None):
    c_att = C_ATT[fam][dim] if c_att is None else c_att
    return E.row_bound(r["bnd"], c_att, C_H[dim] if c_h is None else c_h)


def _tail_pieces(c, r, tabs, b_re):
    ref = {"post": r["ref"]["post"], "feats": r["feats"], "r_e": c["inp"]["r_e"]}
    s_own = E.tail_sigma(ref["post"], ref["feats"], ref["r_e"], tabs, np.zeros_like(ref["post"]), b_re)
    return ref, {"tabs": tabs, "b_re": b_re, "s_own": s_own}


def _check(name, key, got, ref, bound1, bound, flip, record_only=False):
    """Assert |got - ref| <= bound + flip elementwise (``bound`` at the committed constants, ``bound1`` at C = 1);
    records and prints the worst err / (bound1 + flip)."""
    err = np.abs(got.astype(np.float64) - ref)
    r1 = float((err / (bound1 + flip)).max())
    rc = float((err / (bound + flip)).max())
    RATIOS[key].append(r1)
    print(f"{name}: max |got - ref16| {err.max():.3e}, worst err / bound(C = 1) {r1:.3f}, / committed bound {rc:.3f}")
    assert np.isfinite(got).all() and (record_only or rc <= 1.0), f"{name}: {err.max():.3e} beyond the bound ({rc:.2f})"


def _check_attention(c, name, reach, label, batch=None):
    """Rows and logits (fp32 tail) of one bf16 attention kernel on ``batch`` (None: the case's own) against ref16."""
    dim, fam, fused = c["dim"], FAMILY[name], name == "mfma"
    src = c if batch is None else c["one"]
    r = src[fused]
    if fused:
        _flag_cap(r["ref"], f"{label} h_e")                                  # (on the reference, before any output)
    rows, lg, ran, ran2 = _run(c, name, reach, None if batch is None else src["tb"])
    if batch is None:
        cp_entry, sp_entries = KNOBS[name][1:]
        assert cp_entry in ran and sp_entries <= ran2, (name, ran, ran2)
    assert not (ran | ran2) & (set(F32_ATT) | set(TAIL_ENTRIES)), ran | ran2
    _seen[dim].update((ran | ran2) & set(ATT_ENTRIES))
    key = c.get("regime", _tag(c["wide"]))
    flip = r["ref"]["d_post"]
    _check(f"{label} rows", ("rows", dim, key, fam), rows, r["ref"]["post"], _row_bound(r, fam, dim, 1.0, 1.0),
           _row_bound(r, fam, dim), flip)
    tabs = src["inp"]["tabs"]
    t = R.tail_ref(r["ref"]["post"], r["feats"], src["inp"]["r_e"], tabs, d_rows=flip)
    ref, bnd = _tail_pieces(src, r, tabs, src["b_re"])
    _check(f"{label} logits", ("tail", dim, key, fam), lg, t["logit"],
           E.logit_bound(ref, bnd, _row_bound(r, fam, dim, 1.0, 1.0), 1.0),
           E.logit_bound(ref, bnd, _row_bound(r, fam, dim), C_TAIL[dim]), t["d_logit"])
    return rows, lg


# ------------------------------------------------------------------------------------------------- a: gains
@pytest.mark.parametrize("name", list(KNOBS))
@pytest.mark.parametrize("wide", [False, True], ids=["gain1", "wide"])
@pytest.mark.parametrize("dim,mode", GAIN_CASES)
def test_bf16_attention_at_gain(dim, mode, wide, name, monkeypatch):
    """(a) one bf16 attention kernel, rows and logits behind the fp32 tail, on the batch and on the hub pair alone."""
    c = _case(dim, mode, wide)
    cnt = _conditions(c)
    print(f"D = {dim} {mode} gain {c['gain']:.3f}: hub range {c['range'][0]:.2f}, widest {c['range'].max():.2f}, "
          f"{int(cnt.sum())} entries, largest pair {int(cnt.max())}")
    reach = Reach(monkeypatch, WATCHED)
    label = f"[{dim} {mode} {_tag(wide)} {name}]"
    _check_attention(c, name, reach, label)
    _check_attention(c, name, reach, label + " bs = 1", batch="one")


# ------------------------------------------------------------------------------------------------- e: teeth
@pytest.mark.parametrize("wide", [False, True], ids=["gain1", "wide"])
@pytest.mark.parametrize("dim,mode", GAIN_CASES)
def test_bf16_attention_teeth(dim, mode, wide, monkeypatch):
    """(e) for every knob set of the case: (i) the unrounded fp64 reference, (ii) the reference whose roundings
    truncate, (iii) the reference without one entry of the largest pair -- each outside the committed bound, (i) and
    (ii) on at least one row, (iii) on the largest pair."""
    c = _case(dim, mode, wide)
    cnt = _conditions(c)
    inp, args = c["inp"], c["args"]
    big = int(np.argmax(cnt))
    # the entry to lose: the first of the largest pair that weighs at least half an even share, 1 / (2 count), and less
    # than 1/2.  (At gain 1 the weights are near even and it is the first or an early entry, as in test_gpu_bf16; at the
    # wide gain the softmax has saturated and the first entries weigh 1e-30: losing one of those changes no row.  Where
    # one entry holds the pair and no other reaches half an even share, that entry.)
    ent = R.attention_ref(*args, round_z=True, detail=True)["ent"]
    ok = (ent["pair"] == big) & (ent["alpha"] >= 0.5 / cnt[big]) & (ent["alpha"] < 0.5)
    e = int(np.flatnonzero(ok)[0]) if ok.any() else int(np.argmax(np.where(ent["pair"] == big, ent["alpha"], -1.0)))
    ofs = np.cumsum([0] + [0 if s is None else s[0].shape[1] for s in inp["sel"]])
    t_big, e_big = int(ent["type"][e]), e - int(ofs[int(ent["type"][e])])
    print(f"teeth (iii): entry {e_big} of type {t_big} of pair {big} ({int(cnt[big])} entries), alpha {ent['alpha'][e]:.3e}")
    del ent
    near = {}
    for fused in (False, True):
        kw = dict(round_z=True, round_h=fused, round_wfold=fused)
        near[fused] = {"(i) unrounded": c["f32"]["ref"]["post"],
                       "(ii) truncated": R.attention_ref(*args, rounder=R.trunc_bf16, **kw)["post"],
                       "(iii) entry dropped": R.attention_ref(*args, drop=(t_big, e_big), **kw)["post"]}
    reach = Reach(monkeypatch, WATCHED)
    inside = []
    for name in KNOBS:
        fam, fused = FAMILY[name], name == "mfma"
        r = c[fused]
        rows, _, _, _ = _run(c, name, reach)
        bound = _row_bound(r, fam, dim) + r["ref"]["d_post"]
        for what, post in near[fused].items():
            gap = np.abs(rows - post) / bound
            worst = float(gap[big].max() if what.startswith("(iii)") else gap.max())
            print(f"teeth [{dim} {mode} {_tag(wide)} {name}] {what}: {worst:.1f} x the bound; rows outside "
                  f"{int((gap.max(axis=1) > 1).sum())} of {gap.shape[0]}; max gap {np.abs(rows - post).max():.3e} = "
                  f"{np.abs(rows - post).max() / OLD_ATT_TOL:.3f} x the old 5e-3")
            if not worst > 1.0:
                inside.append((name, what, round(worst, 3)))
    assert not inside, f"near-miss references inside the bound: {inside}"


# ------------------------------------------------------------------------------------------------- b: regimes
@pytest.mark.parametrize("dim,regime,name", REGIME_CASES)
def test_bf16_attention_at_regime(dim, regime, name, monkeypatch):
    """(b) one bf16 attention kernel at one regime: rows and logits (fp32 tail) against the folded restatement on the
    model's own fp32 tables with the kernel's roundings on; b_h widens the flag window of h_e and enters the bound as
    C_H b_post_h."""
    c = _regime_case(dim, regime)
    _conditions(c)
    _check_attention(c, name, Reach(monkeypatch, WATCHED), f"[{dim} {regime} {name}]")


# ------------------------------------------------------------------------------------------------- c, d: bf16 tail
def _check_tail(c, name, r, rows_b1, rows_b, attention, label, key, reach, record_only=False):
    """Logits of the bf16 tail behind ``attention`` ("bf16" / "f32") against tail_ref with its roundings on and the
    rows' bound carried in; the flagged-fraction cap is asserted on the reference first.  ``record_only``: the
    fraction and the ratio are printed, neither is asserted."""
    dim, fam = c["dim"], FAMILY[name]
    entry, lite = TAIL_KNOBS[name]
    inp = c["inp"]
    lt = _lite(r["ref"]["counts"], inp["bs"]) if lite else None
    if lite:
        assert lt.any()
    kw = dict(round_act=True, round_w=True, lite=lt, f32_unit=R.U32, win_re=c["win_re"])
    t = R.tail_ref(r["ref"]["post"], r["feats"], inp["r_e"], inp["tabs"], d_rows=rows_b, **kw)
    _flag_cap(t, f"{label} tail", record_only)
    tabs16 = dict(inp["tabs"], w_p0=R.rne_bf16(inp["tabs"]["w_p0"]), A=R.rne_bf16(inp["tabs"]["A"]))
    ref, bnd = _tail_pieces(c, r, tabs16, c["b_re"])
    _, lg, ran, ran2 = _run(c, name, reach, precision=attention, tail="bf16")
    assert entry in ran2 and not ran2 & set(F32.TAIL_ENTRIES), (name, ran2)
    att_ran = (ran | ran2) & (set(ATT_ENTRIES) | set(F32_ATT))
    assert att_ran and att_ran <= set(ATT_ENTRIES if attention == "bf16" else F32_ATT), att_ran
    _seen[dim].update((ran | ran2) & set(ATT_ENTRIES + TAIL_ENTRIES))
    _check(f"{label} logits", key, lg, t["logit"], E.logit_bound(ref, bnd, rows_b1, 1.0),
           E.logit_bound(ref, bnd, rows_b, C_TAIL[dim]), t["d_logit"], record_only)
    return lg, t, kw


BOTH_CASES = [(d, w, k) for d in (32, 64, 128, 256) for w in (False, True) for k in TAIL_KNOBS
              if not (k == "flip" and d == 256)]      # (no lpf_tail_chain_merge_bf16 that wide: built for D <= 128)


@pytest.mark.parametrize("dim,wide,name", BOTH_CASES)
def test_bf16_attention_with_bf16_tail(dim, wide, name, monkeypatch):
    """(c) precision = tail_precision = "bf16", the combination bench.py times.  Teeth (rows4): the tail reference
    rounding by truncation is outside on at least one logit."""
    c = _case(dim, "all", wide)
    _conditions(c)
    fam, r = FAMILY[name], c[False]
    rows_b = _row_bound(r, fam, dim) + r["ref"]["d_post"]
    label = f"[{dim} all {_tag(wide)} {name} + bf16 tail]"
    lg, t, kw = _check_tail(c, name, r, _row_bound(r, fam, dim, 1.0, 1.0), rows_b, "bf16", label,
                            ("both", dim, _tag(wide), fam), Reach(monkeypatch, WATCHED))
    if name == "rows4":
        tr = R.tail_ref(r["ref"]["post"], r["feats"], c["inp"]["r_e"], c["inp"]["tabs"], d_rows=rows_b,
                        **dict(kw, rounder=R.trunc_bf16))
        tabs16 = dict(c["inp"]["tabs"], w_p0=R.rne_bf16(c["inp"]["tabs"]["w_p0"]), A=R.rne_bf16(c["inp"]["tabs"]["A"]))
        ref, bnd = _tail_pieces(c, r, tabs16, c["b_re"])
        gap = np.abs(lg - tr["logit"]) / (E.logit_bound(ref, bnd, rows_b, C_TAIL[dim]) + t["d_logit"])
        print(f"teeth {label} truncating tail: {gap.max():.1f} x the bound, {(gap > 1).mean():.1%} of logits outside")
        assert (gap > 1.0).any()
        # (f) what the mode costs, next to what the reference alone predicts
        exact = R.tail_ref(c["f32"]["ref"]["post"], c["f32"]["feats"], c["inp"]["r_e"], c["inp"]["tabs"])["logit"]
        _cost(dim, _tag(wide), lg, t["logit"], exact)
        if not wide:
            assert np.abs(lg - exact).max() <= OLD_ATT_TOL


def _cost(dim, key, got, ref16, exact):
    COST[(dim, key)] = (float(np.abs(got - exact).max()), float(np.abs(ref16 - exact).max()))
    print(f"cost of the bf16 mode D = {dim} {key}: max |bf16 logits - unrounded fp64 logits| {COST[(dim, key)][0]:.3e} "
          f"(the reference alone predicts {COST[(dim, key)][1]:.3e}; max |logit| {np.abs(exact).max():.2f})")


@pytest.mark.parametrize("name", ["rows4", "rows", "flip"])
@pytest.mark.parametrize("regime", TAIL_REGIMES)
@pytest.mark.parametrize("dim", [64, 128])
def test_bf16_tail_at_regime(dim, regime, name, monkeypatch):
    """(d) the three bf16 tail entry points behind the fp32 attention at init, ln_offset (+30 on the biases in front of
    LN_B and the elementwise LayerNorm: the values the tail rounds carry 30 2^-24) and ln_flat (rows with amplified
    errors enter the first GEMM)."""
    c = _regime_case(dim, regime)
    _conditions(c)
    fam, r = FAMILY[name], c["f32"]
    assert not r["ref"]["d_post"].any()
    _check_tail(c, name, r, _row_bound(r, fam, dim, 1.0, 1.0), _row_bound(r, fam, dim), "f32",
                f"[{dim} {regime} {name}: bf16 tail, fp32 attention]", ("tail16", dim, regime, fam),
                Reach(monkeypatch, WATCHED))


# ------------------------------------------------------------------------------------------------- f: cost at regimes
@pytest.mark.parametrize("regime", PR.REGIMES)
@pytest.mark.parametrize("dim", [32, 64, 128, 256])
def test_bf16_mode_cost_at_regime(dim, regime, monkeypatch):
    """(f) precision = tail_precision = "bf16" at its default knobs at one regime: the distance of the logits to the
    unrounded fp64 logits, recorded next to the reference's prediction; 5e-3 asserted at init, where it is stated today.
    Their ratio to the bound of (c) and the tail's flagged fraction are recorded too and not asserted: under ln_offset at
    D = 256 the tail's window (with the bias-add rounding in it) flags 6.0e-3 of the activations, above the cap that
    keeps a flip bound worth asserting -- (d) asserts bound and cap at D = 64 and 128, where it holds."""
    c = _regime_case(dim, regime)
    _conditions(c)
    r = c[False]
    rows_b = _row_bound(r, "rows", dim) + r["ref"]["d_post"]
    lg, t, _ = _check_tail(c, "rows4", r, _row_bound(r, "rows", dim, 1.0, 1.0), rows_b, "bf16",
                           f"[{dim} {regime} rows4 + bf16 tail]", ("both", dim, regime, "rows"),
                           Reach(monkeypatch, WATCHED), record_only=True)
    assert np.isfinite(lg).all()
    exact = R.tail_ref(c["f32"]["ref"]["post"], c["f32"]["feats"], c["inp"]["r_e"], c["inp"]["tabs"])["logit"]
    _cost(dim, regime, lg, t["logit"], exact)
    if regime == "init":
        assert np.abs(lg - exact).max() <= OLD_ATT_TOL


# ------------------------------------------------------------------------------------------------- coverage
def test_bf16_entry_points_reached_at_every_width(monkeypatch):
    """The five bf16 attention and three bf16 tail entry points ran at every D they are built for (the merge tail: D <=
    128) -- with the two of the encoder, pinned in tests/test_gpu_bf16.py, the ten of the bf16 modes.  Run on its own it
    runs one knob set of each kind per D first."""
    reach = Reach(monkeypatch, WATCHED)
    for dim in (32, 64, 128, 256):
        want = set(ATT_ENTRIES + TAIL_ENTRIES) - ({"lpf_tail_chain_merge_bf16"} if dim == 256 else set())
        if not want <= _seen[dim]:
            c = _case(dim, "all", False)
            for name in KNOBS:
                _check_attention(c, name, reach, f"[{dim} all gain1 {name}]")
            for name in TAIL_KNOBS:
                if not (name == "flip" and dim == 256):
                    r = c[False]
                    fam = FAMILY[name]
                    _check_tail(c, name, r, _row_bound(r, fam, dim, 1.0, 1.0), _row_bound(r, fam, dim), "bf16",
                                f"[{dim} {name} + bf16 tail]", ("both", dim, "gain1", fam), reach)
        print(f"D = {dim}: reached {sorted(_seen[dim])}")
        assert want <= _seen[dim], (dim, want - _seen[dim])
    for key in sorted(RATIOS, key=str):
        print("worst err / bound(C = 1)", key, f"{max(RATIOS[key]):.3f}")
    for key in sorted(COST, key=str):
        print("cost", key, "measured %.3e predicted %.3e" % COST[key])
