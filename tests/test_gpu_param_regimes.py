"""The fp32 scoring kernels at trained-like parameters (tests/param_regimes.py) against the model as defined, unfolded
in fp64 from the state dict (tests/unfolded_reference.py: no fold table, LayerNorms taken directly).

Harness graph and batch as they are (n = 2000, bs = 700, mode "all", seed = D + 3 as in test_gpu_f32_reference); one
reference per (D, regime), built once.  Each regime's condition is asserted on the reference alone before any kernel
output is looked at.  Per case two assertions on calc_pairwise rows and score_pairs logits:

  1. |got - ref| <= C_ATT[family][D] b_post + C_H[D] b_post_h per pair and feature (f32_error_model.unfolded_bounds:
     b_post_h carries b_h = u (sqrt(kappa) |r u| + m) + u |beta|, the conditioning of the closed-form variance as a sum of
     squares, through |W_rp W2|), logits <= C_TAIL[D] s_l with the rows at that bound.  C_ATT and C_TAIL are test_gpu_f32_reference's.
  2. the project's stated contract: max |got - ref| <= 1e-4 max(1, max |ref|), rows and logits, in every regime.

  D        regimes   knobs
  32, 128  all six   rows4, rows, rows_perm, flip, mfma, chain
  64, 256  all six   rows4

C_H follows test_gpu_f32_reference's rule: 4 x the worst ratio  err / (C_ATT b_post + b_post_h)  (rows) or
err / (C_TAIL s_l at those rows) (logits) measured over every case with the case's seed, + 1000 and + 2000, rounded up to
a power of two.

Measured on an AMD Instinct MI355X, worst over the case's seed, + 1000 and + 2000 (252 runs).  Columns 3-6: worst
err / (C_ATT b_post + b_post_h) of the rows per kernel family; "tail": worst err / (C_TAIL s_l) of the logits; the last two:
worst max |got - ref| / (1e-4 max(1, max |ref|)), the ratio to the contract, rows and logits.

  D    regime         rows    flip    mfma  gather    tail   rows/1e-4 logits/1e-4
  32   init          0.082   0.068   0.066   0.067   0.185    0.0042    0.0007
  32   pe_diff       0.082   0.066   0.066   0.066   0.138    0.0072    0.0009
  32   pe_diff_big   0.082   0.066   0.066   0.066   0.167    0.0279    0.0041
  32   pe_steep      0.119   0.110   0.105   0.078   0.153    0.0219    0.0007
  32   ln_offset     0.087   0.086   0.085   0.120   0.113    0.0317    0.0145
  32   ln_flat       0.096   0.113   0.113   0.108   0.150    0.0057    0.0022
  64   init          0.067      --      --      --   0.173    0.0044    0.0008
  64   pe_diff       0.067      --      --      --   0.147    0.0081    0.0009
  64   pe_diff_big   0.067      --      --      --   0.161    0.0274    0.0036
  64   pe_steep      0.085      --      --      --   0.145    0.0248    0.0015
  64   ln_offset     0.086      --      --      --   0.081    0.0716    0.0073
  64   ln_flat       0.078      --      --      --   0.184    0.0042    0.0007
  128  init          0.091   0.091   0.091   0.092   0.164    0.0077    0.0012
  128  pe_diff       0.108   0.108   0.091   0.091   0.157    0.0096    0.0016
  128  pe_diff_big   0.097   0.097   0.091   0.091   0.140    0.0241    0.0037
  128  pe_steep      0.091   0.091   0.091   0.100   0.140    0.0434    0.0022
  128  ln_offset     0.082   0.077   0.077   0.111   0.118    0.0424    0.0155
  128  ln_flat       0.087   0.082   0.069   0.099   0.197    0.0041    0.0013
  256  init          0.176      --      --      --   0.158    0.0071    0.0012
  256  pe_diff       0.176      --      --      --   0.156    0.0102    0.0017
  256  pe_diff_big   0.176      --      --      --   0.158    0.0235    0.0032
  256  pe_steep      0.176      --      --      --   0.134    0.0361    0.0027
  256  ln_offset     0.122      --      --      --   0.085    0.0401    0.0060
  256  ln_flat       0.193      --      --      --   0.175    0.0039    0.0014

  worst ratio -> C_H      0.185 -> 1 (D = 32)   0.184 -> 1 (64)   0.197 -> 1 (128)   0.193 -> 1 (256)

The largest ratios belong to rows that b_post alone holds (the same rows in every regime); b_post_h decides nothing at
these constants, and the contract has a margin of 14 x or more everywhere.

Before.  pe_stat held only the six centred second moments (its rows 0-2 still do) and the kernels evaluated their
quadratic form written out; b_h then took kappa, not sqrt(kappa).  Measured on the same device with the case's seed
only and ``pe_diff_big`` at W1 x 16,
b1 = 2 + 0.01 xi (kappa max 2.5e4 ... 3.7e4; not re-measured at the final multipliers), every family alike:

  rows / 1e-4 contract      D = 32    64      128     256          logits / 1e-4    32      64      128     256
  pe_diff                   0.155     0.436   0.108   0.107                         0.016   0.034   0.019   0.010
  pe_diff_big               4.785     0.537   0.530   0.809                         0.733   0.033   0.078   0.093

so assertion 2 failed at D = 32 (rows 1.6e-3 off at max |ref| 3.4) and stood at 0.5 ... 0.8 elsewhere, identically in all
six knob sets: the loss was in the stored moments and their cancellation, not in one kernel's arithmetic.  With the
triangular factor (rows 3-5 of pe_stat, which the kernels read now) the same regime sits at 0.03.  The other regimes
did not move (init 0.004 ... 0.008 before and after).

The training path (lpf_pe_hidden_fwd_f32, a LayerNorm over the units from W1, b1, gamma, beta) in ``pe_diff_big`` against the
unfolded h: err / (2e-5 max(1, max |h|)) 0.35 ... 0.58 at D = 32, 0.30 ... 0.42 at D = 128 (u sqrt(kappa) |h| is what any fp32
evaluation of this layer is good to: at W1 x 16, b1 = 2 + 0.01 xi it stood at 1.16 for one type at D = 32).
"""
import collections

import numpy as np
import pytest
import torch

from lpformer_amd import _lib
from tests import f32_error_model as E
from tests import param_regimes as PR
from tests import unfolded_reference as U
from tests.scoring_harness import Reach, _DEFAULTS, _np, _setup
from tests.test_gpu_f32_reference import (BF16_ENTRIES, C_ATT, C_TAIL, FAMILY, KNOBS, OLD_TOL, WATCHED, _set,
                                          _tail_entry)

pytestmark = pytest.mark.gpu

_W = (32, 64, 128, 256)
C_H = dict(zip(_W, (1.0, 1.0, 1.0, 1.0)))
FWD_TOL = 2e-5               # x max(1, max|h|): what test_pe_hidden_direct holds lpf_pe_hidden_fwd_f32 to

ALL_KNOBS = ("rows4", "rows", "rows_perm", "flip", "mfma", "chain")
CASES = [(d, r, k) for d in (32, 128) for r in PR.REGIMES for k in ALL_KNOBS] + \
        [(d, r, "rows4") for d in (64, 256) for r in PR.REGIMES]

RATIOS = collections.defaultdict(list)      # (family or "tail", D, regime) -> err / bound with C_H = 1
CONTRACT = collections.defaultdict(list)    # ("rows" or "logits", D, regime) -> max err / (1e-4 max(1, max|ref|))
_cases = {}


def _case(dim, regime, seed_shift=0):
    """Model, batch, unfolded fp64 reference and C = 1 bounds of one (D, regime), built once; the regime's condition is
    asserted here, on the reference alone."""
    key = (dim, regime, seed_shift)
    if key in _cases:
        return _cases[key]
    seed = dim + len("all") + seed_shift
    model, score, data, tb = _setup(dim, "all", seed=seed, regime=regime)
    h = model.propagate()
    sel = [None if s is None else tuple(_np(a) if a.dtype.is_floating_point else a.cpu().numpy() for a in s)
           for s in model.compute_node_mask(tb)]
    assert model.check_selection()
    msd, ssd = U.state64(model), U.state64(score)
    x_node, batch = _np(h), tb.cpu().numpy()
    ref = U.scoring(sel, x_node, batch, msd, ssd, model.count_dim)
    init_ref = _case(dim, "init", seed_shift)["ref"] if regime == "ln_offset" else None
    radius = PR.radii({k: v for k, v in model.state_dict().items()}, dim) if regime == "pe_steep" else None
    plain = None
    if regime == "ln_offset":
        plain = U.scoring(sel, x_node, batch, PR.without_offset(msd), ssd, model.count_dim)
    fig = PR.conditions(regime, ref, init_ref=init_ref, plain_ref=plain, sel=sel, radius=radius)
    bnd = E.unfolded_bounds(ref, x_node, batch, msd, ssd)
    ent = ref["ent"]
    cnt = ref["counts"].sum(axis=1)
    assert cnt.max() > 512 and (cnt == 0).sum() > 64 and (cnt == 1).any() and (batch[0] == batch[1]).any()
    kap = ent["kappa"].max(axis=1)
    print(f"D = {dim} {regime} (seed {seed}): {ent['pair'].size} entries, kappa max {kap.max():.3g} median "
          f"{np.median(kap):.3g}, flipped entries {ent['flipped'].mean():.3f}, median pre-norm variance "
          f"{np.median(ref['pre_var']):.3g}; condition: {fig}")
    c = {"model": model, "score": score, "tb": tb, "h": h, "dim": dim, "regime": regime, "sel": sel,
         "ref": {k: ref[k] for k in ("post", "logit", "feats", "r_e", "counts")},
         "bnd": {k: bnd[k] for k in ("b_post", "b_post_h", "tabs", "b_re", "s_own")}}
    if regime == "pe_diff_big":
        c["h_by_type"] = [ent["h"][ent["type"] == t] for t in range(3)]
    for a in (c["ref"]["post"], c["ref"]["logit"], c["bnd"]["b_post"], c["bnd"]["b_post_h"]):
        a.setflags(write=False)
    _cases[key] = c
    return c


def _run(c, name, reach):
    """calc_pairwise rows and score_pairs logits of one knob set, the entry points it claims reached."""
    model, tb, h, score, dim = c["model"], c["tb"], c["h"], c["score"], c["dim"]
    settings, cp_entry, sp_entries = KNOBS[name]
    _set(model, settings)
    try:
        _, ran = reach.ran(lambda: model.calc_pairwise(tb, h))
        rows = _np(model._last_att).copy()
        assert cp_entry in ran and model.check_selection(), (name, ran)
        lg, ran2 = reach.ran(lambda: model.score_pairs(tb, h, score, logits=True))
        assert sp_entries <= ran2 and _tail_entry(name, dim) in ran2 and model.check_selection(), (name, ran2)
        assert not (ran | ran2) & set(BF16_ENTRIES), ran | ran2
        if name == "rows4" and dim >= 128:      # the pattern tables in use were built from the rewritten parameters
            hit = model._pt_cache
            assert hit is not None and hit[0] == model._pattern_key() and model._folded[1].get("patterns") is hit[1]
    finally:
        _set(model, {k: _DEFAULTS[k] for k in settings})
    return rows, _np(lg)


def measure(dim, regime, name, monkeypatch, seed_shift=0):
    """One case: (ratio of the rows, ratio of the logits, rows / contract, logits / contract), ratios with C_H = 1 and
    the committed C_ATT, C_TAIL.  Prints every figure; asserts nothing about them."""
    c = _case(dim, regime, seed_shift)
    ref, bnd, fam = c["ref"], c["bnd"], FAMILY[name]
    rows, lg = _run(c, name, Reach(monkeypatch, WATCHED))
    assert np.isfinite(rows).all() and np.isfinite(lg).all()
    err = np.abs(rows.astype(np.float64) - ref["post"])
    el = np.abs(lg.astype(np.float64) - ref["logit"])
    rb1 = E.row_bound(bnd, C_ATT[fam][dim], 1.0)
    r_rows = float((err / rb1).max())
    r_all1 = float((err / E.row_bound(bnd, 1.0, 1.0)).max())
    r_log = float((el / E.logit_bound(ref, bnd, rb1, C_TAIL[dim])).max())
    k_rows = float(err.max() / (OLD_TOL * max(1.0, np.abs(ref["post"]).max())))
    k_log = float(el.max() / (OLD_TOL * max(1.0, np.abs(ref["logit"]).max())))
    RATIOS[(fam, dim, regime)].append(r_rows)
    RATIOS[("tail", dim, regime)].append(r_log)
    CONTRACT[("rows", dim, regime)].append(k_rows)
    CONTRACT[("logits", dim, regime)].append(k_log)
    print(f"[{dim} {regime} {name}] rows: max |got - ref| {err.max():.3e}, err / bound at C_H = 1 {r_rows:.3f} (every C = 1: "
          f"{r_all1:.3f}), / 1e-4 contract {k_rows:.4f}; logits: max {el.max():.3e}, err / bound {r_log:.3f}, / contract "
          f"{k_log:.4f}")
    return c, err, el, (r_rows, r_log, k_rows, k_log)


@pytest.mark.parametrize("dim,regime,name", CASES)
def test_regime_rows_and_logits_match_the_unfolded_model(dim, regime, name, monkeypatch):
    c, err, el, _ = measure(dim, regime, name, monkeypatch)
    ref, bnd, fam = c["ref"], c["bnd"], FAMILY[name]
    rb = E.row_bound(bnd, C_ATT[fam][dim], C_H[dim])
    assert (err <= rb).all(), f"rows beyond the bound: {(err / rb).max():.2f}"
    lb = E.logit_bound(ref, bnd, rb, C_TAIL[dim])
    assert (el <= lb).all(), f"logits beyond the bound: {(el / lb).max():.2f}"
    assert err.max() <= OLD_TOL * max(1.0, np.abs(ref["post"]).max()), "rows beyond the 1e-4 contract"
    assert el.max() <= OLD_TOL * max(1.0, np.abs(ref["logit"]).max()), "logits beyond the 1e-4 contract"


@pytest.mark.parametrize("dim", [32, 128])
def test_training_pe_hidden_agrees_with_the_unfolded_model(dim):
    """lpf_pe_hidden_fwd_f32 (the training path: W1, b1, gamma, beta, LayerNorm over the units) on the batch's (pa, pb)
    in ``pe_diff_big`` against the unfolded h, at test_pe_hidden_direct's tolerance."""
    c = _case(dim, "pe_diff_big")
    lib, st = _lib.hip(), torch.cuda.current_stream().cuda_stream
    model = c["model"]
    for t, name in enumerate(U.PE_KEYS):
        mod = getattr(model, name)
        pa, pb = (torch.from_numpy(a).to("cuda:0").contiguous() for a in c["sel"][t][1:])
        want = c["h_by_type"][t]
        n = pa.numel()
        assert n > 0 and want.shape == (n, dim)
        h = torch.full((n, dim), 7.0, dtype=torch.float32, device="cuda:0")
        w1, b1 = mod.linears[0].weight.detach().contiguous(), mod.linears[0].bias.detach().contiguous()
        gam, bet = mod.norm.weight.detach().contiguous(), mod.norm.bias.detach().contiguous()
        _lib.check(lib.lpf_pe_hidden_fwd_f32(n, dim, _lib.ptr(w1), _lib.ptr(b1), _lib.ptr(gam), _lib.ptr(bet),
                                             pa.data_ptr(), pb.data_ptr(), _lib.ptr(h), dim, st), "lpf_pe_hidden_fwd_f32")
        torch.cuda.synchronize()
        err = float(np.abs(_np(h).astype(np.float64) - want).max())
        tol = FWD_TOL * max(1.0, float(np.abs(want).max()))
        print(f"pe hidden (training path) D = {dim} {name}, {n} entries, pe_diff_big: err {err:.3e} / tolerance "
              f"{err / tol:.4f}")
        assert err <= tol, (name, err, tol)
