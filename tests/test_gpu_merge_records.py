"""The record-merge kernels against the fp64 merge of the same records (GPU box only).

lpf_pair_attention_merge_f32 and lpf_tail_chain_merge_f32 take the online-softmax records (acc[D], m, l) of the one-pass
attention kernels as inputs.  tests/merge_reference.py hands them synthetic records -- unit cuts, score ranges and
parameters chosen here, not whatever a graph yields -- with NaN at every float the documented layout does not name, and
states the result in fp64 (reference (b): the merge of the fp32 records the kernel reads; that it is the PyG softmax
over the underlying entries, and that every family meets the conditions below, is checked on the CPU in
tests/test_merge_reference_host.py).

Tolerances: features and logits |got - ref| <= 2e-5 max(1, max|ref|) (the bound the suite holds fp32 attention features
to), probabilities 1e-5 absolute, count columns exact.  Every row of every case is compared.  Conditions: pre-norm
standard deviation of every row >= 0.1, poison present before the launch, no NaN in the output unless sel_ctl[3] is set.

Every test prints its worst error.  A CPU port of pair_merge_kernel's arithmetic (fp32 numpy, same order of operations)
gives 1e-7 .. 2e-7 of max(1, max|ref|) in every family at D = 32; the figures of an MI355X are not recorded here yet.
"""
import numpy as np
import pytest
import torch

from lpformer_amd import _lib, fold
from lpformer_amd._lib import check, ptr
from tests import merge_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.0
WIDTHS = (32, 64, 128, 256)

_cases, _tails = {}, {}


def _case(D, nc, fam, counts="structure"):
    """One case and its reference rows, built once and left unchanged."""
    key = (D, nc, fam, counts)
    if key not in _cases:
        cnt = R.structure_counts(nc) if counts == "structure" else R.single_pair_counts(nc)
        c = R.make_case(cnt, D, nc, fam)
        pre = R.merged_records(c)
        assert float(pre.std(axis=1).min()) >= 0.1                 # LayerNorm condition
        c["ref"] = R.features(c, pre)
        c["ref"].setflags(write=False)
        del c["keys"], c["scores"]                                 # (the records are all the kernels see)
        _cases[key] = c
    return _cases[key]


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _ctl(mode):
    if mode is None:
        return None
    t = torch.zeros(8, dtype=torch.int64)
    t[3] = mode
    return t.to(DEV)


def _run_merge(c, ldo=None, ctl=None):
    D, nc, bs = c["D"], c["n_counts"], c["bs"]
    ldo = ldo or D + 4
    if R.structure_facts(c["type_ptr"])["empty_segments"]:
        assert R.nan_share(c)[0] > 0 and R.nan_share(c)[1] > 0   # poison in place before the launch
    part, bnd, tp = _dev(c["part"]), _dev(c["bnd"]), _dev(c["type_ptr"], torch.int32)
    bias, g, b = _dev(c["att_bias"]), _dev(c["ln_g"]), _dev(c["ln_b"])
    out = torch.full((bs, ldo), SENTINEL, dtype=torch.float32, device=DEV)
    sel = _ctl(ctl)
    check(_lib.hip().lpf_pair_attention_merge_f32(bs, D, nc, ptr(part), ptr(bnd), c["units_cap"], ptr(tp), ptr(bias),
                                                  ptr(g), ptr(b), ptr(sel), ptr(out), ldo, None),
          "lpf_pair_attention_merge_f32")
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64)


def _check_rows(got, ref, D, nc, what):
    assert got.shape[0] == ref.shape[0]
    assert not np.isnan(got).any(), f"{what}: NaN in the output (a float outside the layout was read)"
    scale = max(1.0, float(np.abs(ref[:, :D]).max()))
    err = float(np.abs(got[:, :D] - ref[:, :D]).max())
    print(f"{what}: worst |got - ref| = {err:.3e} = {err / scale:.2e} of max(1, max|ref|) over {got.shape[0]} rows")
    assert err <= 2e-5 * scale, f"{what}: {err:.3e} > 2e-5 * {scale:.3f}"
    assert np.array_equal(got[:, D:D + nc], ref[:, D:D + nc]), f"{what}: count columns"
    assert (got[:, D + nc:] == SENTINEL).all(), f"{what}: columns past D + n_counts were written"


# ------------------------------------------------------------------------------------------------- pair_merge
@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("nc", [1, 3, 4])
@pytest.mark.parametrize("D", WIDTHS)
def test_pair_merge_families(D, nc, fam):
    """Every structure (empty pairs, 1/15/16/17 entries, segments that start or end on a unit boundary, 1, 2 and 40
    boundaries crossed, two crossing segments in one unit; 149 pairs: no multiple of the pairs per wavefront) under
    every score range, sel_ctl null, ldo = D + 4."""
    c = _case(D, nc, fam)
    _check_rows(_run_merge(c), c["ref"], D, nc, f"pair_merge D={D} n_counts={nc} {fam}")


@pytest.mark.parametrize("fam", ["pm3_up", "pm3_down"])
@pytest.mark.parametrize("D", WIDTHS)
def test_pair_merge_shift_invariance(D, fam):
    """Records shifted by +-1e4 give the rows of the UNSHIFTED reference (the shifted case's own reference, computed
    from the shifted records, is what test_pair_merge_families compares with)."""
    c, c0 = _case(D, 4, fam), _case(D, 4, "pm3")
    assert float(np.abs(c["ref"] - c0["ref"]).max()) <= 1e-11
    _check_rows(_run_merge(c), c0["ref"], D, 4, f"pair_merge D={D} {fam} against the unshifted reference")


@pytest.mark.parametrize("nc", [1, 3, 4])
@pytest.mark.parametrize("D", WIDTHS)
def test_pair_merge_single_pair(D, nc):
    c = _case(D, nc, "pm3", counts="single")
    assert c["bs"] == 1
    _check_rows(_run_merge(c), c["ref"], D, nc, f"pair_merge D={D} n_counts={nc} bs=1")


@pytest.mark.parametrize("D", WIDTHS)
def test_pair_merge_wavefront_loop(D):
    """More pairs than the grid's wavefronts take in one pass (4096 blocks x 4 wavefronts x 64 / (D/4) pairs): copies of
    the structural case one behind the other, the last three pairs left off."""
    c0 = _case(D, 4, "pm80")
    per_pass = 4096 * 4 * (64 // (D // 4))
    reps = per_pass // c0["bs"] + 2
    c = R.tile_case(c0, reps, drop_last=3)
    assert c["bs"] > per_pass
    _check_rows(_run_merge(c), R.tiled_rows(c0["ref"], c["bs"]), D, 4, f"pair_merge D={D} bs={c['bs']}")


@pytest.mark.parametrize("nc", [1, 3, 4])
@pytest.mark.parametrize("D", WIDTHS)
def test_pair_merge_wide_rows_keep_their_sentinel(D, nc):
    """ldo = D + 8: the columns behind the count features are not the kernel's."""
    c = _case(D, nc, "pm3")
    got = _run_merge(c, ldo=D + 8)
    assert got.shape[1] == D + 8 and (got[:, D + nc:] == SENTINEL).all()
    _check_rows(got, c["ref"], D, nc, f"pair_merge D={D} n_counts={nc} ldo=D+8")


@pytest.mark.parametrize("D", WIDTHS)
def test_pair_merge_control_word(D):
    """sel_ctl[3] = 0 is the null case bit for bit; sel_ctl[3] = 1 makes every row NaN;
    bs = 0 returns LPF_OK and writes nothing."""
    c = _case(D, 4, "pm3")
    null, zero, one = _run_merge(c), _run_merge(c, ctl=0), _run_merge(c, ctl=1)
    _check_rows(zero, c["ref"], D, 4, f"pair_merge D={D} sel_ctl[3]=0")
    assert np.array_equal(null, zero)
    assert np.isnan(one[:, :D]).all()
    out = torch.full((4, D + 4), SENTINEL, dtype=torch.float32, device=DEV)
    part, bnd, tp = _dev(c["part"]), _dev(c["bnd"]), _dev(c["type_ptr"], torch.int32)
    v = _dev(c["att_bias"])
    rc = _lib.hip().lpf_pair_attention_merge_f32(0, D, 4, ptr(part), ptr(bnd), c["units_cap"], ptr(tp), ptr(v), ptr(v),
                                                 ptr(v), None, ptr(out), D + 4, None)
    torch.cuda.synchronize()
    assert rc == 0 and (out == SENTINEL).all()


# ------------------------------------------------------------------------------------------------- tail_chain merge
def _tail(D, nc):
    """Unpacked weights (fp64 side) and the images of the packer the model uses (LinkTransformer._tail_tables ->
    fold.tail_chain_tables), on the device."""
    if (D, nc) not in _tails:
        w = R.tail_weights(D, nc)
        zeros = np.zeros(D, np.float32)
        tabs = fold.tail_chain_tables(np.zeros((D, 3 * D + 4), np.float32), zeros, zeros, w["w_p0"], w["b_p0"],
                                      w["lnB_g"], w["lnB_b"], w["A"], w["c"], w["w_dot"], w["b_dot"], D)
        _tails[D, nc] = (w, {k: torch.from_numpy(v).to(DEV) for k, v in tabs.items()})
    return _tails[D, nc]


def _run_tail(c, ctl=None, bs=None):
    D, nc = c["D"], c["n_counts"]
    bs = c["bs"] if bs is None else bs
    w, tt = _tail(D, nc)
    r_e = np.maximum(np.random.default_rng([D, nc, 11]).standard_normal((c["bs"], D)), 0.0).astype(np.float32)
    part, bnd, tp = _dev(c["part"]), _dev(c["bnd"]), _dev(c["type_ptr"], torch.int32)
    bias, g, b, re_d = _dev(c["att_bias"]), _dev(c["ln_g"]), _dev(c["ln_b"]), _dev(r_e)
    logit = torch.full((max(c["bs"], 1),), SENTINEL, dtype=torch.float32, device=DEV)
    prob = torch.full((max(c["bs"], 1),), SENTINEL, dtype=torch.float32, device=DEV)
    sel = _ctl(ctl)
    rc = _lib.hip().lpf_tail_chain_merge_f32(
        bs, D, nc, ptr(part), ptr(bnd), c["units_cap"], ptr(tp), ptr(bias), ptr(g), ptr(b), ptr(tt["wB"]),
        ptr(tt["bB"]), ptr(tt["lnB_g"]), ptr(tt["lnB_b"]), ptr(re_d), D, ptr(tt["wC"]), ptr(tt["bC"]),
        ptr(tt["w_dot"]), ptr(tt["b_dot"]), ptr(sel), ptr(logit), ptr(prob), None)
    check(rc, "lpf_tail_chain_merge_f32")
    torch.cuda.synchronize()
    ref = R.tail_ref(c["ref"][:, :D], c["ref"][:, D:], r_e.astype(np.float64), w)
    return logit.cpu().numpy().astype(np.float64), prob.cpu().numpy().astype(np.float64), ref


def _check_tail(logit, prob, ref, what):
    ref_logit, ref_prob = ref
    assert logit.shape == ref_logit.shape
    assert not np.isnan(logit).any() and not np.isnan(prob).any(), f"{what}: NaN (a float outside the layout was read)"
    scale = max(1.0, float(np.abs(ref_logit).max()))
    e_l, e_p = float(np.abs(logit - ref_logit).max()), float(np.abs(prob - ref_prob).max())
    print(f"{what}: worst logit error {e_l:.3e} = {e_l / scale:.2e} of max(1, max|ref|), prob error {e_p:.3e} "
          f"over {logit.size} pairs")
    assert e_l <= 2e-5 * scale, f"{what}: logit {e_l:.3e} > 2e-5 * {scale:.3f}"
    assert e_p <= 1e-5, f"{what}: prob {e_p:.3e}"


@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("nc", [3, 4])
@pytest.mark.parametrize("D", [32, 64, 128])
def test_tail_merge_families(D, nc, fam):
    """The merge stage of lpf_tail_chain_merge_f32 on the same cases, seen through logit and prob: weight images from
    fold.tail_chain_tables, fp64 side from the unpacked weights (R.tail_ref)."""
    c = _case(D, nc, fam)
    logit, prob, ref = _run_tail(c)
    _check_tail(logit, prob, ref, f"tail_merge D={D} n_counts={nc} {fam}")


@pytest.mark.parametrize("fam", ["pm3_up", "pm3_down"])
@pytest.mark.parametrize("D", [32, 64, 128])
def test_tail_merge_shift_invariance(D, fam):
    c, c0 = _case(D, 4, fam), _case(D, 4, "pm3")
    logit, prob, _ = _run_tail(c)
    w, _ = _tail(D, 4)
    r_e = np.maximum(np.random.default_rng([D, 4, 11]).standard_normal((c["bs"], D)), 0.0).astype(np.float32)
    ref0 = R.tail_ref(c0["ref"][:, :D], c0["ref"][:, D:], r_e.astype(np.float64), w)
    _check_tail(logit, prob, ref0, f"tail_merge D={D} {fam} against the unshifted reference")


@pytest.mark.parametrize("nc", [3, 4])
@pytest.mark.parametrize("D", [32, 64, 128])
def test_tail_merge_single_pair(D, nc):
    c = _case(D, nc, "pm3", counts="single")
    logit, prob, ref = _run_tail(c)
    _check_tail(logit, prob, ref, f"tail_merge D={D} n_counts={nc} bs=1")


@pytest.mark.parametrize("D", [32, 64, 128])
def test_tail_merge_control_word(D):
    c = _case(D, 4, "pm3")
    l_null, p_null, ref = _run_tail(c)
    l_zero, p_zero, _ = _run_tail(c, ctl=0)
    _check_tail(l_zero, p_zero, ref, f"tail_merge D={D} sel_ctl[3]=0")
    assert np.array_equal(l_null, l_zero) and np.array_equal(p_null, p_zero)
    l_one, p_one, _ = _run_tail(c, ctl=1)
    assert np.isnan(l_one).all() and np.isnan(p_one).all()
    l_none, p_none, _ = _run_tail(c, bs=0)               # M = 0: LPF_OK (checked in _run_tail), nothing written
    assert (l_none == SENTINEL).all() and (p_none == SENTINEL).all()
