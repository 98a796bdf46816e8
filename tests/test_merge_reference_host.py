"""The synthetic-record helper (tests/merge_reference.py) checked on the CPU: the two fp64 references agree to the
rounding of the records, the NaN poison stays out of the reference, and every case family meets the conditions the GPU
tests (tests/test_gpu_merge_records.py) rely on.

Conditions, checked here for every family:
  * LayerNorm amplifies by 1/std: every reference row has a pre-norm standard deviation >= 0.1 (no case is dropped
    to get there: the keys carry a per-pair direction and att_bias has unit scale);
  * no pair is left out: the references have one finite row per pair;
  * pm300: at least one pair has a piece whose weight e^{m_P - M} is exactly 0 in fp32, and at least one pair with
    several pieces has all of them within 1 of its maximum;
  * the poison is in place: `part` and `bnd` hold NaN in every family (each has empty segments), and none of it
    reaches reference (b).
"""
import numpy as np
import pytest

from tests import merge_reference as R

D_HOST = 32          # the conditions do not depend on the width; the GPU tests build the other widths the same way


@pytest.fixture(scope="module")
def cases():
    return {(fam, nc): R.make_case(R.structure_counts(nc), D_HOST, nc, fam)
            for fam in R.FAMILIES for nc in (1, 3, 4)}


def test_structure_has_every_listed_shape():
    f = R.structure_facts(np.concatenate([np.zeros((3, 1), np.int64),
                                          np.cumsum(R.structure_counts(4), axis=1)], axis=1))
    assert {0, 1, 15, 16, 17} <= f["lengths"]
    assert f["empty_pairs"] >= 1 and f["one_type_pairs"] >= 3
    assert f["cross_from_boundary"] >= 1 and f["end_on_boundary"] >= 1 and f["aligned_unit"] >= 1
    assert {1, 2} <= f["boundaries"] and max(f["boundaries"]) >= 40
    assert f["shared_units"] >= 1                      # slot 0 and slot 1 of one unit belong to different pairs
    bs = R.structure_counts(4).shape[1]
    assert all(bs % (64 // g) for g in (8, 16, 32))    # no multiple of the pairs per wavefront (D = 256: one pair)
    for nc, used in ((1, 1), (3, 2), (4, 3)):
        c = R.structure_counts(nc)
        assert (c[used:] == 0).all() and (c[:used].sum(axis=1) % R.UNIT == 0).all()
    f1 = R.structure_facts(np.concatenate([np.zeros((3, 1), np.int64),
                                           np.cumsum(R.single_pair_counts(4), axis=1)], axis=1))
    assert f1["aligned_unit"] == 1 and 2 in f1["boundaries"]


@pytest.mark.parametrize("nc", [1, 3, 4])
@pytest.mark.parametrize("fam", R.FAMILIES)
def test_references_agree_to_the_rounding_of_the_records(cases, fam, nc):
    """(a) softmax over the entries against (b) merge of the fp32 records.  Bound: m is exact, acc and l carry one fp32
    rounding each (R.record_rounding_bound, first order), times 1 + 1e-3 for the second order, plus 1e-12 for the
    fp64 evaluation of sums of up to 650 terms of size <= 10."""
    c = cases[fam, nc]
    a, b = R.direct_softmax(c), R.merged_records(c)
    assert a.shape == b.shape == (c["bs"], c["D"])
    assert np.isfinite(a).all() and np.isfinite(b).all()          # every pair has a row; no poison in (b)
    bound = R.record_rounding_bound(c) * (1 + 1e-3) + 1e-12
    assert (np.abs(a - b) <= bound).all(), float((np.abs(a - b) - bound).max())
    # uniform form of the same bound: 2 u max|k| (|acc_P| <= l_P max|k|)
    kmax = max(float(np.abs(k).max()) for k in c["keys"] if k.size)
    assert float(np.abs(a - b).max()) <= 2 * R.U32 * kmax * (1 + 1e-3) + 1e-12
    fa, fb = R.features(c, a), R.features(c, b)
    lb = R.layer_norm_bound(b, bound, c["ln_g"]) * (1 + 1e-3) + 1e-12
    assert (np.abs(fa - fb)[:, :c["D"]] <= lb).all()
    assert np.array_equal(fa[:, c["D"]:], fb[:, c["D"]:])
    # LayerNorm condition
    assert float(b.std(axis=1).min()) >= 0.1 and float(a.std(axis=1).min()) >= 0.1
    # poison
    share_part, share_bnd = R.nan_share(c)
    assert R.structure_facts(c["type_ptr"])["empty_segments"] > 0 and share_part > 0 and share_bnd > 0
    assert np.isnan(c["part"][..., c["D"] + 2:]).all() and np.isnan(c["bnd"][..., c["D"] + 2:]).all()


def test_poison_is_noticed_at_a_wrong_address(cases):
    """Reading the other slot, or `part` where the records are in `bnd`, meets NaN: the poison works."""
    c = dict(cases["pm3", 4])
    swapped = dict(c, bnd=c["bnd"][:, :, ::-1].copy())
    assert np.isnan(R.merged_records(swapped)).any()
    tp = c["type_ptr"].astype(np.int64)
    crossing = np.flatnonzero((tp[0, :-1] >> 4) != ((tp[0, 1:] - 1) >> 4))
    assert crossing.size and np.isnan(c["part"][0, crossing]).all()


def test_score_families_are_what_they_say(cases):
    def spread(c):
        m = np.concatenate(c["piece_m"])
        return float(m.min()), float(m.max())
    assert spread(cases["equal", 4]) == (1.5, 1.5)
    for fam, lim, off in (("pm3", 3, 0), ("pm80", 80, 0), ("pm300", 300, 0), ("pm3_up", 3, 1e4), ("pm3_down", 3, -1e4)):
        lo, hi = spread(cases[fam, 4])
        assert off - lim <= lo < off - 0.8 * lim and off + 0.8 * lim < hi <= off + lim
    # a record's m is the maximum of the piece's scores and an fp32 number, shifted or not
    for fam in R.FAMILIES:
        c = cases[fam, 4]
        for t in range(3):
            assert np.array_equal(c["scores"][t].astype(np.float32).astype(np.float64), c["scores"][t])
    # tie: the maximum of a pair with several pieces is held by two pieces
    c = cases["tie", 4]
    pp, m = np.concatenate(c["piece_pair"]), np.concatenate(c["piece_m"])
    n_tied = 0
    for p in np.unique(pp):
        mp = m[pp == p]
        if mp.size >= 2:
            assert (mp == mp.max()).sum() == 2
            n_tied += 1
    assert n_tied >= 20


def test_pm300_underflows_and_has_close_pairs(cases):
    c = cases["pm300", 4]
    pp, m = np.concatenate(c["piece_pair"]), np.concatenate(c["piece_m"])
    zero_weight = close = 0
    for p in np.unique(pp):
        mp = m[pp == p]
        if mp.size < 2:
            continue
        d = (mp - mp.max()).astype(np.float32)
        with np.errstate(under="ignore"):
            zero_weight += bool((np.exp(d) == np.float32(0)).any() and (d < R.F32_EXP_ZERO).any())
        close += bool((d >= -1).all())
    assert zero_weight >= 1 and close >= 1


def test_shifted_records_are_the_unshifted_ones_moved(cases):
    """+-1e4 on the 2^-8 grid is exact in fp32: acc and l are bitwise the unshifted ones, m moves by the shift, and the
    reference computed FROM THE SHIFTED RECORDS equals the unshifted one to fp64 rounding."""
    base = cases["pm3", 4]
    ref0 = R.merged_records(base)
    for fam in ("pm3_up", "pm3_down"):
        c = cases[fam, 4]
        D = c["D"]
        for name in ("part", "bnd"):
            x, y = c[name], base[name]
            assert np.array_equal(np.isnan(x), np.isnan(y))
            assert np.array_equal(x[..., :D], y[..., :D], equal_nan=True)
            assert np.array_equal(x[..., D + 1], y[..., D + 1], equal_nan=True)
            ok = ~np.isnan(y[..., D])
            assert np.array_equal(x[..., D][ok].astype(np.float64), y[..., D][ok].astype(np.float64) + R.SHIFT[fam])
        assert float(np.abs(R.merged_records(c) - ref0).max()) <= 1e-12


def test_tiled_case_copies_the_base_rows():
    """tile_case / tiled_rows (the large batch of the GPU tests): the merge of the tiled records, computed from the
    tiled arrays, is the base reference repeated; the last pairs can be left off."""
    base = R.make_case(R.structure_counts(4), D_HOST, 4, "pm3")
    ref0 = R.merged_records(base)
    t = R.tile_case(base, 3, drop_last=3)
    assert t["bs"] == 3 * base["bs"] - 3 and t["type_ptr"].shape == (3, t["bs"] + 1)
    got = R.merged_records(t)
    assert np.array_equal(got, R.tiled_rows(ref0, t["bs"]))
    assert np.array_equal(R.count_features(t["type_ptr"], 4),
                          R.tiled_rows(R.count_features(base["type_ptr"], 4), t["bs"]))
    assert R.nan_share(t)[0] > 0 and R.nan_share(t)[1] > 0


def test_single_pair_and_empty_pair():
    c = R.make_case(R.single_pair_counts(4), D_HOST, 4, "pm3")
    a, b = R.direct_softmax(c), R.merged_records(c)
    assert float(np.abs(a - b).max()) <= (R.record_rounding_bound(c) * (1 + 1e-3) + 1e-12).max()
    e = R.make_case(np.zeros((3, 2), np.int64), D_HOST, 4, "pm3")
    assert np.array_equal(R.merged_records(e), np.tile(e["att_bias"], (2, 1)))
    assert np.array_equal(R.direct_softmax(e), np.tile(e["att_bias"], (2, 1)))
    assert np.isnan(e["part"]).all() and np.isnan(e["bnd"]).all()
    f = R.features(e, R.merged_records(e))
    assert np.array_equal(f[:, D_HOST:], np.zeros((2, 4)))
    assert np.allclose(f[0, :D_HOST], R.layer_norm(e["att_bias"], e["ln_g"], e["ln_b"]), rtol=0, atol=1e-15)


def test_tail_restatement_against_its_parts():
    """tail_ref on hand-made input: identity-like weights make every stage readable."""
    D, nc = 32, 4
    w = R.tail_weights(D, nc)
    rng = np.random.default_rng(5)
    rows, cnt, r_e = rng.standard_normal((7, D)), rng.integers(0, 50, (7, nc)).astype(np.float64), rng.random((7, D))
    logit, prob = R.tail_ref(rows, cnt, r_e, w)
    # the same in scalar loops
    for i in range(7):
        x = np.concatenate([rows[i], cnt[i]])
        v = np.array([sum(w["w_p0"][o, k] * x[k] for k in range(D + nc)) + w["b_p0"][o] for o in range(D + nc)])
        mu = v.mean()
        y = (v - mu) / np.sqrt(((v - mu) ** 2).mean() + 1e-5) * w["lnB_g"] + w["lnB_b"]
        z = np.concatenate([r_e[i], np.maximum(y, 0)])
        h = w["A"] @ z + w["c"]
        s = float(np.maximum(h, 0) @ w["w_dot"] + w["b_dot"][0])
        assert abs(s - logit[i]) <= 1e-12 * max(1.0, abs(s))
        assert abs(prob[i] - 1 / (1 + np.exp(-s))) <= 1e-15
