"""threshold_profile on the host: the numpy restatement against the oracle's select_nodes for every type and threshold
of the grid (boundary thresholds included), mode "cn", the argument checks, entries() and suggest_thresholds."""
import numpy as np
import pytest
import torch

import lpformer_amd
from lpformer_amd import _lib, graph
from lpformer_amd.threshold_profile import (ThresholdProfile, check_thresholds, profile_reference, suggest_thresholds,
                                            threshold_profile)
from tests import threshold_profile_cases as TC

TAGS = ("cn", "onehop", "non1hop")


@pytest.fixture(scope="module", params=list(TC.CASES))
def case(request):
    return TC.CASES[request.param]()


@pytest.fixture(scope="module")
def profile(case):
    return profile_reference(case.adj, case.ppr, torch.from_numpy(case.pairs), case.grid, per_pair=True)


def test_inputs_hold_the_cases_they_claim(case):
    a, b = case.pairs
    assert case.pairs.shape == (2, 257)
    assert (a == b).any() and np.array_equal(case.pairs[:, 0], case.pairs[:, -1])          # a == b; a duplicated pair
    keys = set(r * case.n + c for r, c in
               zip(np.repeat(np.arange(case.n), np.diff(case.adj.rowptr)).tolist(), case.adj.col.tolist()))
    assert sum((int(x) * case.n + int(y)) in keys for x, y in zip(a, b)) >= 96            # existing edges
    if case.hub is not None:
        deg = np.diff(case.adj.rowptr)
        assert deg[case.hub] >= 80 and deg[case.iso] == 0
        pairs = set(zip(a.tolist(), b.tolist()))
        assert (case.hub, case.hub) in pairs and (case.iso, case.iso) in pairs
        assert any(x == case.hub and deg[y] == 1 for x, y in pairs)
    # the grid: 0, two ordinary values and the two boundary values taken from the oracle's round-tripped output
    assert case.grid.size == 5 and case.grid[0] == 0 and np.all(np.diff(case.grid) > 0)
    assert all(np.float32(t) in case.grid for t in TC.ORDINARY + case.special)
    # no stored PPR value has two different round trips (tests/threshold_profile_cases.py: none can in fp32)
    assert TC.round_trips_differ(case) == 0


def test_boundary_thresholds_need_the_round_trip(case, profile):
    """At each boundary threshold at least one entry is selected only because its ROUND-TRIPPED value reaches the
    threshold: comparing the raw stored values gives a smaller count."""
    sel_all = TC.O.select_nodes(case.pairs, (case.adj.rowptr, case.adj.col.astype(np.int64)),
                                (case.ppr.rowptr, case.ppr.col.astype(np.int64), case.ppr.val), (0.0, 0.0, 0.0),
                                n=case.n)
    for t, (tag, th) in enumerate(zip(("onehop", "cn"), case.special)):
        ix, pa, pb = sel_all[tag]
        raw_a = TC.raw_ppr(case.ppr, case.pairs[0][ix[0]], ix[1])
        raw_b = TC.raw_ppr(case.ppr, case.pairs[1][ix[0]], ix[1])
        th = np.float32(th)
        by_raw = int(np.count_nonzero((raw_a >= th) & (raw_b >= th)))
        j = int(np.flatnonzero(case.grid == th)[0])
        assert int(profile.total[1 - t, j]) == int(np.count_nonzero((pa >= th) & (pb >= th))) > by_raw


@pytest.mark.parametrize("t", [0, 1, 2])
def test_per_pair_equals_the_oracle_selection(case, profile, t):
    """Vary one type's threshold over the grid, hold the other two at a grid value: the bincount of select_nodes."""
    hold = float(case.grid[2])
    assert profile.per_pair.shape == (257, 3, 5) and profile.per_pair.dtype == torch.int32
    for j, th in enumerate(case.grid.tolist()):
        triple = [hold] * 3
        triple[t] = th
        want = case.oracle(tuple(triple))[TAGS[t]]
        np.testing.assert_array_equal(profile.per_pair[:, t, j].numpy(), want, err_msg=f"{case.name} {TAGS[t]} {th}")


def test_reductions_follow_from_per_pair(case, profile):
    pp = profile.per_pair.numpy().astype(np.int64)
    np.testing.assert_array_equal(profile.total.numpy(), pp.sum(axis=0))
    np.testing.assert_array_equal(profile.max_per_pair.numpy(), pp.max(axis=0))
    np.testing.assert_array_equal(profile.nonempty.numpy(), (pp > 0).sum(axis=0))
    assert profile.total.dtype == profile.nonempty.dtype == torch.int64 and profile.max_per_pair.dtype == torch.int32
    assert profile.n_pairs == 257 and profile.thresholds.dtype == torch.float32
    assert np.all(np.diff(pp, axis=2) <= 0)                      # a larger threshold never selects more
    assert pp[:, 1].sum() > 0 and pp[:, 2].sum() > 0
    slim = profile_reference(case.adj, case.ppr, case.pairs.T.copy(), case.grid)       # [P, 2] layout, no per_pair
    assert slim.per_pair is None and torch.equal(slim.total, profile.total)
    assert torch.equal(slim.max_per_pair, profile.max_per_pair) and torch.equal(slim.nonempty, profile.nonempty)


def test_mode_cn_against_the_oracle(case):
    prof = profile_reference(case.adj, case.ppr, case.pairs, case.grid, mode_cn=True, per_pair=True)
    for j, th in enumerate(case.grid.tolist()):
        sel = case.oracle((th, 1, 1))
        assert set(sel) == {"cn"}
        np.testing.assert_array_equal(prof.per_pair[:, 0, j].numpy(), sel["cn"])
    assert not prof.per_pair[:, 1:].any() and not prof.total[1:].any()


def test_ids_out_of_range_count_nothing(case):
    bad = np.array([[-1, case.n, 0, 3], [2, 1, case.n + 5, -7]])
    pairs = np.concatenate([case.pairs[:, :5], bad, case.pairs[:, 5:9]], axis=1)
    prof = profile_reference(case.adj, case.ppr, pairs, case.grid, per_pair=True)
    good = profile_reference(case.adj, case.ppr, case.pairs[:, :9], case.grid, per_pair=True)
    assert not prof.per_pair[5:9].any()
    assert torch.equal(prof.per_pair[[0, 1, 2, 3, 4, 9, 10, 11, 12]], good.per_pair)
    assert torch.equal(prof.total, good.total) and prof.n_pairs == 13


def test_public_entry_runs_the_restatement_without_a_gpu(case, profile, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)    # (with a GPU present host containers are uploaded)
    got = threshold_profile((case.adj, case.ppr), torch.from_numpy(case.pairs), case.grid, per_pair=True)
    assert torch.equal(got.per_pair, profile.per_pair) and torch.equal(got.total, profile.total)
    empty = threshold_profile((case.adj, case.ppr), torch.zeros(2, 0, dtype=torch.int64), per_pair=True)
    assert empty.n_pairs == 0 and empty.per_pair.shape == (0, 3, 6) and not empty.total.any()
    assert empty.thresholds.tolist() == np.float32([0, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1]).tolist()


def _tiny():
    return (graph.CSR(np.array([0, 1, 2, 2], np.int64), np.array([1, 0], np.int32), None, 3),
            graph.CSR(np.array([0, 1, 2, 3], np.int64), np.array([0, 1, 2], np.int32), np.ones(3, np.float32), 3))


@pytest.mark.parametrize("thresholds", [(), tuple(range(33)), (0.0, -1e-3), (0.0, float("nan")), (0.0, float("inf")),
                                        (1e-3, 1e-3), (0.1, np.float32(0.1)), (1e-3, 0.0, 1e-3)])
def test_rejects_bad_thresholds(thresholds):
    with pytest.raises(ValueError):
        check_thresholds(thresholds)
    with pytest.raises(ValueError):
        threshold_profile(_tiny(), torch.zeros(2, 3, dtype=torch.int64), thresholds)


def test_thresholds_are_cast_and_sorted():
    th = check_thresholds([1e-2, 0, 1e-4])
    assert th.dtype == np.float32 and th.tolist() == np.float32([0, 1e-4, 1e-2]).tolist()
    assert check_thresholds(list(range(32))).size == 32


def test_rejects_bad_edges_and_sources():
    src = _tiny()
    with pytest.raises(ValueError):
        threshold_profile(src, torch.zeros(2, 3))                                   # float edges
    with pytest.raises(ValueError):
        threshold_profile(src, torch.zeros(3, 3, dtype=torch.int64))
    with pytest.raises(ValueError):
        threshold_profile(src, torch.zeros(2, 3, dtype=torch.int64), chunk=0)
    with pytest.raises(TypeError):
        threshold_profile(src[0], torch.zeros(2, 3, dtype=torch.int64))
    with pytest.raises(ValueError):
        threshold_profile((src[0], src[0]), torch.zeros(2, 3, dtype=torch.int64))   # a PPR matrix without values


def _hand_made():
    th = torch.tensor([0.0, 1e-3, 1e-2, 1e-1], dtype=torch.float32)
    total = torch.tensor([[40, 30, 20, 10], [400, 200, 100, 0], [4000, 1000, 50, 10]], dtype=torch.int64)
    return ThresholdProfile(th, total, torch.zeros(3, 4, dtype=torch.int32), torch.zeros(3, 4, dtype=torch.int64),
                            None, 10)


def test_entries_on_a_hand_made_profile():
    p = _hand_made()
    assert p.entries(0, 1e-3, 1e-2) == (40, 200, 50)
    assert p.entries(1e-1, 0.0, 1e-1) == (10, 400, 10)
    assert p.entries(0, 1e-2, 1) == (40, 100, 0)          # thresh_non1hop == 1: mask mode "1-hop"
    assert p.entries(1e-3, 1, 1) == (30, 0, 0)            # ... and thresh_1hop == 1: mask mode "cn"
    with pytest.raises(ValueError):
        p.entries(0, 1, 1e-2)                             # 1 is an ordinary one-hop threshold here, and not in the grid
    with pytest.raises(ValueError):
        p.entries(0, 5e-3, 1e-2)
    assert "pairs" in p.table() and len(p.table().splitlines()) == 2 + 4


def test_suggest_thresholds_on_a_hand_made_profile():
    p = _hand_made()
    f = lambda x: float(np.float32(x))    # noqa: E731
    # strictest point: (10 + 0 + 10) / 10 = 2 entries per pair
    s = suggest_thresholds(p, 1.0)
    assert not s["within_budget"] and s["entries_per_pair"] == 2.0
    assert (s["thresh_cn"], s["thresh_1hop"], s["thresh_non1hop"]) == (f(1e-1),) * 3
    # budget 20: >1-hop relaxes to 1e-2 (10 + 0 + 50 = 60; 1e-3 would give 1010), then one-hop to 1e-2 (160; 1e-3:
    # 260), then common neighbours to 0 (190)
    s = suggest_thresholds(p, 20.0)
    assert (s["thresh_cn"], s["thresh_1hop"], s["thresh_non1hop"]) == (0.0, f(1e-2), f(1e-2))
    assert s["within_budget"] and s["entries_per_pair"] == 19.0
    # everything fits
    s = suggest_thresholds(p, 1e9)
    assert (s["thresh_cn"], s["thresh_1hop"], s["thresh_non1hop"]) == (0.0, 0.0, 0.0) and s["entries_per_pair"] == 444.0
    # a fixed >1-hop switch-off leaves its share to the others
    s = suggest_thresholds(p, 20.0, fixed={"thresh_non1hop": 1})
    assert (s["thresh_cn"], s["thresh_1hop"], s["thresh_non1hop"]) == (0.0, f(1e-2), 1) and s["entries_per_pair"] == 14.0
    with pytest.raises(ValueError):
        suggest_thresholds(p, 20.0, fixed={"thresh": 0})
    with pytest.raises(ValueError):
        suggest_thresholds(p, -1.0)


def test_exports_and_abi():
    assert {"threshold_profile", "suggest_thresholds", "ThresholdProfile"} <= set(lpformer_amd.__all__)
    assert _lib.ABI_VERSION == 16 and "lpf_threshold_profile" in _lib.HIP_PROTOTYPES
