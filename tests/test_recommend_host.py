"""CPU checks of top-K recommendation: the chunk planner, recommendation_metrics against a plain Python loop, and the
argument checks of recommend() that need no device."""
import math

import numpy as np
import pytest
import torch

import lpformer_amd
from lpformer_amd import evaluate as E
from lpformer_amd.recommend import MAX_K, Recommendations, _check_args, plan_chunks


def _check_plan(counts, max_pairs, chunks):
    S = len(counts)
    if S == 0:
        assert chunks == []
        return
    assert chunks[0][0] == 0 and chunks[-1][1] == S
    for (lo, hi), (lo2, _) in zip(chunks, chunks[1:]):
        assert hi == lo2
    for lo, hi in chunks:
        assert hi > lo
        total = int(np.sum(counts[lo:hi]))
        assert total <= max_pairs or hi - lo == 1, (lo, hi, total)
    # greedy: a chunk could not have taken the next source
    for (lo, hi), (_, hi2) in zip(chunks, chunks[1:]):
        assert int(np.sum(counts[lo:hi + 1])) > max_pairs


@pytest.mark.parametrize("seed", range(5))
def test_plan_chunks_respects_max_pairs(seed):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 50, size=300)
    for max_pairs in (1, 7, 49, 50, 200, 10_000):
        _check_plan(counts, max_pairs, plan_chunks(counts, max_pairs))
    assert plan_chunks(counts, 1 << 24) == [(0, 300)]


def test_plan_chunks_oversize_source_alone():
    counts = np.array([3, 100, 2, 2, 250, 1])
    chunks = plan_chunks(counts, 10)
    assert chunks == [(0, 1), (1, 2), (2, 4), (4, 5), (5, 6)]
    _check_plan(counts, 10, chunks)
    assert plan_chunks([500], 10) == [(0, 1)]


def test_plan_chunks_empty_and_zero_counts():
    assert plan_chunks([], 10) == []
    assert plan_chunks(np.zeros(0, np.int64), 1) == []
    assert plan_chunks([0, 0, 0], 1) == [(0, 3)]
    chunks = plan_chunks([0, 5, 0, 0, 5, 0], 5)
    assert chunks == [(0, 4), (4, 6)]
    with pytest.raises(ValueError):
        plan_chunks([1, 2], 0)
    with pytest.raises(ValueError):
        plan_chunks([1, -2], 5)


def _loop_metrics(ids, sources, held_out, ks):
    targets = {}
    for u, v in held_out:
        targets.setdefault(int(u), set()).add(int(v))
    out = {}
    rows = [s for s in range(len(sources)) if targets.get(int(sources[s]))]
    for k in ks:
        rec, hit = [], []
        for s in rows:
            t = targets[int(sources[s])]
            top = set(int(x) for x in ids[s][:k] if x >= 0)
            n = len(top & t)
            rec.append(n / len(t))
            hit.append(1.0 if n else 0.0)
        out[f"recall@{k}"] = float(np.mean(rec)) if rows else float("nan")
        out[f"hit@{k}"] = float(np.mean(hit)) if rows else float("nan")
    out["n_sources"] = len(rows)
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for key in a:
        if isinstance(b[key], float) and math.isnan(b[key]):
            assert math.isnan(a[key]), key
        else:
            assert a[key] == pytest.approx(b[key], abs=1e-12), key


def _rec(ids):
    ids = torch.as_tensor(ids, dtype=torch.int64)
    return Recommendations(ids, torch.zeros(ids.shape), (ids >= 0).sum(1), (ids >= 0).sum(1))


def test_recommendation_metrics_hand_cases():
    ks = (1, 2, 3, 5)
    # source 0: targets {4, 7}; top = 7, 3, 4 -> hit@1, recall@1 = 1/2, recall@3 = 1
    # source 1: no targets (left out); source 2: all hits; source 0 again (duplicate row), padded: k > count
    ids = [[7, 3, 4], [1, 2, 3], [5, 6, -1], [4, -1, -1]]
    sources = [0, 1, 2, 0]
    held = [[0, 4], [0, 7], [2, 5], [2, 6], [0, 7], [9, 1]]
    got = E.recommendation_metrics(_rec(ids), torch.tensor(sources), torch.tensor(held), ks=ks)
    want = _loop_metrics(ids, sources, held, ks)
    _same(got, want)
    assert got["n_sources"] == 3
    assert got["recall@3"] == pytest.approx((1.0 + 1.0 + 0.5) / 3)
    assert got["hit@1"] == pytest.approx(1.0)


def test_recommendation_metrics_no_targets():
    got = E.recommendation_metrics(_rec([[1, 2], [3, -1]]), torch.tensor([0, 1]), torch.tensor([[5, 0]]), ks=(1, 2))
    assert got["n_sources"] == 0 and all(math.isnan(got[k]) for k in ("recall@1", "hit@1", "recall@2", "hit@2"))
    empty = E.recommendation_metrics(_rec([[1, 2]]), torch.tensor([0]), torch.zeros((0, 2), dtype=torch.int64), ks=(1,))
    assert empty["n_sources"] == 0 and math.isnan(empty["recall@1"])


def test_recommendation_metrics_random_against_loop():
    rng = np.random.default_rng(3)
    S, K, n = 60, 12, 40
    ids = rng.integers(-1, n, size=(S, K))
    ids[:, 3] = ids[:, 1]          # repeated ids count once
    sources = rng.integers(0, n, size=S)
    held = rng.integers(0, n, size=(150, 2))
    ks = (1, 5, 12, 50)            # 50 > K: all columns
    got = E.recommendation_metrics(_rec(ids), torch.from_numpy(sources), torch.from_numpy(held), ks=ks)
    _same(got, _loop_metrics(ids, sources, held, ks))


def test_argument_checks_without_device():
    src = torch.tensor([0, 1, 2])
    for bad_k in (0, -1, MAX_K + 1, 2.5, True):
        with pytest.raises(ValueError):
            _check_args(src, bad_k, "ppr")
    for mode in ("PPR", "two-hop", ""):
        with pytest.raises(ValueError):
            _check_args(src, 10, mode)
    with pytest.raises(TypeError):
        _check_args(torch.tensor([0.0, 1.0]), 10, "ppr")
    with pytest.raises(TypeError):
        _check_args(torch.tensor([True, False]), 10, "all")
    with pytest.raises(ValueError):
        _check_args(torch.tensor([[0, 1]]), 10, "all")
    with pytest.raises(ValueError):
        _check_args(src, 10, torch.zeros((2, 4), dtype=torch.int64))   # one row per source
    with pytest.raises(TypeError):
        _check_args(src, 10, torch.zeros((3, 4)))
    s, c = _check_args(src, MAX_K, torch.zeros((3, 4), dtype=torch.int32))
    assert c.shape == (3, 4) and s.shape == (3,)
    # the public entry point runs the same checks before it touches the model
    with pytest.raises(ValueError):
        lpformer_amd.recommend(None, None, src, k=0)
    with pytest.raises(ValueError):
        lpformer_amd.recommend(None, None, src, candidates="bogus")
    with pytest.raises(TypeError):
        lpformer_amd.recommend(None, None, torch.tensor([0.5]))
