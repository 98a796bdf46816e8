"""The numpy restatement of random_walks (lpformer_amd/random_walks.py) against the contract written out walk by walk
in Python integers, its own properties, the node2vec distribution on a hand graph, and the torch helpers.  No GPU."""
import bisect

import numpy as np
import pytest
import torch

from lpformer_amd import graph, negatives
from lpformer_amd.random_walks import (Walks, node2vec_embeddings, random_walks, walk_pairs, walk_thresholds,
                                       walks_reference)
from tests import random_walks_cases as RC

G, M64 = negatives.G, (1 << 64) - 1


def _host(csr, starts, **kw):
    """Through the public function where it takes the host path (no GPU present), else the restatement itself."""
    fn = walks_reference if torch.cuda.is_available() else random_walks
    out = fn(csr, None if starts is None else torch.as_tensor(starts), **kw)
    assert isinstance(out, Walks) and not out.walks.is_cuda and not out.forced.is_cuda
    assert out.walks.dtype == torch.int32 and out.forced.dtype == torch.int32
    return out.walks.numpy(), out.forced.numpy()


def _literal_walk(csr, start, walk_id, L, thr, T, seed):
    """One walk by the contract's seven steps, in Python integers."""
    n, rowptr, col = int(csr.n), csr.rowptr, csr.col
    if not 0 <= start < n:
        return [-1] * (L + 1), 0
    key = negatives.mix64(seed + G * (walk_id + 1))

    def u(j):
        return negatives.mix64(key + G * (j + 1))
    second = any(t != 1 << 63 for t in thr)
    walk, forced = [start], 0
    for t in range(1, L + 1):
        cur = walk[-1]
        r0, d = int(rowptr[cur]), int(rowptr[cur + 1] - rowptr[cur])
        if d == 0:
            walk.append(cur)
            continue
        for a in range(T):
            j = 2 * ((t - 1) * T + a)
            x = int(col[r0 + ((u(j) * d) >> 64)])
            if t == 1 or d == 1 or not second:
                break
            prev = walk[-2]
            row = col[rowptr[prev]:rowptr[prev + 1]]
            i = bisect.bisect_left(row, x)
            cls = 0 if x == prev else (1 if i < len(row) and row[i] == x else 2)
            if (u(j + 1) >> 1) < thr[cls]:
                break
        else:
            forced += 1
        walk.append(x)
    return walk, forced


def test_thresholds():
    assert walk_thresholds(0.25, 4) == (1 << 63, 1 << 61, 1 << 59)
    assert walk_thresholds(1, 1) == (1 << 63,) * 3
    assert walk_thresholds(4, 0.25) == (1 << 59, 1 << 61, 1 << 63)
    assert walk_thresholds(0.5, 2) == (1 << 63, 1 << 62, 1 << 61)
    r, c, o = walk_thresholds(3.0, 0.7)                       # floor of exact fractions of the doubles
    assert o == 1 << 63 and c == (1 << 63) * 3152519739159347 // (1 << 52) and r == c // 3
    assert all(isinstance(t, int) for t in (r, c, o))
    for bad in ((0, 1), (1, -2.0), (float("nan"), 1), (1, float("inf"))):
        with pytest.raises(ValueError):
            walk_thresholds(*bad)


@pytest.mark.parametrize("name", RC.NAMES)
@pytest.mark.parametrize("pq", RC.PQ)
def test_restatement_equals_the_literal_contract(name, pq):
    """A slice of the shared reference (bad starts and isolated nodes included) against the walk written out in Python
    integers; at max_tries = 2 the forced counts as well."""
    csr, starts = RC.case(name).csr, RC.starts(name)
    W = 2 * starts.size
    pick = np.unique(np.concatenate([np.arange(0, W, 97), np.arange(RC.case(name).n - 3, RC.case(name).n + 10)]))
    for T in (64, 2):
        walks, forced = RC.reference(name, *pq, T)
        assert walks.shape == (W, RC.LENGTH + 1) and forced.shape == (W,)
        thr = walk_thresholds(*pq)
        for w in pick:
            want, f = _literal_walk(csr, int(starts[w % starts.size]), int(w), RC.LENGTH, thr, T, RC.SEED)
            assert walks[w].tolist() == want and forced[w] == f, (name, pq, T, w)


@pytest.mark.parametrize("name", RC.NAMES)
def test_moves_follow_stored_entries_and_isolated_nodes_stay(name):
    case, starts = RC.case(name), RC.starts(name)
    deg = np.diff(case.csr.rowptr)
    keys = negatives._entry_keys(case.csr)
    for pq in RC.PQ:
        walks, forced = RC.reference(name, *pq)
        bad = np.tile((starts < 0) | (starts >= case.n), 2)
        assert (walks[bad] == -1).all() and (forced[bad] == 0).all() and bad.sum() == 8
        good = walks[~bad].astype(np.int64)
        assert (good[:, 0] == np.tile(starts, 2)[~bad]).all() and (good >= 0).all() and (good < case.n).all()
        a, b = good[:, :-1].reshape(-1), good[:, 1:].reshape(-1)
        stored = negatives._stored(keys, case.n, a, b)
        assert (stored | ((deg[a] == 0) & (a == b))).all()
        lonely = good[deg[good[:, 0]] == 0]
        assert (lonely == lonely[:, :1]).all()
        if name == "H":
            assert lonely.shape[0] >= 100                      # nodes 3950 .. 3999, twice
        if pq == (1.0, 1.0):
            assert not forced.any()


@pytest.mark.parametrize("name", ("S", "Kloops"))
def test_first_order_walks_equal_the_one_line_formula(name):
    case, starts = RC.case(name), RC.starts(name)
    walks, _ = RC.reference(name, 1.0, 1.0)
    rowptr, col = case.csr.rowptr, case.csr.col
    ok = np.flatnonzero(walks[:, 0] >= 0)
    key = negatives.draw_key(RC.SEED, ok.astype(np.uint64))
    cur = walks[ok, 0].astype(np.int64)
    for t in range(1, RC.LENGTH + 1):
        d = rowptr[cur + 1] - rowptr[cur]
        u = negatives.draw_u(key, np.uint64(2 * (t - 1) * 64))
        idx = np.array([(int(x) * int(y)) >> 64 for x, y in zip(u, d)], dtype=np.int64)
        cur = np.where(d > 0, col[np.minimum(rowptr[cur] + idx, col.size - 1)], cur)
        np.testing.assert_array_equal(walks[ok, t], cur)


def test_chunking_by_walk_base_changes_nothing():
    case, starts = RC.case("H"), RC.starts("H")
    walks, forced = RC.reference("H", 0.25, 4.0)
    both = np.tile(starts, 2)
    for lo, hi in ((0, 1000), (1000, 4001), (4001, both.size)):
        w, f = _host(case.csr, both[lo:hi].copy(), length=RC.LENGTH, p=0.25, q=4.0, seed=RC.SEED, walk_base=lo)
        np.testing.assert_array_equal(w, walks[lo:hi])
        np.testing.assert_array_equal(f, forced[lo:hi])
    w, _ = _host(case.csr, None, length=3, seed=1)             # starts=None: every node
    assert w.shape == (case.n, 4) and (w[:, 0] == np.arange(case.n)).all()
    w2, _ = _host(case.csr, None, length=3, seed=2)
    assert not np.array_equal(w, w2)


@pytest.mark.parametrize("pq", tuple(RC.BIAS_WANT))
def test_second_step_frequencies_are_node2vec(pq):
    """65,536 walks from node 0 of the hand graph; among those that went to node 1, the second step's frequencies lie
    within 4 binomial standard deviations of the node2vec probabilities.  A pure function of the seed: not flaky."""
    walks, forced = _host(RC.bias_graph(), np.zeros(RC.BIAS_WALKS, np.int64), length=2, p=pq[0], q=pq[1], seed=0)
    z = RC.bias_z(walks, RC.BIAS_WANT[pq])
    print(pq, "|z| per target", z.round(2), "forced", int(forced.sum()))
    assert (z < 4.0).all()


def test_max_tries_forces_the_last_candidate():
    case = RC.case("S")
    _, forced = RC.reference("S", 4.0, 0.25, 2)
    _, relaxed = RC.reference("S", 4.0, 0.25, 64)
    print("forced steps at max_tries 2:", int(forced.sum()), "at 64:", int(relaxed.sum()), "of", forced.size * RC.LENGTH)
    assert forced.sum() > 0 and forced.max() <= RC.LENGTH and forced.sum() > relaxed.sum()
    assert case.n == 3000


def test_walk_pairs_hand_example():
    walks = torch.tensor([[0, 1, 2, 3], [-1, -1, -1, -1], [4, 5, 6, 7]], dtype=torch.int32)
    got = walk_pairs(walks, 3)
    assert got.dtype == torch.int64 and got.tolist() == [[0, 0, 1, 1, 4, 4, 5, 5], [1, 2, 2, 3, 5, 6, 6, 7]]
    assert walk_pairs(walks, 4).tolist() == [[0, 0, 0, 4, 4, 4], [1, 2, 3, 5, 6, 7]]
    assert walk_pairs(walks.t().contiguous().t(), 2).tolist() == [[0, 1, 2, 4, 5, 6], [1, 2, 3, 5, 6, 7]]   # a view
    assert walk_pairs(walks[1:2], 2).shape == (2, 0)
    for bad in (1, 5):
        with pytest.raises(ValueError):
            walk_pairs(walks, bad)


def test_argument_checks():
    csr = RC.bias_graph()
    for kw in ({"length": 0}, {"length": 2, "max_tries": 0}, {"length": 2, "p": 0.0}, {"length": 2, "walk_base": -1},
               {"length": 2, "walks_per_node": 0}):
        with pytest.raises(ValueError):
            walks_reference(csr, None, seed=0, **kw)
    with pytest.raises(ValueError):
        random_walks(csr, None, length=2, seed=0, form="fast")
    with pytest.raises(ValueError):
        walks_reference(csr, torch.tensor([0.5]), length=2, seed=0)
    empty = walks_reference(graph.CSR(np.zeros(1, np.int64), np.zeros(0, np.int32), None, 0), torch.tensor([0, 3]),
                            length=2, seed=0)
    assert empty.walks.tolist() == [[-1] * 3] * 2 and empty.forced.tolist() == [0, 0]


def test_host_csr_without_a_gpu_takes_the_restatement_path(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)     # (where there is one: as if there were none)
    case = RC.case("C")
    starts = torch.from_numpy(RC.starts("C").copy())
    out = random_walks(case.csr, starts, length=RC.LENGTH, walks_per_node=2, p=4.0, q=0.25, seed=RC.SEED)
    walks, forced = RC.reference("C", 4.0, 0.25)
    assert not out.walks.is_cuda
    np.testing.assert_array_equal(out.walks.numpy(), walks)
    np.testing.assert_array_equal(out.forced.numpy(), forced)
    emb, losses = node2vec_embeddings(case.csr, 8, walk_length=6, context=3, walks_per_node=1, batch_walks=128, lr=0.05)
    assert emb.shape == (case.n, 8) and emb.dtype == torch.float32 and not emb.is_cuda and len(losses) == 1
    assert torch.isfinite(emb).all() and np.isfinite(losses[0])
