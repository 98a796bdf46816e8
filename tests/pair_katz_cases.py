"""Pair batches and the scipy reference shared by tests/test_pair_katz_host.py and tests/test_gpu_pair_katz.py, on the
graphs S, H and C of tests/pair_distance_cases.py (unchanged).  Uniform random pairs are almost all zero here (on S only
0.7 % of them have W_3 > 0), so an all-zero kernel would nearly pass them: most of a batch is built from walks.  Every
reference is computed once per process and handed out read-only."""
from functools import lru_cache
from typing import NamedTuple

import numpy as np
import scipy.sparse as sp

from lpformer_amd import graph
from tests import pair_distance_cases as PC

MAX_LENS = (1, 2, 3, 4)
WALK_PAIRS = 250                              # per walk length 1 .. 4
RUN = 256                                     # partners of the HeaRT-shaped run


class Case(NamedTuple):
    n: int
    A: sp.csr_matrix                          # binary, symmetric, no diagonal
    csr: graph.CSR
    pairs: np.ndarray                         # int64 [2, P]
    hub: int
    edges: slice                              # the positions of the 64 stored edges in ``pairs``


def _row_counts(A, A2, a, b) -> np.ndarray:
    Ab, A2a, A2b = A[b], A2[a], A2[b]
    w1 = np.asarray(A[a, b]).ravel()
    w2 = np.asarray(A2[a, b]).ravel()
    w3 = np.asarray(A2a.multiply(Ab).sum(axis=1)).ravel()
    w4 = np.asarray(A2a.multiply(A2b).sum(axis=1)).ravel()
    out = np.stack([w1, w2, w3, w4], axis=1)
    assert out.max(initial=0) < 2.0 ** 53
    return out.astype(np.int64)


def walk_counts(A, a, b) -> np.ndarray:
    """int64 [P, 4]: W_1 = A[a, b], W_2 = A2[a, b], W_3 = sum A2[a] * A[b], W_4 = sum A2[a] * A2[b] of in-range pairs
    by scipy, A2 = A @ A in float64 (exact below 2^53)."""
    A = A.astype(np.float64)
    return _row_counts(A, (A @ A).tocsr(), a, b)


def scipy_walks(A, pairs) -> np.ndarray:
    """int64 [P, 4] of any pairs: an id outside [0, n) gives 0 for every l."""
    a, b = np.asarray(pairs)
    n = A.shape[0]
    ok = (a >= 0) & (a < n) & (b >= 0) & (b < n)
    out = np.zeros((a.size, 4), np.int64)
    out[ok] = walk_counts(A, a[ok], b[ok])
    return out


class WithoutEdge:
    """The same computation on a copy of A without one edge at a time.  The copy is made once; per pair its stored
    entries (a, b) and (b, a) are set to 0, the rows a and b of A2 = A @ A are formed from it, and the entries are put
    back (a stored zero adds nothing to a product)."""

    def __init__(self, A):
        self.B = A.astype(np.float64).tocsr(copy=True)
        self.B.sort_indices()

    def _at(self, r, c):
        lo, hi = self.B.indptr[r], self.B.indptr[r + 1]
        k = lo + int(np.searchsorted(self.B.indices[lo:hi], c))
        assert k < hi and self.B.indices[k] == c
        return k

    def counts(self, a: int, b: int) -> np.ndarray:
        """int64 [4]: W_1 .. W_4 of the stored edge (a, b) without that edge."""
        B = self.B
        at = [self._at(a, b), self._at(b, a)]
        B.data[at] = 0.0
        try:
            rows = B[[a, b]]
            two = (rows @ B).tocsr()
            w = [B[a, b], two[0, b], two[0].multiply(rows[1]).sum(), two[0].multiply(two[1]).sum()]
        finally:
            B.data[at] = 1.0
        assert max(w) < 2.0 ** 53
        return np.array(w, np.float64).astype(np.int64)


def _random_walks(A, rng, steps: int, count: int) -> np.ndarray:
    """[2, count]: (u, the endpoint of a random walk of ``steps`` stored entries from u)."""
    indptr, indices = A.indptr, A.indices
    deg = np.diff(indptr)
    u = rng.choice(np.flatnonzero(deg > 0), count)
    v = u.copy()
    for _ in range(steps):
        v = indices[indptr[v] + rng.integers(0, deg[v])]
    return np.stack([u, v]).astype(np.int64)


def _batch(base: PC.Case, seed: int, hub: int):
    A, n = base.A, base.n
    rng = np.random.default_rng(seed)
    deg = np.diff(A.indptr)
    parts = [_random_walks(A, rng, k, WALK_PAIRS) for k in MAX_LENS]
    parts.append(rng.integers(0, n, (2, 256)))
    r, c = A.nonzero()
    pick = rng.choice(r.size, 64, replace=False)
    lo = sum(p.shape[1] for p in parts)
    parts.append(np.stack([r[pick], c[pick]]).astype(np.int64))
    partners = rng.choice(np.setdiff1d(np.arange(n), [hub]), RUN, replace=False)
    run = np.stack([np.full(RUN, hub), partners])
    parts += [run, run[::-1]]
    same = [int(np.argmax(deg)), int(np.flatnonzero(deg == deg[deg > 0].min())[0])]
    same += [int(v) for v in np.flatnonzero(deg == 0)[:1]]          # (graph C has no isolated node)
    parts.append(np.array([same, same]))
    parts.append(np.array([[-1, 5, n, -1], [5, n, n, -1]]))
    pairs = np.ascontiguousarray(np.concatenate(parts, axis=1), dtype=np.int64)
    pairs.setflags(write=False)
    return Case(n, A, base.csr, pairs, hub, slice(lo, lo + 64))


@lru_cache(maxsize=None)
def case(name: str) -> Case:
    base = PC.CASES[name]()
    hub = {"S": int(np.argmax(np.diff(base.A.indptr))), "H": 0, "C": 0}[name]
    # (H: the seed is one at which the share condition below holds; most seeds give 22 - 24 % where it asks for 25 %)
    return _batch(base, {"S": 21, "H": 25, "C": 23}[name], hub)


@lru_cache(maxsize=None)
def exact(name: str) -> np.ndarray:
    """int64 [P, 4], read-only."""
    c = case(name)
    w = scipy_walks(c.A, c.pairs)
    w.setflags(write=False)
    _check_condition(name, w)
    return w


@lru_cache(maxsize=None)
def exact_ignore_direct(name: str) -> np.ndarray:
    """int64 [P, 4] under ignore_direct: every pair that is a stored entry is recomputed on a per-pair copy of A
    without that edge; every other pair is unchanged."""
    c = case(name)
    w = exact(name).copy()
    a, b = c.pairs
    ok = (a >= 0) & (a < c.n) & (b >= 0) & (b < c.n)
    cut = WithoutEdge(c.A)
    for i in np.flatnonzero(ok & (w[:, 0] > 0)):
        w[i] = cut.counts(int(a[i]), int(b[i]))
    w.setflags(write=False)
    return w


def _shares(w):
    return float((w[:, 2] > 0).mean()), float(((w[:, 3] > w[:, 2]) & (w[:, 2] > 0)).mean())


def shares(name: str):
    """(share of the pairs with W_3 > 0, share with W_4 > W_3 > 0)."""
    return _shares(exact(name))


def _check_condition(name: str, w) -> None:
    """What keeps a trivial kernel from passing.  On every graph the walk-built pairs of length l have W_l >= 1, by
    construction: 250 non-zero targets in every column.  On H and C at least half of the pairs have W_3 > 0 and at least
    a quarter have W_4 > W_3 > 0.  Graph S cannot meet those two shares with any batch of this recipe: with 4,000 random
    edges on 3,000 nodes it is nearly a forest, and W_3 > 0 together with W_4 > 0 needs a closed walk of odd length 7
    through the pair, that is an odd cycle of at most 7 nodes next to it.  Measured on S: 31.4 % of the pairs have
    W_3 > 0 and 0.1 % have W_4 > W_3 > 0; S is held to the by-construction property and to 30 % for W_3 > 0."""
    for l in MAX_LENS:
        assert (w[(l - 1) * WALK_PAIRS:l * WALK_PAIRS, l - 1] >= 1).all(), (name, l)
    s3, s43 = _shares(w)
    if name == "S":
        assert s3 >= 0.3, (name, s3)
    else:
        assert s3 >= 0.5 and s43 >= 0.25, (name, s3, s43)
