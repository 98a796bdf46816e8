"""The scipy reference and the hand cases shared by tests/test_pair_hops_host.py and tests/test_gpu_pair_hops.py, on the
graphs S, H and C of tests/pair_distance_cases.py and the batches of tests/pair_katz_cases.case(name), both unchanged.
The reference is independent of the module's restatement: scipy's unweighted shortest paths from the distinct
endpoints, binned into classes and counted.  Every reference is computed once per process and handed out read-only."""
from functools import lru_cache
from typing import NamedTuple

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import shortest_path

from lpformer_amd import graph
from tests import pair_katz_cases as KC

HOPS = (1, 2)
NAMES = ("S", "H", "C")
K_MAX = 2
SOURCES_PER_CALL = 512                        # rows of the distance matrix held at once


def _classes(D, k: int) -> np.ndarray:
    """int8: d where d <= k, else k + 1 (inf included)."""
    return np.where(D <= k, D, k + 1).astype(np.int8)


def _count(ca, cb, k: int) -> np.ndarray:
    """int32 [P, k+2, k+2] from the class rows ca, cb int8 [P, n] of each pair's endpoints."""
    P, cells = ca.shape[0], (k + 2) ** 2
    key = ca.astype(np.int64) * (k + 2) + cb + np.arange(P, dtype=np.int64)[:, None] * cells
    return np.bincount(key.ravel(), minlength=P * cells).reshape(P, k + 2, k + 2).astype(np.int32)


def _merge(c, k: int) -> np.ndarray:
    """The classes at hops = k from those at hops = K_MAX."""
    return np.minimum(c, k + 1)


def _valid(pairs, n):
    a, b = np.asarray(pairs)
    return (a >= 0) & (a < n) & (b >= 0) & (b < n)


@lru_cache(maxsize=None)
def _endpoint_classes(name: str):
    """(distinct endpoints int64 [U], their classes at hops = K_MAX int8 [U, n]) of the case's in-range pairs."""
    c = KC.case(name)
    ok = _valid(c.pairs, c.n)
    src = np.unique(c.pairs[:, ok])
    rows = [_classes(shortest_path(c.A, method="D", unweighted=True, indices=src[lo:lo + SOURCES_PER_CALL]), K_MAX)
            for lo in range(0, src.size, SOURCES_PER_CALL)]
    return src, np.concatenate(rows)


def _without_edge(A, a: int, b: int) -> sp.csr_matrix:
    B = A.copy()
    for r, c in ((a, b), (b, a)):
        lo, hi = B.indptr[r], B.indptr[r + 1]
        at = lo + int(np.searchsorted(B.indices[lo:hi], c))
        assert at < hi and B.indices[at] == c
        B.data[at] = 0.0
    B.eliminate_zeros()
    return B


@lru_cache(maxsize=None)
def stored(name: str) -> np.ndarray:
    """bool [P]: the pairs that are stored entries of the graph (read-only)."""
    c = KC.case(name)
    ok = _valid(c.pairs, c.n)
    s = np.zeros(c.pairs.shape[1], bool)
    s[ok] = np.asarray(c.A[c.pairs[0, ok], c.pairs[1, ok]]).ravel() != 0
    s.setflags(write=False)
    return s


@lru_cache(maxsize=None)
def _pair_classes(name: str, ignore_direct: bool):
    """(ca, cb) int8 [P, n] at hops = K_MAX (rows of out-of-range pairs are unused)."""
    c = KC.case(name)
    src, cls = _endpoint_classes(name)
    ok = _valid(c.pairs, c.n)
    ca = np.zeros((c.pairs.shape[1], c.n), np.int8)
    cb = np.zeros_like(ca)
    ca[ok] = cls[np.searchsorted(src, c.pairs[0, ok])]
    cb[ok] = cls[np.searchsorted(src, c.pairs[1, ok])]
    if ignore_direct:
        # every pair that is a stored entry: recomputed on a per-pair copy of A without that edge
        for i in np.flatnonzero(stored(name)):
            a, b = int(c.pairs[0, i]), int(c.pairs[1, i])
            D = shortest_path(_without_edge(c.A, a, b), method="D", unweighted=True, indices=[a, b])
            ca[i], cb[i] = _classes(D, K_MAX)
    return ca, cb


@lru_cache(maxsize=None)
def exact(name: str, hops: int = 2, ignore_direct: bool = False) -> np.ndarray:
    """int32 [P, hops+2, hops+2], read-only: an out-of-range pair's table is all zero."""
    c = KC.case(name)
    ca, cb = _pair_classes(name, bool(ignore_direct))
    t = _count(_merge(ca, hops), _merge(cb, hops), hops)
    t[~_valid(c.pairs, c.n)] = 0
    t.setflags(write=False)
    if hops == 2:
        _check_ignore_direct(name, t) if ignore_direct else _check_condition(name, t)
    return t


def positive_shares(t) -> dict:
    """The share of the pairs on which each of the cells T[1][1], T[1][2], T[2][1], T[2][2] is positive."""
    return {(i, j): float((t[:, i, j] > 0).mean()) for i in (1, 2) for j in (1, 2)}


def distinct_tables(t) -> int:
    return int(np.unique(t.reshape(t.shape[0], -1), axis=0).shape[0])


# What the shares must reach at hops = 2, asserted on the reference alone.  Measured with these batches:
# S 23 / 27 / 30 / 26 %, H 36 / 51 / 54 / 66 %, C 78 / 6.8 / 6.9 / 65 % for the cells (1,1) / (1,2) / (2,1) / (2,2);
# 1,240 distinct tables on S and 1,628 on H.
SHARE_FLOORS = {"S": {(1, 1): 0.2, (1, 2): 0.2, (2, 1): 0.2, (2, 2): 0.2},
                "H": {(1, 1): 0.3, (1, 2): 0.3, (2, 1): 0.3, (2, 2): 0.3},
                "C": {(1, 1): 0.5, (1, 2): 0.05, (2, 1): 0.05, (2, 2): 0.5}}
DISTINCT_FLOORS = {"S": 1000, "H": 1000}


def _check_condition(name: str, t) -> None:
    """What keeps a trivial kernel from passing: the near cells are positive on a good share of the pairs, the tables
    differ from pair to pair, and every valid pair's table sums to n."""
    c = KC.case(name)
    shares = positive_shares(t)
    for cell, floor in SHARE_FLOORS[name].items():
        assert shares[cell] >= floor, (name, cell, shares[cell])
    if name in DISTINCT_FLOORS:
        assert distinct_tables(t) >= DISTINCT_FLOORS[name], (name, distinct_tables(t))
    ok = _valid(c.pairs, c.n)
    sums = t.reshape(t.shape[0], -1).sum(axis=1)
    assert (sums[ok] == c.n).all() and (sums[~ok] == 0).all() and int((~ok).sum()) == 4, name


def _check_ignore_direct(name: str, t) -> None:
    """Under ignore_direct the table changes on exactly the pairs that are stored entries, and those include all 64 of
    ``case.edges``."""
    c = KC.case(name)
    plain = exact(name, 2, False)
    changed = (t != plain).reshape(t.shape[0], -1).any(axis=1)
    assert np.array_equal(changed, stored(name)), name
    assert stored(name)[c.edges].all() and stored(name)[c.edges].sum() == 64, name
    ok = _valid(c.pairs, c.n)
    assert (t.reshape(t.shape[0], -1).sum(axis=1)[ok] == c.n).all(), name


# ------------------------------------------------------------------------------------------------------- hand cases
class Hand(NamedTuple):
    what: str
    csr: graph.CSR
    hops: int
    ignore_direct: bool
    pairs: np.ndarray                         # int64 [2, P]
    tables: np.ndarray                        # int32 [P, hops+2, hops+2]


def _csr(n: int, edges, loops=()) -> graph.CSR:
    """The symmetric pattern of the undirected ``edges`` plus the stored self-loops ``loops``."""
    e = np.array(edges, np.int64).reshape(-1, 2)
    r = np.concatenate([e[:, 0], e[:, 1], np.array(loops, np.int64)])
    c = np.concatenate([e[:, 1], e[:, 0], np.array(loops, np.int64)])
    A = sp.coo_matrix((np.ones(r.size), (r, c)), shape=(n, n)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return graph.CSR(A.indptr.astype(np.int64), A.indices.astype(np.int32), None, n)


def _hand(what, csr, hops, ignore_direct, cases) -> Hand:
    pairs = np.array([p for p, _ in cases], np.int64).T
    tables = np.array([t for _, t in cases], np.int32)
    assert tables.shape == (pairs.shape[1], hops + 2, hops + 2)
    pairs.setflags(write=False)
    tables.setflags(write=False)
    return Hand(what, csr, hops, ignore_direct, pairs, tables)


Z3 = [[0, 0, 0]] * 3
Z4 = [[0, 0, 0, 0]] * 4


@lru_cache(maxsize=None)
def hand_cases():
    """Row i of a table: the nodes at distance i from a (last row: farther than ``hops``, or unreachable); column j:
    the same for b."""
    path = _csr(5, [(0, 1), (1, 2), (2, 3), (3, 4)])                       # 0 - 1 - 2 - 3 - 4
    star = _csr(6, [(0, v) for v in range(1, 6)])                          # centre 0, leaves 1 .. 5
    # triangle 0 1 2, node 3 pendant on 2, node 4 isolated, stored self-loops on 0 and 2
    tri = _csr(5, [(0, 1), (1, 2), (0, 2), (2, 3)], loops=(0, 2))
    tri_plain = [
        ((0, 1), [[0, 1, 0, 0], [1, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]),   # 2 is the common neighbour, 3 at (2, 2)
        ((2, 3), [[0, 1, 0, 0], [1, 0, 2, 0], [0, 0, 0, 0], [0, 0, 0, 1]]),   # the bridge
        ((2, 2), [[1, 0, 0, 0], [0, 3, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1]]),   # a == b: diagonal
        ((0, 0), [[1, 0, 0, 0], [0, 2, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]),
        ((4, 0), [[0, 0, 0, 1], [0, 0, 0, 0], [0, 0, 0, 0], [1, 2, 1, 0]]),   # an isolated endpoint
        ((4, 4), [[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 4]]),
        ((-1, 0), Z4), ((0, 5), Z4), ((5, 5), Z4), ((-3, 7), Z4),             # ids outside [0, n)
    ]
    tri_cut = [
        ((0, 1), [[0, 0, 1, 0], [0, 1, 0, 0], [1, 0, 1, 0], [0, 0, 0, 1]]),   # the triangle's edge: distance 1 -> 2
        ((2, 3), [[0, 0, 0, 1], [0, 0, 0, 2], [0, 0, 0, 0], [1, 0, 0, 1]]),   # the bridge: 3 becomes unreachable
        ((3, 2), [[0, 0, 0, 1], [0, 0, 0, 0], [0, 0, 0, 0], [1, 2, 0, 1]]),
        ((2, 2), [[1, 0, 0, 0], [0, 3, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1]]),   # the skipped entry is the self-loop
        ((0, 3), [[0, 0, 1, 0], [0, 1, 1, 0], [1, 0, 0, 0], [0, 0, 0, 1]]),   # no stored entry: unaffected
        ((4, 0), [[0, 0, 0, 1], [0, 0, 0, 0], [0, 0, 0, 0], [1, 2, 1, 0]]),
        ((5, 0), Z4),
    ]
    return (
        _hand("path of 5 nodes", path, 2, False, [
            ((0, 4), [[0, 0, 0, 1], [0, 0, 0, 1], [0, 0, 1, 0], [1, 1, 0, 0]]),
            ((0, 2), [[0, 0, 1, 0], [0, 1, 0, 0], [1, 0, 0, 0], [0, 1, 1, 0]]),
            ((1, 3), [[0, 0, 1, 0], [0, 1, 0, 1], [1, 0, 0, 0], [0, 1, 0, 0]]),
        ]),
        _hand("path of 5 nodes, one hop", path, 1, False, [
            ((0, 2), [[0, 0, 1], [0, 1, 0], [1, 1, 1]]),
            ((0, 1), [[0, 1, 0], [1, 0, 0], [0, 1, 2]]),
            ((7, 1), Z3),
        ]),
        _hand("star", star, 2, False, [
            ((1, 2), [[0, 0, 1, 0], [0, 1, 0, 0], [1, 0, 3, 0], [0, 0, 0, 0]]),
            ((0, 1), [[0, 1, 0, 0], [1, 0, 4, 0], [0, 0, 0, 0], [0, 0, 0, 0]]),
        ]),
        _hand("triangle with a pendant node, an isolated node and stored self-loops", tri, 2, False, tri_plain),
        _hand("the same under ignore_direct", tri, 2, True, tri_cut),
        _hand("the same, one hop, under ignore_direct", tri, 1, True, [
            ((0, 1), [[0, 0, 1], [0, 1, 0], [1, 0, 2]]),
            ((2, 3), [[0, 0, 1], [0, 0, 2], [1, 0, 1]]),
        ]),
    )
