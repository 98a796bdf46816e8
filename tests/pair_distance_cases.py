"""Graphs, pair batches and the scipy reference shared by tests/test_pair_distance_host.py and
tests/test_gpu_pair_distance.py.  Every reference is computed once per process and handed out read-only."""
from functools import lru_cache
from typing import NamedTuple

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import shortest_path

from lpformer_amd import graph

MAX_DISTS = (1, 2, 3, 5)
HUBS = (0, 1, 2)
PATH_FIRST, PATH_LAST = 3890, 3949            # graph H: the path hung on node 5
CLIQUE = 300                                  # graph C: cliques [0, 300) and [300, 600), path 600 .. 604 between them


class Case(NamedTuple):
    n: int
    A: sp.csr_matrix                          # binary, symmetric, no diagonal
    csr: graph.CSR
    pairs: np.ndarray                         # int64 [2, P]


def _adjacency(rows, cols, n) -> sp.csr_matrix:
    """Symmetrised, deduplicated, diagonal dropped."""
    r, c = np.concatenate([rows, cols]), np.concatenate([cols, rows])
    keep = r != c
    A = sp.coo_matrix((np.ones(int(keep.sum())), (r[keep], c[keep])), shape=(n, n)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    A.data[:] = 1.0
    return A


def _case(A, n, pairs) -> Case:
    csr = graph.CSR(A.indptr.astype(np.int64), A.indices.astype(np.int32), None, n)
    pairs = np.ascontiguousarray(pairs, dtype=np.int64)
    pairs.setflags(write=False)
    return Case(n, A, csr, pairs)


@lru_cache(maxsize=None)
def graph_s() -> Case:
    """n = 3000, 4000 random edges: hundreds of components, small degrees, distances 0 .. 15."""
    n = 3000
    e = np.random.default_rng(7).integers(0, n, (2, 4000))
    return _case(_adjacency(e[0], e[1], n), n, np.random.default_rng(8).integers(0, n, (2, 4096)))


@lru_cache(maxsize=None)
def graph_h() -> Case:
    """n = 4000: a random body on nodes 0 .. 3889, hubs 0, 1, 2 above the workgroup width, a 60-node path hung on node
    5, nodes 3950 .. 3999 isolated."""
    n, body = 4000, 3890
    rng = np.random.default_rng(11)
    e = rng.integers(0, body, (2, 5000))
    rows, cols = [e[0]], [e[1]]
    for hub, k in zip(HUBS, (600, 300, 257)):
        nb = rng.choice(np.arange(3, body), k, replace=False)
        rows.append(np.full(k, hub))
        cols.append(nb)
    path = np.arange(PATH_FIRST, PATH_LAST + 1)
    rows += [np.array([5]), path[:-1]]
    cols += [np.array([PATH_FIRST]), path[1:]]
    A = _adjacency(np.concatenate(rows), np.concatenate(cols), n)
    return _case(A, n, np.random.default_rng(12).integers(0, n, (2, 4096)))


@lru_cache(maxsize=None)
def graph_c() -> Case:
    """n = 605: two 300-node cliques joined by a 5-node path (0 - 600 - 601 - 602 - 603 - 604 - 300).  A side's visit
    list fills with a whole clique; both sides together visit almost every node."""
    n = 2 * CLIQUE + 5
    i, j = np.triu_indices(CLIQUE, 1)
    chain = np.array([0, 600, 601, 602, 603, 604, CLIQUE])
    A = _adjacency(np.concatenate([i, i + CLIQUE, chain[:-1]]), np.concatenate([j, j + CLIQUE, chain[1:]]), n)
    rng = np.random.default_rng(14)
    across = np.stack([rng.integers(1, CLIQUE, 256), rng.integers(CLIQUE + 1, 2 * CLIQUE, 256)])
    pairs = np.concatenate([rng.integers(0, n, (2, 512)), across, across[::-1, :64],
                            np.array([[0, 1, 600, 602, 299], [CLIQUE, 2 * CLIQUE - 1, 604, 299, 601]])], axis=1)
    return _case(A, n, pairs)


CASES = {"S": graph_s, "H": graph_h, "C": graph_c}


def scipy_distance(A, pairs) -> np.ndarray:
    """int32 [P]: hops by scipy's unweighted Dijkstra from the distinct first endpoints, inf -> -1."""
    a, b = np.asarray(pairs)
    src, inv = np.unique(a, return_inverse=True)
    D = shortest_path(A, method="D", unweighted=True, indices=src)
    d = D[inv, b]
    return np.where(np.isfinite(d), d, -1).astype(np.int32)


@lru_cache(maxsize=None)
def exact(name: str) -> np.ndarray:
    case = CASES[name]()
    d = scipy_distance(case.A, case.pairs)
    d.setflags(write=False)
    return d


def masked(d: np.ndarray, m: int) -> np.ndarray:
    """What max_dist = m must give: where(exact <= m, exact, -1)."""
    return np.where(d <= m, d, -1).astype(np.int32)


def scipy_without_edge(A, a: int, b: int) -> int:
    """Hops from a to b on a copy of A with the edge {a, b} removed."""
    B = A.tolil(copy=True)
    B[a, b] = 0
    B[b, a] = 0
    B = B.tocsr()
    B.eliminate_zeros()
    d = shortest_path(B, method="D", unweighted=True, indices=[a])[0, b]
    return int(d) if np.isfinite(d) else -1


@lru_cache(maxsize=None)
def ignore_direct_h():
    """(pairs int64 [2, 128], reference int32 [128], plain int32 [128]) on graph H: 64 edges, whose reference is the
    per-edge scipy run on a copy without that edge, then 64 non-edges, which ignore_direct must leave unchanged."""
    case = graph_h()
    rng = np.random.default_rng(13)
    r, c = case.A.nonzero()
    pick = rng.choice(r.size, 64, replace=False)
    edges = np.stack([r[pick], c[pick]]).astype(np.int64)
    cand = rng.integers(0, case.n, (2, 400))
    is_edge = np.asarray(case.A[cand[0], cand[1]]).ravel() != 0
    non = cand[:, ~is_edge & (cand[0] != cand[1])][:, :64]
    assert non.shape[1] == 64
    pairs = np.concatenate([edges, non], axis=1)
    plain = scipy_distance(case.A, pairs)
    ref = plain.copy()
    ref[:64] = [scipy_without_edge(case.A, int(a), int(b)) for a, b in edges.T]
    for arr in (pairs, ref, plain):
        arr.setflags(write=False)
    return pairs, ref, plain
