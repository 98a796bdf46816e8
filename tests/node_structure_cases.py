"""Graphs, hand cases and references shared by tests/test_node_structure_host.py and tests/test_gpu_node_structure.py.
Every reference is computed once per process and handed out read-only.

Graphs S, H and C are those of tests/pair_distance_cases.py, unchanged.  Graph K is there because S and H hold almost no
triangles: planted cliques whose sizes straddle the wavefront width and the row-length switch of lpf_core_sweep
(LPF_CORE_LONG_ROW = 64 entries) and the walked-length switch of lpf_node_triangles (LPF_HEUR_SPLIT_DEFAULT = 32).
Graph P is a path: the worst case of the h-index iteration."""
from functools import lru_cache
from typing import NamedTuple

import numpy as np

from lpformer_amd import graph
from lpformer_amd.structure import KINDS, structure_reference
from tests import pair_distance_cases as DC

K_N, K_ACTIVE = 2000, 1960                    # graph K: nodes 1960 .. 1999 are isolated
K_CLIQUES = ((0, 130), (120, 65), (200, 64), (300, 63), (400, 17), (500, 3))   # (first node, size): the first two share 10
P_N = 2001                                    # graph P: the path 0 - 1 - ... - 2000
# Changing sweeps the SYNCHRONOUS h-index iteration needs on a path hanging free: a node at distance i from a free end
# drops to 1 in sweep i, so a path of L edges with both ends free (P: L = 2000) needs ceil(L / 2), and one hung on a
# denser body by one end (H: 60 edges from node 5 to the free end) more than that.
SWEEP_BOUND = {"P": (P_N - 1 + 1) // 2, "H": (DC.PATH_LAST - DC.PATH_FIRST + 1 + 1) // 2}


def _with_self_loops(A, nodes):
    B = A.tolil(copy=True)
    for v in nodes:
        B[v, v] = 1.0
    B = B.tocsr()
    B.sort_indices()
    return B


@lru_cache(maxsize=None)
def graph_k() -> DC.Case:
    rng = np.random.default_rng(21)
    rows, cols = [], []
    for first, size in K_CLIQUES:
        i, j = np.triu_indices(size, 1)
        rows.append(i + first)
        cols.append(j + first)
    e = rng.integers(0, K_ACTIVE, (2, 6000))
    rows.append(e[0])
    cols.append(e[1])
    A = DC._adjacency(np.concatenate(rows), np.concatenate(cols), K_N)
    pairs = np.concatenate([rng.integers(0, K_N, (2, 1000)), np.array([[-1, 0, K_N, 5], [3, K_N + 7, 2, -4]])], axis=1)
    return DC._case(A, K_N, pairs)


@lru_cache(maxsize=None)
def graph_k_loops() -> DC.Case:
    """K with 100 stored self-loops (clique members, random-body nodes and isolated nodes among them)."""
    k = graph_k()
    nodes = np.random.default_rng(22).choice(K_N, 100, replace=False)
    return DC._case(_with_self_loops(k.A, nodes), K_N, k.pairs)


@lru_cache(maxsize=None)
def graph_p() -> DC.Case:
    i = np.arange(P_N - 1)
    return DC._case(DC._adjacency(i, i + 1, P_N), P_N, np.random.default_rng(23).integers(0, P_N, (2, 64)))


CASES = {"S": DC.graph_s, "H": DC.graph_h, "C": DC.graph_c, "K": graph_k, "P": graph_p}
NAMES = tuple(CASES)


def _frozen(ns) -> dict:
    out = {k: getattr(ns, k).numpy() for k in KINDS}
    for a in out.values():
        a.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def reference(name: str) -> dict:
    """kind -> numpy array of ``structure_reference`` on the named graph ("Kloops": K with stored self-loops)."""
    case = graph_k_loops() if name == "Kloops" else CASES[name]()
    return _frozen(structure_reference(case.csr))


class Hand(NamedTuple):
    what: str
    csr: graph.CSR
    want: dict                                # kind -> list, written out by hand


def _csr(n, edges) -> graph.CSR:
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    A = DC._adjacency(e[:, 0], e[:, 1], n)
    return graph.CSR(A.indptr.astype(np.int64), A.indices.astype(np.int32), None, n)


def hand_cases():
    star = [(0, leaf) for leaf in range(1, 71)]
    return (
        Hand("empty_n5", _csr(5, []),
             {"degree": [0] * 5, "core": [0] * 5, "component": [0, 1, 2, 3, 4], "triangles": [0] * 5}),
        Hand("single_edge", _csr(4, [(1, 3)]),
             {"degree": [0, 1, 0, 1], "core": [0, 1, 0, 1], "component": [0, 1, 2, 1], "triangles": [0] * 4}),
        # triangle 1 - 2 - 4 with the pendant 0 on node 2; node 3 isolated
        Hand("triangle_with_pendant", _csr(5, [(1, 2), (2, 4), (1, 4), (0, 2)]),
             {"degree": [1, 2, 3, 0, 2], "core": [1, 2, 2, 0, 2], "component": [0, 0, 0, 3, 0],
              "triangles": [0, 1, 1, 0, 1]}),
        # the hub's row is longer than a wavefront and than LPF_CORE_LONG_ROW
        Hand("star_70", _csr(71, star),
             {"degree": [70] + [1] * 70, "core": [1] * 71, "component": [0] * 71, "triangles": [0] * 71}),
    )


def permuted(case: DC.Case, seed: int = 5):
    """(case with node v renamed perm[v], perm)."""
    perm = np.random.default_rng(seed).permutation(case.n)
    coo = case.A.tocoo()
    pairs = perm[np.clip(case.pairs, 0, case.n - 1)]
    return DC._case(DC._adjacency(perm[coo.row], perm[coo.col], case.n), case.n, pairs), perm


def sync_core_sweeps(case: DC.Case) -> int:
    """Changing sweeps of the SYNCHRONOUS (Jacobi) h-index iteration from the degrees, in numpy: the schedule the bound
    above is about."""
    indptr, indices = case.A.indptr, case.A.indices
    est = np.diff(indptr).astype(np.int64)
    rows = np.repeat(np.arange(case.n), np.diff(indptr))
    sweeps = 0
    while True:
        # H_v = max h with at least h neighbours of est >= h: sort each row's neighbour values descending
        vals = est[indices]
        order = np.lexsort((-vals, rows))
        sorted_vals = vals[order]
        rank = np.arange(vals.size) - indptr[rows] + 1          # 1-based rank inside the row
        ok = sorted_vals >= rank
        h = np.zeros(case.n, np.int64)
        np.maximum.at(h, rows[ok], rank[ok])
        new = np.minimum(est, h)
        if np.array_equal(new, est):
            return sweeps
        est, sweeps = new, sweeps + 1
