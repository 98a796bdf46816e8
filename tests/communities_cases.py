"""Graphs, hand cases and references shared by tests/test_communities_host.py and tests/test_gpu_communities.py.  Every
reference is computed once per process and handed out read-only.

Graphs S, H, C, K, Kloops and P are those of tests/node_structure_cases.py, unchanged: K's rows lie on both sides of
LPF_COMM_LONG_ROW = 64 entries, H's hubs (603 entries) and C's cliques (300) are listed rows.  Added here:

  D   disjoint cliques of 3, 17, 63, 64, 65 and 130 nodes and 5 isolated nodes, n = 347: the planted answer is one
      community per clique; the 65- and 130-cliques' rows are listed rows, and with lds_slots = 64 they take the
      device-memory table
  R   a ring of 12 seven-cliques (clique i's last node joined to clique i + 1's first): one community per clique
  B   the planted partition 8 x 40 at p_in = 0.4, p_out = 0.01 from a fixed numpy seed

QUALITY MARGIN.  On B, K, P and R, seeds 0 - 3, the restatement's modularity is compared with
``networkx.community.louvain_communities(seed=0)``'s.  Measured shortfalls 1 - Q / Q_networkx of the committed
restatement (tests/test_communities_host.py prints them; negative: better than networkx):

    B   seeds 0-3:  0.0000   0.0000   0.0066   0.0000        (networkx: Q = 0.7093)
    K   seeds 0-3:  0.0046   0.0032   0.0029   0.0086        (networkx: Q = 0.5926)
    P   seeds 0-3:  0.0003   0.0003   0.0005   0.0002        (networkx: Q = 0.9549)
    R   seeds 0-3:  0.0000   0.0000   0.0000   0.0000        (networkx: Q = 0.8712)

The largest is 0.0086 (K, seed 3); the margin is twice that, 0.0172, and not below 0.01.  The factor 2 is there because
the bound guards against a broken schedule (without the activation bit the restatement loses 99 % on the path P:
Q = 0.008 against 0.955), not against seed noise."""
from functools import lru_cache
from typing import NamedTuple

import numpy as np

from lpformer_amd import graph
from lpformer_amd.community import communities_reference
from lpformer_amd.structure import structure_reference
from tests import node_structure_cases as NC
from tests import pair_distance_cases as DC

D_CLIQUES = (3, 17, 63, 64, 65, 130)          # graph D: consecutive node ranges, then 5 isolated nodes
D_N = sum(D_CLIQUES) + 5
R_CLIQUES, R_SIZE = 12, 7                     # graph R
B_BLOCKS, B_SIZE, B_P_IN, B_P_OUT = 8, 40, 0.4, 0.01
QUALITY_GRAPHS, QUALITY_SEEDS = ("B", "K", "P", "R"), (0, 1, 2, 3)
QUALITY_MARGIN = 0.0172                       # twice the largest measured shortfall (see above), not below 0.01


@lru_cache(maxsize=None)
def graph_d() -> DC.Case:
    rows, cols, first = [], [], 0
    for size in D_CLIQUES:
        i, j = np.triu_indices(size, 1)
        rows.append(i + first)
        cols.append(j + first)
        first += size
    pairs = np.concatenate([np.random.default_rng(31).integers(0, D_N, (2, 500)),
                            np.array([[-1, 0, D_N, 5], [3, D_N + 7, 2, -4]])], axis=1)
    return DC._case(DC._adjacency(np.concatenate(rows), np.concatenate(cols), D_N), D_N, pairs)


def d_planted() -> np.ndarray:
    """The label D must get: the first node of each clique, an isolated node itself."""
    starts = np.cumsum((0,) + D_CLIQUES[:-1])
    return np.concatenate([np.repeat(starts, D_CLIQUES), np.arange(D_N - 5, D_N)]).astype(np.int32)


@lru_cache(maxsize=None)
def graph_r() -> DC.Case:
    n = R_CLIQUES * R_SIZE
    i, j = np.triu_indices(R_SIZE, 1)
    rows = [i + c * R_SIZE for c in range(R_CLIQUES)]
    cols = [j + c * R_SIZE for c in range(R_CLIQUES)]
    last = np.arange(R_CLIQUES) * R_SIZE + R_SIZE - 1
    rows.append(last)
    cols.append((last + 1) % n)
    return DC._case(DC._adjacency(np.concatenate(rows), np.concatenate(cols), n), n,
                    np.random.default_rng(32).integers(0, n, (2, 64)))


def r_planted() -> np.ndarray:
    return np.repeat(np.arange(R_CLIQUES) * R_SIZE, R_SIZE).astype(np.int32)


@lru_cache(maxsize=None)
def graph_b() -> DC.Case:
    n = B_BLOCKS * B_SIZE
    rng = np.random.default_rng(33)
    i, j = np.triu_indices(n, 1)
    p = np.where(i // B_SIZE == j // B_SIZE, B_P_IN, B_P_OUT)
    keep = rng.random(i.size) < p
    return DC._case(DC._adjacency(i[keep], j[keep], n), n, rng.integers(0, n, (2, 64)))


CASES = dict(NC.CASES, Kloops=NC.graph_k_loops, D=graph_d, R=graph_r, B=graph_b)
NAMES = tuple(CASES)


def _frozen(c):
    for t in [c.label] + c.hierarchy:
        t.numpy().setflags(write=False)
    return c


@lru_cache(maxsize=None)
def reference(name: str, seed: int = 0, max_rounds: int = 64, max_levels: int = 16):
    """``communities_reference`` on the named graph."""
    return _frozen(communities_reference(CASES[name]().csr, seed=seed, max_rounds=max_rounds, max_levels=max_levels))


@lru_cache(maxsize=None)
def component(name: str) -> np.ndarray:
    """``structure_reference``'s component label of the named graph."""
    out = structure_reference(CASES[name]().csr, kinds=("component",)).component.numpy()
    out.setflags(write=False)
    return out


class Hand(NamedTuple):
    what: str
    csr: graph.CSR
    label: list                               # written out by hand
    count: int


def hand_cases():
    star = [(0, leaf) for leaf in range(1, 71)]
    return (
        Hand("no_edge_n5", NC._csr(5, []), [0, 1, 2, 3, 4], 5),
        Hand("one_edge", NC._csr(4, [(1, 3)]), [0, 1, 2, 1], 3),
        # triangle 1 - 2 - 4 with the pendant 0 on node 2; node 3 isolated.  2m = 8, and Qnum = 0 is the maximum, reached
        # by {0, 1, 2, 4} (8 * 8 - 8^2) and by {0, 2} {1, 4} (8 * 4 - 4^2 - 4^2): the pendant joins its only neighbour,
        # 1 and 4 join each other, and merging the two halves gains exactly 0 -- a level accepts only a strict gain
        Hand("triangle_with_pendant", NC._csr(5, [(1, 2), (2, 4), (1, 4), (0, 2)]), [0, 1, 0, 3, 1], 3),
        # the hub's row is a listed row; every split of a star lowers Q
        Hand("star_70", NC._csr(71, star), [0] * 71, 1),
        # triangles 0 1 2 and 3 4 5 joined by 2 - 3
        Hand("two_triangles", NC._csr(6, [(0, 1), (0, 2), (1, 2), (3, 4), (3, 5), (4, 5), (2, 3)]),
             [0, 0, 0, 3, 3, 3], 2),
    )


def weighted_level(case: DC.Case, seed: int = 41):
    """A level-1 shape on ``case``'s pattern, made by hand: symmetric int64 weights in 1 .. 9 per stored entry (0 on a
    stored self-loop's entry is NOT needed: the kernels skip col == row), self weights s in 0 .. 20, k from both, and
    a non-trivial ``comm``: blocks of 7 consecutive nodes named by their first node, every 11th node a singleton.
    Returns a dict of numpy arrays: indptr, indices, weight, s, k, comm, tot, cnt, two_m."""
    rng = np.random.default_rng(seed)
    A = case.A.tocsr()
    indptr, indices = A.indptr.astype(np.int64), A.indices.astype(np.int32)
    n = case.n
    rows = np.repeat(np.arange(n), np.diff(indptr))
    lo, hi = np.minimum(rows, indices), np.maximum(rows, indices)
    weight = (1 + (lo * 7919 + hi * 104729 + seed) % 9).astype(np.int64)         # the same for (u, v) and (v, u)
    s = rng.integers(0, 21, n).astype(np.int64)
    k = s.copy()
    np.add.at(k, rows[rows != indices], weight[rows != indices])
    ids = np.arange(n)
    comm = np.where(ids % 11 == 0, ids, (ids // 7) * 7).astype(np.int32)
    tot = np.zeros(n, np.int64)
    np.add.at(tot, comm, k)
    cnt = np.bincount(comm, minlength=n).astype(np.int32)
    return {"indptr": indptr, "indices": indices, "weight": weight, "s": s, "k": k, "comm": comm, "tot": tot,
            "cnt": cnt, "two_m": int(k.sum())}
