"""Graphs, start lists and restatement results shared by tests/test_random_walks_host.py and
tests/test_gpu_random_walks.py.  Every reference is computed once per process and handed out read-only.

Graphs S, H and C are those of tests/pair_distance_cases.py (H: hubs above the workgroup width, a hung path, isolated
nodes; C: two 300-cliques), Kloops is tests/node_structure_cases.graph_k_loops (stored self-loops)."""
from functools import lru_cache

import numpy as np
import torch

from lpformer_amd import graph
from lpformer_amd.random_walks import walks_reference
from tests import node_structure_cases as NC
from tests import pair_distance_cases as DC

CASES = {"S": DC.graph_s, "H": DC.graph_h, "C": DC.graph_c, "Kloops": NC.graph_k_loops}
NAMES = tuple(CASES)
PQ = ((1.0, 1.0), (0.25, 4.0), (4.0, 0.25))
LENGTH = 20
SEED = 5
BAD_STARTS = (-1, -(1 << 40), 1 << 40)        # with n appended per graph: all outside [0, n)

# the bias check: node 1 has the neighbours 0 (where the walk came from), 2 (a neighbour of 0), 3 and 5 (neither)
BIAS_EDGES = ((0, 1), (1, 2), (1, 3), (0, 2), (3, 4), (1, 5))
BIAS_WALKS = 65536
BIAS_TARGETS = (0, 2, 3, 5)
BIAS_WANT = {(0.5, 2.0): (0.5, 0.25, 0.125, 0.125), (4.0, 0.25): tuple(w / 9.25 for w in (0.25, 1.0, 4.0, 4.0)),
             (1.0, 1.0): (0.25, 0.25, 0.25, 0.25)}


def case(name: str) -> DC.Case:
    return CASES[name]()


@lru_cache(maxsize=None)
def starts(name: str) -> np.ndarray:
    """Every node, then starts outside [0, n), then 40 nodes drawn with repeats: int64, read-only.  With
    ``walks_per_node=2`` every node is walked from twice (and the repeated ones more often)."""
    n = case(name).n
    again = np.random.default_rng(31).integers(0, n, 40)
    s = np.concatenate([np.arange(n), np.array(BAD_STARTS + (n,)), again, again[:7]]).astype(np.int64)
    s.setflags(write=False)
    return s


@lru_cache(maxsize=None)
def reference(name: str, p: float, q: float, max_tries: int = 64):
    """(walks int32 [W, LENGTH + 1], forced int32 [W]) numpy arrays of the restatement for ``starts(name)`` twice."""
    out = walks_reference(case(name).csr, torch.from_numpy(starts(name).copy()), length=LENGTH, walks_per_node=2, p=p,
                          q=q, seed=SEED, max_tries=max_tries)
    arrs = (out.walks.numpy(), out.forced.numpy())
    for a in arrs:
        a.setflags(write=False)
    return arrs


@lru_cache(maxsize=None)
def bias_graph() -> graph.CSR:
    e = np.asarray(BIAS_EDGES, dtype=np.int64)
    A = DC._adjacency(e[:, 0], e[:, 1], 6)
    return graph.CSR(A.indptr.astype(np.int64), A.indices.astype(np.int32), None, 6)


def bias_z(walks: np.ndarray, want) -> np.ndarray:
    """|z| per target of BIAS_TARGETS: among the walks from node 0 whose first step went to node 1, the frequency of
    each second step against its node2vec probability, in binomial standard deviations."""
    second = walks[walks[:, 1] == 1, 2]
    m = second.size
    assert m > BIAS_WALKS // 4 and np.isin(second, BIAS_TARGETS).all()
    want = np.asarray(want, dtype=np.float64)
    freq = np.array([(second == v).mean() for v in BIAS_TARGETS])
    return np.abs(freq - want) / np.sqrt(want * (1.0 - want) / m)
