"""Graphs, pair lists, tables, weights, references and error bounds shared by tests/test_cn_pool_host.py and
tests/test_gpu_cn_pool.py.  Every reference is computed once per process and handed out as it is: do not write to one.

Cases: graphs S, H and C of tests/pair_distance_cases.py with their pair lists (H also with the hub pairs (0, 1),
(0, 2), (1, 2) in both orders: 53 / 32 / 19 common neighbours behind walked rows of 302 / 260 / 260 entries), and the
graph ``fan`` built here, whose pairs share exactly 0, 1, 63, 64, 65, 129 and 192 neighbours -- every edge of the chunk
rule.  Each list ends with four pairs that hold an id of -1, n, 2^31 and n + 5.

Bounds.  They are derived, not measured: u = 2^-24, the first-order bound of a chunked sequential fused-multiply-add sum
(m terms summed in order from zero carry at most m roundings each of relative size u; adding c chunk rows in order adds
at most c more), one more u of slack for the reference's own fp32 weights times fp64 rows, and 1 % for second order:

    forward    |pool - ref| <= 1.01 (min(k, 64) + ceil(k / 64) + 1) u sum_i |w[u_i] T[u_i]|          elementwise
    backward   |dT - ref|   <= 1.01 (min(c, 128) + ceil(c / 128) + 1) u |w[u]| sum |g[p]|            c = occurrences of u

Worst error / bound ratios printed by tests/test_gpu_cn_pool.py on an MI355X (a ratio above 1 means the kernel or the
derivation is wrong):

    forward, worst over weights none / aa / tensor      S       H       C       fan
        D = 4                                           0.259   0.290   0.235   0.298
        D = 36                                          0.315   0.315   0.303   0.314
        D = 128                                         0.363   0.325   0.313   0.329
        D = 512                                         0.327   0.399   0.316   0.328
    backward, worst over weights none / ra / tensor     H       C       C2      fan
        D = 36                                          0.374   0.276   0.288   0.417
        D = 128                                         0.382   0.305   0.263   0.462
    (most occurrences of one node: H 79, C 135, C2 270, fan 5; on C with unit weights the ratios are 0.005 - 0.020:
    298 terms of mixed sign cancel, the bound does not)
    h.grad through the pooling, NCNPredictor on graph C with the fp64 dense part's upstream gradient: 0.131
"""
from functools import lru_cache
from typing import NamedTuple

import numpy as np
import scipy.sparse as sp
import torch

from lpformer_amd import graph, ncn
from tests import pair_distance_cases as DC

U24 = 2.0 ** -24
CHUNK = ncn.CHUNK
BWD_CHUNK = 128                                  # LPF_SKIPGRAM_CHUNK: the backward's rule
DIMS = (4, 36, 128, 512)
INT_DIM = 36
WEIGHT_KINDS = ("none", "aa", "tensor")
THRESHOLDS = (0, 1, 8, 64, 299, 1 << 30)
FAN_KS = (0, 1, 63, 64, 65, 129, 192)
FAN_PRIVATE_A, FAN_PRIVATE_B = 5, 300
HUB_PAIRS = ((0, 1), (0, 2), (1, 2))
NAMES = ("S", "H", "C", "fan")
# the backward's cases: C2 is graph C with its pair list twice -- C's own list gives a node at most 135 occurrences
# (two chunks of 128: its 257 pairs with 298 common neighbours are spread over two cliques), C2 gives 270: three chunks
BACKWARD_NAMES = ("H", "C", "C2", "fan")


class Case(NamedTuple):
    name: str
    n: int
    A: sp.csr_matrix                             # binary
    csr: graph.CSR
    pairs: torch.Tensor                          # int64 [2, P]
    n_bad: int                                   # the trailing pairs with an id outside [0, n)


def _bad_pairs(n):
    return np.array([[-1, 0, 1 << 31, 1], [0, n, 1, n + 5]], dtype=np.int64)


def _finish(name, A, n, pairs) -> Case:
    csr = graph.CSR(A.indptr.astype(np.int64), A.indices.astype(np.int32), None, n)
    bad = _bad_pairs(n)
    pairs = torch.from_numpy(np.concatenate([np.asarray(pairs, dtype=np.int64), bad], axis=1))
    return Case(name, n, A, csr, pairs, bad.shape[1])


def _fan():
    """(A, n, pairs, facts): per k a pair (a_k, b_k) with exactly k common neighbours, 5 private neighbours of a_k and
    300 of b_k -- the short row is walked, the probed row is long -- and the mirrored pair; a pair (c, d) with 10
    neighbours on either end, 4 of them shared, in both orders (the min(a, b) tie); 96 random pairs.  Node ids are a
    seeded shuffle, so the shared neighbours are spread through both rows."""
    rng = np.random.default_rng(21)
    rows, cols, named, nxt = [], [], [], 0

    def fresh(m):
        nonlocal nxt
        ids = np.arange(nxt, nxt + m)
        nxt += m
        return ids

    def star(centre, leaves):
        rows.append(np.full(leaves.size, centre))
        cols.append(leaves)

    for k in FAN_KS:
        a, b = fresh(2)
        shared = fresh(k)
        star(a, np.concatenate([shared, fresh(FAN_PRIVATE_A)]))
        star(b, np.concatenate([shared, fresh(FAN_PRIVATE_B)]))
        named.append((a, b, k))
    c, d = fresh(2)
    shared = fresh(4)
    star(c, np.concatenate([shared, fresh(6)]))
    star(d, np.concatenate([shared, fresh(6)]))
    named.append((c, d, 4))
    n = nxt
    perm = rng.permutation(n)
    A = DC._adjacency(perm[np.concatenate(rows)], perm[np.concatenate(cols)], n)
    listed = [(perm[a], perm[b]) for a, b, _ in named] + [(perm[b], perm[a]) for a, b, _ in named]
    pairs = np.concatenate([np.array(listed, dtype=np.int64).T, rng.integers(0, n, (2, 96))], axis=1)
    facts = [(int(perm[a]), int(perm[b]), k) for a, b, k in named]
    return A, n, pairs, facts


@lru_cache(maxsize=None)
def fan_facts():
    return _fan()[3]


@lru_cache(maxsize=None)
def case(name: str) -> Case:
    if name == "fan":
        A, n, pairs, facts = _fan()
        deg = np.diff(A.indptr)
        for a, b, k in facts[:-1]:
            assert deg[a] == k + FAN_PRIVATE_A and deg[b] == k + FAN_PRIVATE_B
            assert int(A[a].multiply(A[b]).sum()) == k
        c, d, k = facts[-1]
        assert deg[c] == deg[d] == 10 and int(A[c].multiply(A[d]).sum()) == k == 4
        return _finish(name, A, n, pairs)
    base = DC.CASES["C" if name == "C2" else name]()
    pairs = np.concatenate([base.pairs, base.pairs], axis=1) if name == "C2" else base.pairs
    if name == "H":
        hubs = np.array(HUB_PAIRS + tuple((b, a) for a, b in HUB_PAIRS), dtype=np.int64).T
        pairs = np.concatenate([pairs, hubs], axis=1)
    return _finish(name, base.A, base.n, pairs)


@lru_cache(maxsize=None)
def dense_rows(name: str) -> sp.csr_matrix:
    """A[a] o A[b] as a sparse [P, n] 0/1 matrix in fp64 (rows of bad pairs empty): the contract's neighbour sets."""
    c = case(name)
    a, b = c.pairs.numpy()
    ok = (a >= 0) & (a < c.n) & (b >= 0) & (b < c.n)
    A = c.A.astype(np.float64)
    M = A[np.where(ok, a, 0)].multiply(A[np.where(ok, b, 0)]).tocsr()
    M = sp.diags(ok.astype(np.float64)) @ M
    M.eliminate_zeros()
    M.sort_indices()
    return M


@lru_cache(maxsize=None)
def counts(name: str) -> torch.Tensor:
    """int64 [P]: k per pair."""
    return torch.from_numpy(np.diff(dense_rows(name).indptr).astype(np.int64))


@lru_cache(maxsize=None)
def entries(name: str) -> ncn.CnEntries:
    c = case(name)
    return ncn.cn_entries_reference(c.csr, c.pairs)


@lru_cache(maxsize=None)
def table(name: str, dim: int) -> torch.Tensor:
    """Standard normal float32 [n, dim]."""
    rng = np.random.default_rng(100 + dim)
    return torch.from_numpy(rng.standard_normal((case(name).n, dim)).astype(np.float32))


@lru_cache(maxsize=None)
def int_table(name: str) -> torch.Tensor:
    """Integers -3 .. 3 as float32 [n, INT_DIM]: with ``int_weights`` every summation order is exact in fp32."""
    rng = np.random.default_rng(7)
    return torch.from_numpy(rng.integers(-3, 4, (case(name).n, INT_DIM)).astype(np.float32))


@lru_cache(maxsize=None)
def int_weights(name: str) -> torch.Tensor:
    rng = np.random.default_rng(8)
    return torch.from_numpy(rng.integers(1, 5, case(name).n).astype(np.float32))


@lru_cache(maxsize=None)
def weights(name: str, kind: str):
    """float32 [n] or None: what ``cn_pool(weights=kind)`` uses (``"tensor"``: uniform in [0.5, 1.5))."""
    c = case(name)
    if kind == "tensor":
        return torch.from_numpy((0.5 + np.random.default_rng(9).random(c.n)).astype(np.float32))
    return ncn._host_weights(c.csr, kind)


def dense_pool(name: str, tab: torch.Tensor, w) -> torch.Tensor:
    """((A[a] o A[b]) diag(w)) @ T in fp64 through scipy: the contract without any chunk."""
    M = dense_rows(name)
    if w is not None:
        M = M @ sp.diags(w.numpy().astype(np.float64))
    return torch.from_numpy(np.asarray(M @ tab.numpy().astype(np.float64)))


@lru_cache(maxsize=None)
def reference(name: str, dim: int, kind: str):
    """(ref, mag) float64 [P, dim]: ``cn_pool_reference`` and sum_i |w[u_i] T[u_i]| of the same entries."""
    c, t, w = case(name), table(name, dim), weights(name, kind)
    return ncn.cn_pool_reference(c.csr, c.pairs, t, w), ncn.cn_pool_reference(c.csr, c.pairs, t.abs(), w)


@lru_cache(maxsize=None)
def int_reference(name: str) -> torch.Tensor:
    c = case(name)
    ref = ncn.cn_pool_reference(c.csr, c.pairs, int_table(name), int_weights(name))
    assert float(ref.abs().max()) < 2 ** 24 and torch.equal(ref, ref.round())
    return ref


def forward_bound(name: str, mag: torch.Tensor) -> torch.Tensor:
    k = counts(name).to(torch.float64)
    terms = torch.minimum(k, torch.tensor(float(CHUNK))) + torch.ceil(k / CHUNK) + 1.0
    return 1.01 * U24 * terms[:, None] * mag


def backward_reference(n: int, ent, g: torch.Tensor, w):
    """(dT, bound, occ) for the entries ``ent`` of P pairs on n nodes and an upstream gradient g [P, D], in fp64:
    dT[u] = w[u] sum over the pairs that hold u of g[p]; the backward bound; occ[u] = c, the node's occurrence count."""
    P = ent.seg.numel() - 1
    pos = torch.repeat_interleave(torch.arange(P), ent.seg[1:] - ent.seg[:-1])
    node = ent.node.to(torch.int64)
    g64 = g.to(torch.float64)
    wv = torch.ones(n, dtype=torch.float64) if w is None else w.to(torch.float64)
    dT = torch.zeros((n, g.shape[1]), dtype=torch.float64).index_add_(0, node, g64[pos]) * wv[:, None]
    mag = torch.zeros((n, g.shape[1]), dtype=torch.float64).index_add_(0, node, g64[pos].abs()) * wv.abs()[:, None]
    occ = torch.bincount(node, minlength=n).to(torch.float64)
    terms = torch.minimum(occ, torch.tensor(float(BWD_CHUNK))) + torch.ceil(occ / BWD_CHUNK) + 1.0
    return dT, 1.01 * U24 * terms[:, None] * mag, occ


def clique_pairs(seed: int = 3, m: int = 96):
    """Graph C: m intra-clique pairs (label 1) and m cross-clique pairs (label 0) as (pairs int64 [2, 2 m], labels)."""
    rng, k = np.random.default_rng(seed), DC.CLIQUE
    side = rng.integers(0, 2, m) * k
    intra = np.stack([side + rng.integers(0, k, m), side + rng.integers(0, k, m)])
    cross = np.stack([rng.integers(1, k, m), k + rng.integers(1, k, m)])
    pairs = torch.from_numpy(np.concatenate([intra, cross], axis=1).astype(np.int64))
    return pairs, torch.cat([torch.ones(m), torch.zeros(m)])
