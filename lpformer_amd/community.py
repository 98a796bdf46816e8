"""Louvain communities of the typing adjacency, on the device.

``node_structure`` describes a node by its degree, core number, component and triangles; on every graph we use the
component is one giant label.  ``communities`` gives the level between a node's neighbourhood and its component: a
partition by modularity, so that a positive can be called intra- or inter-community (``same_community``) and a
``recommend`` list can be checked for where it concentrates.  The reference has no such code; the host baseline is
``networkx.community.louvain_communities``.

Contract (shared by the kernels of csrc/community.hip and the numpy restatement below).  The graph is the simple
undirected graph of a binary CSR with sorted, unique int32 columns and a SYMMETRIC pattern, the contract of
``structure.py``: ``u ~ v`` iff ``u != v`` and v is in row u; values are ignored, stored self-loops are skipped.

Level graph.  A level works on a weighted graph: int64 weights ``w(u, v)`` (level 0: all 1) and an int64 self weight
``s[v]`` (level 0: all 0).  ``k[v] = sum_{u != v} w(v, u) + s[v]``, ``2m = sum k`` -- the same at every level -- and
``2m < 2^31``, so every product below is below 2^62.

Quality.  ``Qnum(comm) = 2m inside - sum_c tot_c^2`` with ``tot_c`` the sum of k over c and ``inside = sum s +`` the sum
of w over the stored entries (both directions) that join equal communities: an exact integer; the modularity is
``Qnum / (2m)^2``, one fp64 division.

One round r of level l reads the accepted ``comm`` / ``tot`` / ``cnt`` and writes ``new``.  Node v is ACTIVE iff the top
bit of ``mix64(key(seed, (l << 32) + r) + G (v + 1))`` is set (the draw of ``negatives.py``); an inactive node keeps its
community.  An active node with ``cur = comm[v]`` visits every community C among its neighbours' communities, ``w_C`` the
weight of its entries into C::

    gain(C) = 2m w_C - k_v (tot_C - [C = cur] k_v)          stay = gain(cur), w_cur = 0 with no neighbour in cur

A candidate is a ``C != cur`` with ``gain(C) > stay``; it is dropped when ``cnt[cur] == 1 and cnt[C] == 1 and C > cur``
(two singletons may not swap).  The largest gain wins, ties to the smaller id; a node with no candidate stays.

A level starts from the identity with ``q = Qnum``, ``stall = 0``.  Each round computes ``new`` and ``qn = Qnum(new)``;
``stall`` becomes 0 if ``qn - q >= min_gain`` and ``stall + 1`` otherwise; the round is ACCEPTED iff ``qn > q`` (then
``comm, q = new, qn``; else ``comm`` stays).  The level ends at ``stall == patience`` or after ``max_rounds`` rounds;
``min_gain = max(1, floor(tolerance (2m)^2))``.  q never falls.  Between levels the community ids are ranked densely in
ascending order, the coarse graph sums w by (rank, rank), and its diagonal goes into ``s'`` together with the members'
``s``.  The run stops at a level that accepted no round (that level is discarded), after ``max_levels`` levels, or when
``2m == 0``.  Labels are composed over the levels and every community is named by the SMALLEST ORIGINAL NODE ID in it
(the convention of ``component``); an isolated node is its own community.

The result is a pure function of (graph, seed, options): integers only, two runs are bitwise equal, and the device
equals ``communities_reference`` integer for integer.  There is no incremental refresh under ``update_graph``.

    c = communities(model, test_set=True)
    intra = same_community(c, pos_edges)                     # bool [P]
    evaluate.metrics_by_bin(pos, neg, intra.to(torch.int64), bins=COMMUNITY_BINS)
    evaluate.metrics_by_bin(pos, neg, pair_node_values(c.size, pos_edges), bins=...)   # community size as an axis
    partition_quality(model, ns.component)                   # (Qnum, 2m) of any labelling
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np
import torch

from . import _lib, graph, negatives, ops, sources, structure
from ._lib import check, ptr

COMMUNITY_BINS = ((0, 1), (1, 2))     # same_community(...).to(int64): inter-community, intra-community
LONG_ROW = _lib.CONST["LPF_COMM_LONG_ROW"]
LDS_SLOTS = _lib.CONST["LPF_COMM_LDS_SLOTS"]
LDS_SLOTS_MAX = _lib.CONST["LPF_COMM_LDS_SLOTS_MAX"]
_TWO_M_MAX = 1 << 31                  # 2m < 2^31
_MAX = (1 << 31) - 2                  # n, nnz < 2^31 - 1


# ----------------------------------------------------------------------------------------------------------- result
@dataclass
class Communities:
    """``label`` int32 [n]: the smallest original node id of each node's community; ``count`` communities; ``two_m``,
    ``quality_num`` (the exact modularity numerator, a Python int) and ``modularity = quality_num / two_m^2`` (0.0 for a
    graph without edges); ``levels``: per KEPT level ``{"nodes", "rounds", "accepted", "quality_num"}`` (the nodes of
    the level graph, the rounds run and accepted, Qnum at its end); ``hierarchy``: the label after each kept level, named
    the same way (``hierarchy[-1]`` is ``label``)."""
    n: int
    label: torch.Tensor
    count: int
    two_m: int
    quality_num: int
    modularity: float
    levels: list = field(default_factory=list)
    hierarchy: list = field(default_factory=list)

    @property
    def size(self) -> torch.Tensor:
        """int64 [n]: the number of nodes in each node's community."""
        label = self.label.to(torch.int64)
        return torch.bincount(label, minlength=self.n)[label]

    def summary(self) -> dict:
        """``communities``, ``largest_share`` (of the nodes), ``median_size`` (over the communities), ``modularity`` and
        ``levels`` (kept) as a plain dict."""
        sizes = torch.bincount(self.label.to(torch.int64), minlength=self.n) if self.n else torch.zeros(0, dtype=torch.int64)
        sizes = sizes[sizes > 0]
        return {"communities": int(sizes.numel()),
                "largest_share": float(sizes.max()) / self.n if self.n else 0.0,
                "median_size": float(sizes.to(torch.float64).median()) if self.n else 0.0,
                "modularity": self.modularity, "levels": len(self.levels)}


def same_community(c: Communities, edges) -> torch.Tensor:
    """bool [P]: whether the endpoints of each pair share a community; False for a pair with an id outside ``[0, n)``
    (the semantics of ``same_component``)."""
    batch = sources.as_pairs(edges).to(c.label.device, dtype=torch.int64)
    ok = ((batch >= 0) & (batch < c.n)).all(dim=0)
    if c.n == 0:
        return ok
    safe = torch.where(ok.unsqueeze(0), batch, torch.zeros_like(batch))
    return ok & (c.label[safe[0]] == c.label[safe[1]])


# ---------------------------------------------------------------------------------------------------------- options
def _check_options(seed, max_levels, max_rounds, tolerance, patience, lds_slots):
    seed = negatives._check_seed(seed)
    max_levels = structure._check_count(max_levels, "max_levels")
    max_rounds = structure._check_count(max_rounds, "max_rounds")
    patience = structure._check_count(patience, "patience")
    if isinstance(tolerance, bool) or not isinstance(tolerance, (int, float, np.integer, np.floating)) or \
            not 0.0 <= float(tolerance) < 1.0:
        raise ValueError(f"tolerance must be a number in [0, 1); got {tolerance!r}")
    if lds_slots is not None:
        lds_slots = structure._check_count(lds_slots, "lds_slots")
        if not 64 <= lds_slots <= LDS_SLOTS_MAX or lds_slots & (lds_slots - 1):
            raise ValueError(f"lds_slots must be a power of two in [64, {LDS_SLOTS_MAX}]; got {lds_slots}")
    return seed, max_levels, max_rounds, float(tolerance), patience, lds_slots


def _min_gain(tolerance: float, two_m: int) -> int:
    """``max(1, floor(tolerance (2m)^2))`` in Python integers: the float is taken as the exact rational it is."""
    return max(1, math.floor(Fraction(tolerance) * two_m * two_m))


def _check_two_m(two_m: int, who: str):
    if two_m >= _TWO_M_MAX:
        raise ValueError(f"{who}: the graph must have fewer than 2^30 undirected edges (2m < 2^31); got 2m = {two_m}")


def _result(n, label, two_m, q, levels, hierarchy) -> Communities:
    count = int(torch.unique(label).numel()) if n else 0
    return Communities(n, label, count, two_m, q, q / (two_m * two_m) if two_m else 0.0, levels, hierarchy)


# ------------------------------------------------------------------------------------------------- host restatement
def active_nodes(seed: int, level: int, rnd: int, n: int) -> np.ndarray:
    """bool [n]: the activation bit of round ``rnd`` of level ``level``."""
    key = negatives.draw_key(seed, (int(level) << 32) + int(rnd))
    with np.errstate(over="ignore"):
        z = negatives.mix64_np(key + np.uint64(negatives.G) * (np.arange(n, dtype=np.uint64) + np.uint64(1)))
    return (z >> np.uint64(63)).astype(bool)


def _entry_rows(indptr) -> np.ndarray:
    return np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr))


def _sum_by_key(key, values):
    """(unique keys ascending, the int64 sum of ``values`` per key)."""
    if key.size == 0:
        return key, values
    order = np.argsort(key, kind="stable")
    uniq, start = np.unique(key[order], return_index=True)
    return uniq, np.add.reduceat(values[order], start)


def move_round_reference(indptr, indices, weight, k, comm, tot, cnt, two_m, seed, level, rnd) -> np.ndarray:
    """One round of local moves in numpy, what ``lpf_community_move`` computes: ``new`` int64 [n] from the accepted
    ``comm`` / ``tot`` / ``cnt`` of a level graph (``weight`` None: all 1).  The neighbour-community weights are the
    sparse n x n sum of w over (node, community of the neighbour); the arg-max is a ``lexsort``."""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices).astype(np.int64)
    k, comm, tot, cnt = (np.asarray(a).astype(np.int64) for a in (k, comm, tot, cnt))
    n, two_m = k.size, int(two_m)
    rows = _entry_rows(indptr)
    act = active_nodes(seed, level, rnd, n)
    keep = (rows != indices) & act[rows]
    w = np.ones(int(keep.sum()), np.int64) if weight is None else np.asarray(weight, np.int64)[keep]
    nodes = np.nonzero(act)[0]
    # (v, community, weight) of every entry of an active row, and (v, cur, 0): the stay term exists for every active node
    r = np.concatenate([rows[keep], nodes])
    c = np.concatenate([comm[indices[keep]], comm[nodes]])
    uniq, w_c = _sum_by_key(r * n + c, np.concatenate([w, np.zeros(nodes.size, np.int64)]))
    v, c = uniq // max(n, 1), uniq % max(n, 1)
    cur = comm[v]
    is_cur = c == cur
    gain = two_m * w_c - k[v] * (tot[c] - is_cur * k[v])
    stay = np.zeros(n, np.int64)
    stay[v[is_cur]] = gain[is_cur]
    cand = ~is_cur & (gain > stay[v]) & ~((cnt[cur] == 1) & (cnt[c] == 1) & (c > cur))
    v, c, gain = v[cand], c[cand], gain[cand]
    order = np.lexsort((c, -gain, v))                        # by node, then gain descending, then id ascending
    v, c = v[order], c[order]
    first = np.ones(v.size, bool)
    first[1:] = v[1:] != v[:-1]
    new = comm.copy()
    new[v[first]] = c[first]
    return new


def _sum_at(index, values, n) -> np.ndarray:
    out = np.zeros(n, np.int64)
    np.add.at(out, index, values)
    return out


def quality_reference(indptr, indices, weight, s, k, comm) -> int:
    """``Qnum(comm)`` of a level graph as a Python int; ``comm`` may hold any integer labels."""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices).astype(np.int64)
    comm = np.asarray(comm).astype(np.int64)
    rows = _entry_rows(indptr)
    same = (rows != indices) & (comm[rows] == comm[indices])
    inside = int(same.sum()) if weight is None else int(np.asarray(weight, np.int64)[same].sum())
    inside += 0 if s is None else int(np.asarray(s, np.int64).sum())
    k = np.asarray(k, np.int64)
    _, dense = np.unique(comm, return_inverse=True)
    tot = _sum_at(dense.ravel(), k, k.size)
    return int(k.sum()) * inside - sum(t * t for t in tot[tot > 0].tolist())


def _coarsen_reference(indptr, indices, weight, s, k, comm):
    """(rank of every node's community, the coarse level graph): ids ranked densely ascending, w summed by (rank, rank),
    the diagonal moved into s' with the members' s."""
    uniq, rank = np.unique(comm, return_inverse=True)
    rank = rank.ravel().astype(np.int64)
    nc = uniq.size
    rows = _entry_rows(indptr)
    keep = rows != indices
    w = np.ones(int(keep.sum()), np.int64) if weight is None else weight[keep]
    key, wsum = _sum_by_key(rank[rows[keep]] * nc + rank[indices[keep]], w)
    ru, rv = key // nc, key % nc
    s2 = _sum_at(rank, s, nc) if s is not None else np.zeros(nc, np.int64)
    diag = ru == rv
    s2[ru[diag]] += wsum[diag]
    ru, rv, wsum = ru[~diag], rv[~diag], wsum[~diag]
    indptr2 = np.concatenate([[0], np.cumsum(np.bincount(ru, minlength=nc))]).astype(np.int64)
    return rank, (indptr2, rv, wsum, s2, _sum_at(rank, k, nc))


def _named_by_smallest(lab: np.ndarray, n: int) -> np.ndarray:
    first = np.full(int(lab.max()) + 1 if n else 0, n, np.int64)
    np.minimum.at(first, lab, np.arange(n))
    return first[lab].astype(np.int32)


def communities_reference(adj: graph.CSR, *, seed: int = 0, max_levels: int = 16, max_rounds: int = 64,
                          tolerance: float = 1e-6, patience: int = 3) -> Communities:
    """``communities`` of a host CSR in numpy (CPU tensors out): the schedule of the module docstring, vectorised -- the
    restatement the kernels are tested against integer for integer, and what ``communities`` runs when there is no
    GPU."""
    seed, max_levels, max_rounds, tolerance, patience, _ = _check_options(seed, max_levels, max_rounds, tolerance,
                                                                          patience, None)
    n = int(adj.n)
    A = structure._simple(adj)
    indptr, indices = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    weight, s = None, None
    k = np.diff(indptr).astype(np.int64)
    two_m = int(k.sum())
    _check_two_m(two_m, "communities_reference")
    lab = np.arange(n, dtype=np.int64)                       # level node of every original node
    q = -sum(x * x for x in k.tolist())                      # Qnum of the singletons
    levels, hierarchy = [], []
    min_gain = _min_gain(tolerance, two_m)
    for level in range(max_levels if two_m else 0):
        nl = k.size
        comm = np.arange(nl, dtype=np.int64)
        tot, cnt = k.copy(), np.ones(nl, np.int64)
        lq = quality_reference(indptr, indices, weight, s, k, comm)
        stall = rounds = accepted = 0
        while stall < patience and rounds < max_rounds:
            new = move_round_reference(indptr, indices, weight, k, comm, tot, cnt, two_m, seed, level, rounds)
            qn = quality_reference(indptr, indices, weight, s, k, new)
            stall = 0 if qn - lq >= min_gain else stall + 1
            rounds += 1
            if qn > lq:
                comm, lq, accepted = new, qn, accepted + 1
                tot, cnt = _sum_at(comm, k, nl), np.bincount(comm, minlength=nl).astype(np.int64)
        if accepted == 0:
            break
        rank, (indptr, indices, weight, s, k) = _coarsen_reference(indptr, indices, weight, s, k, comm)
        lab, q = rank[lab], lq
        levels.append({"nodes": nl, "rounds": rounds, "accepted": accepted, "quality_num": lq})
        hierarchy.append(torch.from_numpy(_named_by_smallest(lab, n)))
    label = hierarchy[-1] if hierarchy else torch.arange(n, dtype=torch.int32)
    return _result(n, label, two_m, q, levels, hierarchy)


# ------------------------------------------------------------------------------------------------------ device path
class _Level:
    """A level graph on the device: the CSR, the row id of every entry, int64 weights and self weights (None at level
    0), k, and what the move kernel needs beside them (the listed rows, the table size, the zeroed scratch)."""

    def __init__(self, rowptr, col, row, weight, s, k, lds_slots):
        self.rowptr, self.col, self.row, self.weight, self.s, self.k = rowptr, col, row, weight, s, k
        self.n, self.nnz = int(k.numel()), int(col.numel())
        lens = rowptr[1:] - rowptr[:-1]
        self.long_rows = torch.nonzero(lens > LONG_ROW).flatten().to(torch.int32)
        n_long = int(self.long_rows.numel())
        longest = int(lens.max()) if n_long else 0
        if lds_slots is None:
            # no more LDS than the longest row's table needs: the short rows share the launch and its LDS
            lds_slots = min(LDS_SLOTS, max(64, 1 << (2 * longest - 1).bit_length())) if n_long else 64
        self.lds_slots = lds_slots
        nbytes = int(_lib.hip().lpf_community_workspace_bytes(n_long, longest, lds_slots))
        if nbytes < 0:
            check(nbytes, "lpf_community_workspace_bytes")
        self.scratch = torch.zeros(nbytes, dtype=torch.uint8, device=k.device) if nbytes else None
        self.s_sum = s.sum() if s is not None else torch.zeros((), dtype=torch.int64, device=k.device)


def _inside(hip, st, lv: _Level, comm, out):
    check(hip.lpf_community_quality(lv.n, lv.nnz, ptr(lv.row), ptr(lv.col), ptr(lv.weight), ptr(comm), ptr(out), st),
          "lpf_community_quality")
    return out[0]


def _run_level(hip, st, lv: _Level, two_m, seed, level, max_rounds, min_gain, patience):
    """(comm int32 [n], Qnum, rounds, accepted) of one level.  ONE scalar read-back per round decides accept / reject:
    a round reads the accepted state, so it cannot be queued behind an undecided one."""
    dev, n = lv.k.device, lv.n
    comm = torch.arange(n, dtype=torch.int32, device=dev)
    new = torch.empty_like(comm)
    tot, cnt = lv.k.clone(), torch.ones(n, dtype=torch.int32, device=dev)
    moved = torch.zeros(1, dtype=torch.int32, device=dev)    # (counted over the level, not read: the accept needs Qnum)
    inside = torch.empty(1, dtype=torch.int64, device=dev)
    q = int(two_m * lv.s_sum - (lv.k * lv.k).sum())          # the identity joins no entry
    n_long = int(lv.long_rows.numel())
    stall = rounds = accepted = 0
    while stall < patience and rounds < max_rounds:
        check(hip.lpf_community_move(n, lv.nnz, ptr(lv.rowptr), ptr(lv.col), ptr(lv.weight), ptr(lv.k), ptr(comm),
                                     ptr(tot), ptr(cnt), two_m, seed, level, rounds,
                                     ptr(lv.long_rows) if n_long else None, n_long, lv.lds_slots, ptr(lv.scratch),
                                     int(lv.scratch.numel()) if lv.scratch is not None else 0, ptr(new), ptr(moved),
                                     st), "lpf_community_move")
        tot_n = torch.zeros_like(tot).index_add_(0, new.to(torch.int64), lv.k)
        qn = int(two_m * (_inside(hip, st, lv, new, inside) + lv.s_sum) - (tot_n * tot_n).sum())   # the read-back
        stall = 0 if qn - q >= min_gain else stall + 1
        rounds += 1
        if qn > q:
            comm, new, q, accepted = new, comm, qn, accepted + 1
            tot, cnt = tot_n, torch.bincount(comm.to(torch.int64), minlength=n).to(torch.int32)
    return comm, q, rounds, accepted


def _coarsen(lv: _Level, comm, lds_slots):
    """(rank int64 [n], the coarse ``_Level``): torch sort / unique_consecutive / index_add_ on the device."""
    dev = lv.k.device
    uniq, rank = torch.unique(comm, return_inverse=True)
    nc = int(uniq.numel())
    row, col = lv.row.to(torch.int64), lv.col.to(torch.int64)
    keep = row != col
    w = lv.weight[keep] if lv.weight is not None else torch.ones(int(keep.sum()), dtype=torch.int64, device=dev)
    key, order = torch.sort(rank[row[keep]] * nc + rank[col[keep]])
    key, inverse = torch.unique_consecutive(key, return_inverse=True)
    wsum = torch.zeros(key.numel(), dtype=torch.int64, device=dev).index_add_(0, inverse, w[order])
    ru, rv = key // nc, key % nc
    s2 = torch.zeros(nc, dtype=torch.int64, device=dev)
    if lv.s is not None:
        s2.index_add_(0, rank, lv.s)
    diag = ru == rv
    s2.index_add_(0, ru[diag], wsum[diag])
    ru, rv, wsum = ru[~diag], rv[~diag], wsum[~diag]
    rowptr = torch.zeros(nc + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(ru, minlength=nc), 0, out=rowptr[1:])
    k2 = torch.zeros(nc, dtype=torch.int64, device=dev).index_add_(0, rank, lv.k)
    return rank, _Level(rowptr, rv.to(torch.int32).contiguous(), ru.to(torch.int32).contiguous(), wsum.contiguous(),
                        s2, k2, lds_slots)


def _named_by_smallest_device(lab: torch.Tensor, n: int, count: int) -> torch.Tensor:
    ids = torch.arange(n, dtype=torch.int64, device=lab.device)
    first = torch.full((count,), n, dtype=torch.int64, device=lab.device).scatter_reduce_(0, lab, ids, "amin")
    return first[lab].to(torch.int32)


def _degree(hip, st, adj: graph.DeviceCSR) -> torch.Tensor:
    deg = torch.empty(adj.n, dtype=torch.int32, device=adj.rowptr.device)
    check(hip.lpf_node_degree(adj.n, adj.nnz, ptr(adj.rowptr), ptr(adj.col), ptr(deg), st), "lpf_node_degree")
    return deg.to(torch.int64)


def _resolve(source, test_set, who):
    dev, adj, _, _ = sources.resolve(source, test_set, torch.empty(0), who=who, host_ok=True)
    if dev is not None and (int(adj.n) > _MAX or int(adj.nnz) > _MAX):
        raise ValueError(f"{who}: the graph must have fewer than 2^31 - 1 nodes and stored entries")
    return dev, adj


@torch.no_grad()
def communities(source, *, test_set: bool = False, seed: int = 0, max_levels: int = 16, max_rounds: int = 64,
                tolerance: float = 1e-6, patience: int = 3, lds_slots=None) -> Communities:
    """Louvain communities of the typing adjacency by the module docstring's schedule: a ``Communities`` of device
    tensors, equal to ``communities_reference`` integer for integer.

    ``source``: a ``LinkTransformer`` (the typing adjacency of the split ``test_set`` selects), a ``graph.CSR`` or a
    ``graph.DeviceCSR`` (binary SYMMETRIC pattern, fewer than 2^30 undirected edges).  A host ``graph.CSR`` with no GPU
    present goes through ``communities_reference`` and gives CPU tensors.

    Each round is one launch of ``lpf_community_move`` (rows of at most LPF_COMM_LONG_ROW entries eight lanes each with
    the row in registers; longer rows a workgroup each with an open-addressing table in LDS, or in device memory for a
    row of more than ``lds_slots / 2`` entries), ``tot`` / ``cnt`` / sum tot^2 in torch, ``lpf_community_quality`` for the
    inside weight, and ONE scalar read-back that decides accept / reject.  The coarse graph between levels is torch
    sort / ``unique_consecutive`` / ``index_add_`` on the device.  ``lds_slots``: slots of the LDS table, a power of two
    in [64, LPF_COMM_LDS_SLOTS_MAX]; default: LPF_COMM_LDS_SLOTS, or less where the longest row of a level needs less;
    the result is the same for every value (a small one is how tests reach the device-memory table)."""
    seed, max_levels, max_rounds, tolerance, patience, lds_slots = _check_options(seed, max_levels, max_rounds,
                                                                                  tolerance, patience, lds_slots)
    dev, adj = _resolve(source, test_set, "communities")
    if dev is None:
        return communities_reference(adj, seed=seed, max_levels=max_levels, max_rounds=max_rounds, tolerance=tolerance,
                                     patience=patience)
    n, nnz = int(adj.n), int(adj.nnz)
    with torch.cuda.device(dev):
        identity = torch.arange(n, dtype=torch.int32, device=dev)
        if n == 0 or nnz == 0:
            return _result(n, identity, 0, 0, [], [])
        hip, st = _lib.hip(), ops.raw_stream(dev)
        k = _degree(hip, st, adj)
        two_m = int(k.sum())
        _check_two_m(two_m, "communities")
        if two_m == 0:
            return _result(n, identity, 0, 0, [], [])
        q = -int((k * k).sum())
        lv = _Level(adj.rowptr, adj.col, structure.entry_rows(adj), None, None, k, lds_slots)
        lab = torch.arange(n, dtype=torch.int64, device=dev)
        levels, hierarchy = [], []
        min_gain = _min_gain(tolerance, two_m)
        for level in range(max_levels):
            comm, lq, rounds, accepted = _run_level(hip, st, lv, two_m, seed, level, max_rounds, min_gain, patience)
            if accepted == 0:
                break
            rank, coarse = _coarsen(lv, comm, lds_slots)
            lab, q = rank[lab], lq
            levels.append({"nodes": lv.n, "rounds": rounds, "accepted": accepted, "quality_num": lq})
            hierarchy.append(_named_by_smallest_device(lab, n, coarse.n))
            lv = coarse
        return _result(n, hierarchy[-1] if hierarchy else identity, two_m, q, levels, hierarchy)


@torch.no_grad()
def partition_quality(source, label, *, test_set: bool = False):
    """``(quality_num, two_m)`` of ANY labelling of the typing adjacency: the exact modularity numerator
    ``2m inside - sum_c tot_c^2`` as a Python int (modularity = quality_num / two_m^2).  ``label``: [n] integers (a
    tensor or an array; equal values are one part) -- ``ns.component``, a ``hierarchy`` level, a partition of one's own.
    On the device through ``lpf_community_quality``; a host ``graph.CSR`` with no GPU present runs the restatement."""
    dev, adj = _resolve(source, test_set, "partition_quality")
    n = int(adj.n)
    label = torch.as_tensor(label)
    if label.dim() != 1 or label.shape[0] != n or label.dtype.is_floating_point or label.dtype == torch.bool:
        raise ValueError(f"label must hold one integer per node ([{n}]); got {tuple(label.shape)} {label.dtype}")
    if dev is None:
        A = structure._simple(adj)
        k = np.diff(A.indptr).astype(np.int64)
        two_m = int(k.sum())
        _check_two_m(two_m, "partition_quality")
        return quality_reference(A.indptr, A.indices, None, None, k, label.numpy()), two_m
    with torch.cuda.device(dev):
        if n == 0 or adj.nnz == 0:
            return 0, 0
        hip, st = _lib.hip(), ops.raw_stream(dev)
        k = _degree(hip, st, adj)
        two_m = int(k.sum())
        _check_two_m(two_m, "partition_quality")
        _, dense = torch.unique(label.to(dev), return_inverse=True)
        comm = dense.to(torch.int32)
        inside = torch.empty(1, dtype=torch.int64, device=dev)
        check(hip.lpf_community_quality(n, adj.nnz, ptr(structure.entry_rows(adj)), ptr(adj.col), None, ptr(comm),
                                        ptr(inside), st), "lpf_community_quality")
        tot = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, dense, k)
        return int(two_m * inside[0] - (tot * tot).sum()), two_m
