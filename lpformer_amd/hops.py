"""Nodes by distance to both endpoints of candidate pairs on the typing adjacency.

``pair_heuristics``, ``pair_distance`` and ``pair_walks`` say how a and b are connected; ``threshold_profile`` and
``explain`` say what the model selected and attended to, per node class.  ``pair_hop_counts`` says what there was to
select: for a pair (a, b), how many nodes sit at distance i from a and distance j from b.  It is the denominator of
``threshold_profile`` (selected among available, per class), an axis for ``evaluate.metrics_by_bin`` and
``attention_profile`` (pairs with no common neighbour but a thick 2-hop overlap; pairs whose one-hop sets are
disjoint), and, number for number, the structure-feature vector of ELPH / BUDDY, which only estimate these counts with
sketches.  The reference has no such code.

Contract (shared by the kernel, ``lpf_pair_hop_counts`` in csrc/pair_hops.hip, and the numpy restatement below).  The
graph is a binary CSR with sorted, unique int32 columns and a SYMMETRIC pattern -- the typing adjacency the selection
reads; values are ignored; a non-symmetric pattern is outside the contract.  ``hops = k`` is 1 or 2, default 2.

* classes: for a node v and an endpoint u, ``cls_u(v) = d(u, v)`` if that is ``<= k``, else ``k + 1`` (farther than k,
  or unreachable);
* table: for pair p = (a, b), ``T[i][j] = |{v in [0, n) : cls_a(v) = i and cls_b(v) = j}|``: int32 ``[P, k+2, k+2]``.
  The far/far cell ``T[k+1][k+1]`` is included, so a valid pair's table sums to n; row i sums to the number of nodes
  in class i of a, column j to the number in class j of b;
* ``a == b`` is no special case (the table is diagonal); stored self-loops change nothing; an id outside ``[0, n)``
  gives an all-zero table, so a sum of 0 is the flag for a bad id;
* ``ignore_direct=True``: for THIS pair the stored entries (a, b) and (b, a) count as absent when distances are taken
  (the rule of ``pair_distance`` and ``pair_walks``).  A pair that is no stored entry is unaffected; for ``a == b`` the
  skipped entry is the self-loop, which changes no distance.

The result is a pure function of (graph, pair, options): it does not depend on the pair's position in the batch, on
chunking, on the number of workgroups, on the orientation the host chose or on timing; ``(b, a)`` gives the transposed
table; two runs are bitwise equal.  Integers only.

    table = pair_hop_counts(model, pos_edges, test_set=True)              # int32 [P, 4, 4]
    feats = elph_features(table)                                          # [P, 8]: A[1..2, 1..2], B_a[1..2], B_b[1..2]
    evaluate.metrics_by_bin(pos_scores, neg_scores, ball_jaccard(table), bins=...)
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, graph, katz, ops, sources
from ._lib import check, ptr

MAX_HOPS = 2                          # lpf_pair_hop_counts: 1 <= hops <= 2
# Workgroups, workspace and run length: distance.py's / katz.py's constants (katz._units cuts the runs at
# katz.RUN_MAX), chosen for the BFS of pair_distance and NOT tuned for this kernel, whose dense state is 8 n bytes per
# workgroup as pair_walks' is.  tools/pair_hop_counts_time.py sweeps the workgroup count (profiles/
# pair_hop_counts_timing.json: collab-like graph, 32,768 pairs, 256 / 1,024 / 2,048 workgroups against the 1,138 these
# defaults give): hops 2 moves by at most 9 % with no consistent direction, hops 1 is 14-18 % faster at 256, where less
# state is zeroed per call.  Nothing was changed on that; RUN_MAX is not measured for this kernel.
MAX_GROUPS = katz.MAX_GROUPS
ABI_MAX_GROUPS = 65535                # lpf_pair_hop_counts: 1 <= n_groups <= 65535
WORKSPACE_MB = katz.WORKSPACE_MB
MAX_PAIRS = (1 << 30) - 1             # lpf_pair_hop_counts: m < 2^30 pairs per launch (30-bit epoch stamps)


# ---------------------------------------------------------------------------------------------------------- options
def _check_hops(hops) -> int:
    if isinstance(hops, bool) or not isinstance(hops, (int, np.integer)) or not 1 <= int(hops) <= MAX_HOPS:
        raise ValueError(f"hops must be 1 or 2; got {hops!r}")
    return int(hops)


def _check_launch(groups, workspace_mb) -> None:
    if groups is not None and not 1 <= int(groups) <= ABI_MAX_GROUPS:
        raise ValueError(f"groups must be in [1, {ABI_MAX_GROUPS}]; got {groups!r}")
    if not workspace_mb > 0:
        raise ValueError("workspace_mb must be positive")


def _check_table(table) -> int:
    """k of an integer table [P, k+2, k+2]."""
    if (not isinstance(table, torch.Tensor) or table.dim() != 3 or table.shape[1] != table.shape[2] or
            table.shape[1] - 2 not in (1, 2) or table.dtype.is_floating_point or table.dtype == torch.bool):
        raise ValueError("table must be an integer tensor [P, k+2, k+2] with k = 1 or 2")
    return table.shape[1] - 2


# ------------------------------------------------------------------------------------------------- derived features
def elph_features(table: torch.Tensor) -> torch.Tensor:
    """The ELPH / BUDDY structure features of a hop-count table, int64 ``[P, k*k + 2k]`` on the table's device, in this
    order: first ``A[d_a, d_b] = T[d_a][d_b]`` for d_a, d_b in 1 .. k, row-major (d_a the slow index); then
    ``B_a[d] = T[d][k+1]`` for d = 1 .. k (at distance d from a, farther than k from b); then ``B_b[d] = T[k+1][d]``."""
    k = _check_table(table)
    t = table.to(torch.int64)
    return torch.cat([t[:, 1:k + 1, 1:k + 1].reshape(t.shape[0], k * k), t[:, 1:k + 1, k + 1], t[:, k + 1, 1:k + 1]],
                     dim=1)


def ball_jaccard(table: torch.Tensor) -> torch.Tensor:
    """float32 ``[P]`` = |B_k(a) & B_k(b)| / |B_k(a) | B_k(b)|, B_k(u) the nodes within k hops of u (u included): the
    intersection is the sum of the cells T[i][j] with i, j <= k, the union every cell but far/far.  Computed from the
    table in fp64 (one division) and rounded once; 0 where the union is empty, which happens only for a bad id.  A
    ready axis for ``metrics_by_bin`` / ``attention_profile``."""
    k = _check_table(table)
    t = table.to(torch.int64)
    inter = t[:, :k + 1, :k + 1].sum(dim=(1, 2))
    union = t.sum(dim=(1, 2)) - t[:, k + 1, k + 1]
    ratio = inter.to(torch.float64) / union.clamp(min=1).to(torch.float64)
    return torch.where(union > 0, ratio, torch.zeros_like(ratio)).to(torch.float32)


# ------------------------------------------------------------------------------------------------- host restatement
def hop_counts_reference(adj: graph.CSR, edges, *, hops=2, ignore_direct: bool = False) -> torch.Tensor:
    """``pair_hop_counts`` of a host CSR in numpy (a CPU int32 tensor [P, k+2, k+2] out): per distinct endpoint a
    level-by-level breadth-first search of k levels gives (node ids, classes) of its ball; a pair's near cells are a
    2-D histogram of (class of a, class of b) over b's ball, the far row and column are the class sizes minus those, the
    far/far cell what is left of n.  Pairs that are stored entries get balls of their own, without the pair's
    transitions, under ``ignore_direct``.  The restatement the device kernel is tested against, and what
    ``pair_hop_counts`` runs when there is no GPU."""
    k = _check_hops(hops)
    batch = sources.as_pairs(edges).cpu().to(torch.int64).numpy()
    a, b = batch[0], batch[1]
    n = int(adj.n)
    rowptr, col = np.asarray(adj.rowptr, np.int64), np.asarray(adj.col)
    out = np.zeros((a.size, k + 2, k + 2), np.int32)
    idx = np.flatnonzero((a >= 0) & (a < n) & (b >= 0) & (b < n))
    if not idx.size:
        return torch.from_numpy(out)
    far = k + 1
    dense = np.full(n, far, np.int8)           # scratch: the classes of the endpoint in hand; reset after use

    def ball(u, drop):
        """(ids, classes) of the nodes within k hops of u, by levels; ``drop`` = (a, b): without the transitions
        {a, b}."""
        ids, cls = [np.array([u], np.int64)], [np.zeros(1, np.int8)]
        dense[u] = 0
        front = ids[0]
        for d in range(1, k + 1):
            flat, pos = sources.csr_rows(rowptr, front)
            dst, src = col[flat].astype(np.int64), front[pos]
            keep = (dst >= 0) & (dst < n)
            if drop is not None:
                keep &= ~(((src == drop[0]) & (dst == drop[1])) | ((src == drop[1]) & (dst == drop[0])))
            dst = dst[keep]
            dst = dst[dense[dst] == far]
            dense[dst] = d                     # (repeats write the same level)
            front = np.unique(dst)
            ids.append(front)
            cls.append(np.full(front.size, d, np.int8))
        ids, cls = np.concatenate(ids), np.concatenate(cls)
        dense[ids] = far
        return ids, cls

    def table(i, xa, xb):
        dense[xa[0]] = xa[1]
        near = np.bincount(dense[xb[0]].astype(np.int64) * (k + 2) + xb[1], minlength=(k + 2) ** 2)
        dense[xa[0]] = far
        t = near.reshape(k + 2, k + 2).astype(np.int64)        # row k+1: in b's ball, far from a; column k+1 empty
        t[:far, far] = np.bincount(xa[1], minlength=far) - t[:far, :far].sum(axis=1)
        t[far, far] = n - t.sum()
        out[i] = t

    own = np.zeros(idx.size, bool)             # pairs that get balls of their own: their edge is removed
    if ignore_direct and col.size:
        keys = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr)) * n + col.astype(np.int64)
        q = a[idx] * n + b[idx]
        own = keys[np.minimum(np.searchsorted(keys, q), keys.size - 1)] == q
        for i in idx[own]:
            drop = (a[i], b[i])
            table(i, ball(a[i], drop), ball(b[i], drop))
    balls: dict = {}                           # per distinct endpoint
    for i in idx[~own]:
        for u in (a[i], b[i]):
            if u not in balls:
                balls[u] = ball(u, None)
        table(i, balls[a[i]], balls[b[i]])
    return torch.from_numpy(out)


# ------------------------------------------------------------------------------------------------------ device path
def default_groups(n: int, pairs: int, workspace_mb=WORKSPACE_MB) -> int:
    """The largest number of workgroups whose workspace (``lpf_pair_hop_counts_workspace_bytes``: 16 bytes, then 8 n
    each) fits ``workspace_mb``, clamped to [1, min(pairs, MAX_GROUPS)]."""
    hip = _lib.hip()
    n = max(int(n), 1)
    one = int(hip.lpf_pair_hop_counts_workspace_bytes(n, 1))
    each = int(hip.lpf_pair_hop_counts_workspace_bytes(n, 2)) - one
    fit = (int(workspace_mb * (1 << 20)) - (one - each)) // each
    return int(max(1, min(fit, int(pairs), MAX_GROUPS)))


@torch.no_grad()
def pair_hop_counts(source, edges, *, hops=2, test_set: bool = False, ignore_direct: bool = False,
                    chunk: int = 1 << 20, groups=None, workspace_mb=WORKSPACE_MB) -> torch.Tensor:
    """The hop-count tables of ``edges`` ([P, 2] or [2, P], host or device) on the typing adjacency: int32
    [P, k+2, k+2], ``T[i][j]`` = the nodes in class i of a and class j of b, by the module docstring's contract.

    ``source``: a ``LinkTransformer`` (the typing adjacency of the split ``test_set`` selects, the same resident object
    the selection, ``pair_heuristics``, ``pair_distance`` and ``pair_walks`` read), a ``graph.CSR`` or a
    ``graph.DeviceCSR`` (binary SYMMETRIC pattern: values are ignored, a non-symmetric pattern is outside the
    contract).  ``hops``: 1 or 2.  ``ignore_direct``: leave each pair's own edge out of its distances.  ``chunk``:
    pairs per launch.  ``groups``: workgroups, each with 8 n bytes of dense state (default: as many as fit
    ``workspace_mb``, at most min(P, 2048)).  The result depends on none of the last three.

    The pairs are oriented, sorted and cut into units by ``katz._units`` (the endpoint that occurs more often in the
    launch is spread once for all its pairs; on a tie the side with the smaller two-hop row sum E2 is expanded, so a
    pair costs E2 of its cheaper side in touches); where that spread b instead of a, the pair's table is transposed
    back on the device.  The result is a device tensor; nothing is read back.  A host ``graph.CSR`` with CPU ``edges``
    and no GPU present goes through ``hop_counts_reference`` and gives a CPU tensor."""
    k = _check_hops(hops)
    _check_launch(groups, workspace_mb)
    chunk = min(sources.clamp_chunk(chunk), MAX_PAIRS)
    batch = sources.as_pairs(edges)
    dev, adj, _, _ = sources.resolve(source, test_set, batch, who="pair_hop_counts", host_ok=True)
    if dev is None:
        return hop_counts_reference(adj, batch, hops=k, ignore_direct=ignore_direct)
    batch = batch.to(dev, dtype=torch.int64).contiguous()
    P = batch.shape[1]
    with torch.cuda.device(dev):
        if P == 0 or adj.n <= 0:
            return torch.zeros((P, k + 2, k + 2), dtype=torch.int32, device=dev)
        table = torch.empty((P, k + 2, k + 2), dtype=torch.int32, device=dev)
        hip = _lib.hip()
        m_max = min(P, chunk)
        n_groups = int(groups) if groups is not None else default_groups(adj.n, m_max, workspace_mb)
        nbytes = int(hip.lpf_pair_hop_counts_workspace_bytes(adj.n, n_groups))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        st = ops.raw_stream(dev)
        for lo, m in sources.chunks(P, chunk):
            a = batch[0, lo:lo + m]
            pairs, unit_ptr, order = katz._units(adj, a, batch[1, lo:lo + m], bool(ignore_direct))
            part = torch.empty((m, k + 2, k + 2), dtype=torch.int32, device=dev)
            check(hip.lpf_pair_hop_counts(m, adj.n, ptr(pairs), m, ptr(adj.rowptr), ptr(adj.col), k,
                                          1 if ignore_direct else 0, ptr(unit_ptr), ptr(ws), n_groups, ptr(part), st),
                  "lpf_pair_hop_counts")
            # the kernel wrote T[class of s][class of t]: transpose where s is not the pair's a (a pair with a bad id
            # holds zeros either way, and a == b a symmetric table)
            flipped = (pairs[0] != a[order]).view(m, 1, 1)
            table[lo:lo + m].index_copy_(0, order, torch.where(flipped, part.transpose(1, 2), part))
    return table
