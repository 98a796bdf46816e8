"""Shortest-path hops between the endpoints of candidate pairs on the typing adjacency.

The global structural heuristic next to ``pair_heuristics`` (local: CN / AA / RA; PPR; features): how many edges apart
a and b are.  It is the "shortest path" baseline of HeaRT / OGB comparisons, the natural axis for "how does the model do
on pairs 2 / 3 / 4+ hops apart", and it tells whether a ``recommend`` result closes a two-hop path or is a long-range
link.  The reference has no such code; on the host it takes a scipy ``shortest_path`` per batch.

Contract (shared by the kernel, ``lpf_pair_bfs`` in csrc/pair_bfs.hip, and the numpy restatement below).  The graph is a
binary CSR with sorted, unique int32 columns and a SYMMETRIC pattern -- the typing adjacency the selection reads; values
are ignored; a non-symmetric pattern is outside the contract.  For pair p = (a, b), by the first rule that applies:

* ``a == b``: 0, whatever the options;
* an id outside ``[0, n)``: -1;
* otherwise the number of edges on a shortest a-b path, -1 when there is none;
* ``ignore_direct=True``: the stored entries (a, b) and (b, a) of THIS pair are treated as absent and nothing else
  changes (the usual way to value a training positive that is itself in the graph; a pair that is no edge is unaffected);
* ``max_dist=m``: a distance above m reads -1, element for element ``where(exact <= m, exact, -1)``; the search stops as
  soon as that is decided;
* stored self-loops change nothing.

The result is a pure function of (graph, pair, options): it does not depend on the pair's position in the batch, on
(a, b) versus (b, a), on the work split, on the number of workgroups or on timing; two runs are bitwise equal.

    dist = pair_distance(model, pos_edges, test_set=True)
    evaluate.metrics_by_bin(pos_scores, neg_scores, dist, bins=DIST_BINS)      # ranking quality per hop distance
    attention_profile(expl, values=dist, bins=DIST_BINS)                        # attention mass per hop distance
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, graph, ops, sources
from ._lib import check, ptr

# half-open [lo, hi) cells for evaluate.metrics_by_bin / explain.attention_profile:
# unreachable, the same node, 1, 2, 3, 4-5 and 6 or more hops
DIST_BINS = ((-1, 0), (0, 1), (1, 2), (2, 3), (3, 4), (4, 6), (6, float("inf")))
MAX_GROUPS = 2048                     # resident workgroups of the search kernel the default sizing asks for at most
ABI_MAX_GROUPS = 65535                # lpf_pair_bfs: 1 <= n_groups <= 65535
# 8 n + 8 bytes per workgroup.  Chosen from the workgroup sweep of tools/pair_distance_time.py
# (profiles/pair_distance_timing.json: MI355X, collab-like graph n = 235,868, 32,768 held-out positives, unlimited,
# whole-call ms): 64 / 128 / 256 / 512 / 1024 / 2048 workgroups (115 / 230 / 461 / 921 / 1843 / 3685 MB) take
# 6.72 / 3.44 / 1.84 / 1.49 / 1.24 / 1.32 ms, uniform random pairs 7.58 / 3.85 / 2.02 / 1.54 / 1.26 / 1.31 ms.  Time
# halves with the workgroups up to 256, still falls 17 % from 512 to 1024 and rises past that: the memset of 4 n bytes
# of stamps per launched workgroup grows while the search no longer gains.  2048 MB is the smallest power of two that
# holds the fastest measured count on that graph (it gives 1138 workgroups there); 1024 MB (569) costs 17 % more time.
WORKSPACE_MB = 2048


def _check_options(max_dist, groups, workspace_mb):
    if max_dist is not None:
        if isinstance(max_dist, bool) or not isinstance(max_dist, (int, np.integer)) or int(max_dist) < 1:
            raise ValueError(f"max_dist must be None or an integer >= 1; got {max_dist!r}")
        max_dist = min(int(max_dist), (1 << 31) - 1)
    if groups is not None and not 1 <= int(groups) <= ABI_MAX_GROUPS:
        raise ValueError(f"groups must be in [1, {ABI_MAX_GROUPS}]; got {groups!r}")
    if not workspace_mb > 0:
        raise ValueError("workspace_mb must be positive")
    return max_dist


# ------------------------------------------------------------------------------------------------- host restatement
def _neighbours(rowptr, col, nodes):
    """The concatenated rows ``nodes``."""
    return col[sources.csr_rows(rowptr, nodes)[0]].astype(np.int64)


def distance_reference(adj: graph.CSR, edges, *, max_dist=None, ignore_direct: bool = False) -> torch.Tensor:
    """``pair_distance`` of a host CSR in numpy (a CPU int32 tensor out): plain level-by-level frontier sets, one search
    per distinct first endpoint (one per pair where ``ignore_direct`` removes the pair's own edge).  The restatement the
    device kernel is tested against, and what ``pair_distance`` runs when there is no GPU."""
    max_dist = _check_options(max_dist, None, 1)
    batch = sources.as_pairs(edges).cpu().to(torch.int64).numpy()
    a, b = batch[0], batch[1]
    n = int(adj.n)
    rowptr, col = np.asarray(adj.rowptr, np.int64), np.asarray(adj.col)
    out = np.full(a.size, -1, np.int32)
    out[a == b] = 0
    idx = np.flatnonzero((a != b) & (a >= 0) & (a < n) & (b >= 0) & (b < n))
    limit = float("inf") if max_dist is None else max_dist
    depth = np.full(n, -1, np.int32)           # shared by the searches: the visited entries are reset after each

    def search(src, targets, drop):
        depth[src] = 0
        frontier = np.array([src], np.int64)
        seen = [frontier]
        d = 0
        while frontier.size and d < limit and (depth[targets] < 0).any():
            nb = _neighbours(rowptr, col, frontier)
            if d == 0 and drop is not None:
                nb = nb[nb != drop]
            nb = nb[(nb >= 0) & (nb < n)]
            frontier = np.unique(nb[depth[nb] < 0])
            d += 1
            depth[frontier] = d
            seen.append(frontier)
        res = depth[targets].copy()
        depth[np.concatenate(seen)] = -1
        return res

    own = np.zeros(idx.size, bool)             # pairs that get a search of their own: their edge is removed
    if ignore_direct and idx.size:
        keys = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr)) * n + col.astype(np.int64)
        q = a[idx] * n + b[idx]
        at = np.minimum(np.searchsorted(keys, q), max(keys.size - 1, 0))
        own = (keys[at] == q) if keys.size else own
        for i in idx[own]:
            out[i] = search(a[i], b[i:i + 1], b[i])[0]
    rest = idx[~own]
    order = rest[np.argsort(a[rest], kind="stable")]
    cuts = np.flatnonzero(np.diff(a[order])) + 1
    for grp in np.split(order, cuts):
        if grp.size:
            out[grp] = search(a[grp[0]], b[grp], None)
    return torch.from_numpy(out)


# ------------------------------------------------------------------------------------------------------ device path
def default_groups(n: int, pairs: int, workspace_mb=WORKSPACE_MB) -> int:
    """The largest number of search workgroups whose workspace (8 n + 8 bytes each) fits ``workspace_mb``, clamped to
    [1, min(pairs, MAX_GROUPS)]."""
    fit = int(workspace_mb * (1 << 20)) // (8 * max(int(n), 1) + 8)
    return int(max(1, min(fit, int(pairs), MAX_GROUPS)))


@torch.no_grad()
def pair_distance(source, edges, *, test_set: bool = False, max_dist=None, ignore_direct: bool = False,
                  chunk: int = 1 << 20, split_threshold: int = -1, groups=None,
                  workspace_mb=WORKSPACE_MB) -> torch.Tensor:
    """Hop distance of ``edges`` ([P, 2] or [2, P], host or device) on the typing adjacency: int32 [P], by the module
    docstring's contract (0: a == b; -1: no path, an id outside [0, n), or farther than ``max_dist``).

    ``source``: a ``LinkTransformer`` (the typing adjacency of the split ``test_set`` selects, the same resident object
    the selection and ``pair_heuristics`` read), a ``graph.CSR`` or a ``graph.DeviceCSR`` (binary SYMMETRIC pattern:
    values are ignored, a non-symmetric pattern is outside the contract).  ``max_dist``: ``None`` or an int >= 1.
    ``ignore_direct``: leave each pair's own edge out of its search.  ``chunk``: pairs per launch.
    ``split_threshold``: shorter-row length up to which the front kernel settles distance 2 itself (negative:
    ``LPF_BFS_SPLIT_DEFAULT``).  ``groups``: workgroups of the search kernel, each with 8 n + 8 bytes of dense state
    (default: as many as fit ``workspace_mb``, at most min(P, 2048)).  The result depends on none of the last four.

    The result is a device tensor and nothing is read back.  A host ``graph.CSR`` with CPU ``edges`` and no GPU present
    goes through ``distance_reference`` and gives a CPU tensor."""
    max_dist = _check_options(max_dist, groups, workspace_mb)
    chunk = sources.clamp_chunk(chunk)
    batch = sources.as_pairs(edges)
    dev, adj, _, _ = sources.resolve(source, test_set, batch, who="pair_distance", host_ok=True)
    if dev is None:
        return distance_reference(adj, batch, max_dist=max_dist, ignore_direct=ignore_direct)
    batch = batch.to(dev, dtype=torch.int64).contiguous()
    P = batch.shape[1]
    with torch.cuda.device(dev):
        dist = torch.empty(P, dtype=torch.int32, device=dev)
        if P == 0:
            return dist
        hip = _lib.hip()
        m_max = min(P, chunk)
        n_groups = int(groups) if groups is not None else default_groups(adj.n, m_max, workspace_mb)
        nbytes = int(hip.lpf_pair_bfs_workspace_bytes(adj.n, n_groups))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        scratch = torch.empty(m_max + 1, dtype=torch.int32, device=dev)
        st = ops.raw_stream(dev)
        for lo, m in sources.chunks(P, chunk):
            check(hip.lpf_pair_bfs(m, adj.n, batch.data_ptr() + lo * 8, P, ptr(adj.rowptr),
                                   ptr(adj.col), 0 if max_dist is None else max_dist, 1 if ignore_direct else 0,
                                   int(split_threshold), ptr(scratch), ptr(ws), n_groups,
                                   dist.data_ptr() + lo * 4, st), "lpf_pair_bfs")
    return dist
