"""Walk counts and the truncated Katz index of candidate pairs on the typing adjacency.

Katz(a, b) = sum_{l >= 1} beta^l (A^l)[a, b], in practice truncated at walks of length 3: the other global structural
baseline of the HeaRT / OGB comparisons next to the shortest path.  ``pair_heuristics``' CN sees walks of length 2
only; ``pair_distance`` says that a and b are 3 hops apart, not whether one path or a thousand join them.  The reference
has no such code; on the host it is a sparse ``A @ A`` per batch, which fills in on hub graphs.

Contract (shared by the kernel, ``lpf_pair_walks`` in csrc/pair_walks.hip, and the numpy restatement below).  The graph
is a binary CSR with sorted, unique int32 columns and a SYMMETRIC pattern -- the typing adjacency the selection reads;
values are ignored; a non-symmetric pattern is outside the contract.  For pair p = (a, b) and l = 1 .. ``max_len``:

* ``W_l(a, b) = (A^l)[a, b]``: the number of walks of l stored entries from a to b.  Stored self-loops count as the
  entries they are; ``a == b`` is no special case (closed walks: ``W_2(a, a) = deg(a)``); an id outside ``[0, n)``
  gives 0 for every l;
* ``max_len``: an integer in 1 .. 4, default 3 (HeaRT's truncation);
* ``ignore_direct=True``: for THIS pair every transition x -> y with {x, y} = {a, b} is skipped at every step of the
  walk, which is counting on a copy of A without the stored entries (a, b) and (b, a).  A pair that is no edge is
  unaffected; for ``a == b`` the skipped entry is the self-loop, if stored;
* counts are exact int64.  ``W_l <= maxdeg^(l - 1)``: the graph's largest degree is read once per graph object (the only
  host read) and ``maxdeg^(max_len - 1) >= 2^63`` raises ``ValueError`` (``check_range``);
* ``katz_from_walks``: with ``p_l = beta ** l`` as Python floats, ``W_1 * p_1``, then ``+ W_2 * p_2``, ... in fp64, one
  op per multiply and per add in ascending l, rounded once to float32 -- the same IEEE operations on either device.

The result is a pure function of (graph, pair, options): it does not depend on the pair's position in the batch, on
(a, b) versus (b, a), on chunking, on the number of workgroups, on the work split or on timing; two runs are bitwise
equal.

    katz = pair_katz(model, pos_edges, test_set=True)
    evaluate.metrics_by_bin(pos_scores, neg_scores, katz, bins=...)           # ranking quality per Katz cell
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib, distance, graph, ops, sources
from ._lib import check, ptr

MAX_LEN = 4                           # lpf_pair_walks: 1 <= max_len <= 4 (length 5 needs three-hop rows)
# Workgroups and workspace: distance.py's constants, which were measured for the BFS of pair_distance and NOT for this
# kernel (8 n bytes of dense state per workgroup here, 8 n + 8 there).  Not measured for pair_walks: tools/
# pair_katz_time.py sweeps the workgroup count and writes profiles/pair_katz_timing.json.
MAX_GROUPS = distance.MAX_GROUPS
ABI_MAX_GROUPS = 65535                # lpf_pair_walks: 1 <= n_groups <= 65535
WORKSPACE_MB = distance.WORKSPACE_MB
# Pairs of one spread endpoint a workgroup walks after one spread; longer runs are cut, so that a hub's run (a HeaRT
# batch holds one endpoint k / 2 times, a recommend result shares its source) is not the whole launch.  Not measured.
RUN_MAX = 64

_GRAPH: dict = {}                     # per graph object (sources.per_object): max degree, E2 table


# ---------------------------------------------------------------------------------------------------------- options
def check_range(max_deg: int, max_len: int) -> None:
    """``W_l <= max_deg^(l - 1)`` must fit int64 for every l <= ``max_len``: raises ``ValueError`` when
    ``max_deg^(max_len - 1) >= 2^63``."""
    if int(max_deg) ** (int(max_len) - 1) >= 1 << 63:
        raise ValueError(f"walk counts of length {max_len} may not fit int64 on a graph of largest degree {max_deg} "
                         f"({max_deg}^{max_len - 1} >= 2^63); lower max_len")


def _check_max_len(max_len) -> int:
    if isinstance(max_len, bool) or not isinstance(max_len, (int, np.integer)) or not 1 <= int(max_len) <= MAX_LEN:
        raise ValueError(f"max_len must be an integer in [1, {MAX_LEN}]; got {max_len!r}")
    return int(max_len)


def _check_beta(beta) -> float:
    if isinstance(beta, bool) or not isinstance(beta, (int, float, np.integer, np.floating)):
        raise ValueError(f"beta must be a finite float > 0; got {beta!r}")
    beta = float(beta)
    if not (math.isfinite(beta) and beta > 0.0):
        raise ValueError(f"beta must be a finite float > 0; got {beta!r}")
    return beta


def _check_launch(groups, workspace_mb) -> None:
    if groups is not None and not 1 <= int(groups) <= ABI_MAX_GROUPS:
        raise ValueError(f"groups must be in [1, {ABI_MAX_GROUPS}]; got {groups!r}")
    if not workspace_mb > 0:
        raise ValueError("workspace_mb must be positive")


def katz_from_walks(walks: torch.Tensor, beta: float = 0.005) -> torch.Tensor:
    """float32 [P] from walk counts int64 [P, L], on the device ``walks`` lives on: ``W_1 * beta``, then
    ``+ W_2 * beta ** 2``, ... in fp64 (one op per multiply and per add, ascending l), rounded once to float32."""
    beta = _check_beta(beta)
    if walks.dim() != 2 or walks.dtype.is_floating_point or walks.dtype == torch.bool:
        raise ValueError("walks must be an integer tensor [P, L]")
    w = walks.to(torch.float64)
    acc = torch.zeros(walks.shape[0], dtype=torch.float64, device=walks.device)
    for l in range(walks.shape[1]):
        term = w[:, l] * (beta ** (l + 1))
        acc = term if l == 0 else acc + term
    return acc.to(torch.float32)


# ------------------------------------------------------------------------------------------------- host restatement
def walks_reference(adj: graph.CSR, edges, *, max_len=3, ignore_direct: bool = False) -> torch.Tensor:
    """``pair_walks`` of a host CSR in numpy (a CPU int64 tensor [P, max_len] out): per endpoint the plain frontier
    vectors x_1 = A e_u and x_2 = A x_1 (node ids with integer counts), met in the middle --
    W_1 = x_1^a[b], W_2 = x_1^a . x_1^b, W_3 = x_2^a . x_1^b, W_4 = x_2^a . x_2^b -- one pair of vectors per distinct
    endpoint, and per pair, without that pair's own transitions, where ``ignore_direct`` removes a stored edge.  The
    restatement the device kernel is tested against, and what ``pair_walks`` runs when there is no GPU."""
    L = _check_max_len(max_len)
    batch = sources.as_pairs(edges).cpu().to(torch.int64).numpy()
    a, b = batch[0], batch[1]
    n = int(adj.n)
    rowptr, col = np.asarray(adj.rowptr, np.int64), np.asarray(adj.col)
    out = np.zeros((a.size, L), np.int64)
    idx = np.flatnonzero((a >= 0) & (a < n) & (b >= 0) & (b < n))
    if not idx.size:
        return torch.from_numpy(out)
    check_range(int(np.diff(rowptr).max()) if n else 0, L)

    def step(ids, cnt, drop):
        """(ids, cnt) of A x for the vector x = (ids, cnt); ``drop`` = (a, b): without the transitions {a, b}."""
        flat, pos = sources.csr_rows(rowptr, ids)
        dst, src, wt = col[flat].astype(np.int64), ids[pos], cnt[pos]
        keep = (dst >= 0) & (dst < n)
        if drop is not None:
            keep &= ~(((src == drop[0]) & (dst == drop[1])) | ((src == drop[1]) & (dst == drop[0])))
        # (a count of x_2 is at most a degree: the float64 sums of bincount are exact)
        dense = np.bincount(dst[keep], weights=wt[keep].astype(np.float64), minlength=n).astype(np.int64)
        to = np.flatnonzero(dense)
        return to, dense[to]

    def vectors(u, drop, hops):
        x1 = step(np.array([u], np.int64), np.ones(1, np.int64), drop)
        return x1, (step(*x1, drop) if hops == 2 else None)

    def dense(vec):
        d = np.zeros(n, np.int64)
        if vec is not None:
            d[vec[0]] = vec[1]
        return d

    def counts(i, xa1, xa2, yb):
        (y1, y2) = yb
        out[i, 0] = xa1[b[i]]
        if L >= 2:
            out[i, 1] = int(xa1[y1[0]].sum())
        if L >= 3:
            out[i, 2] = int(xa2[y1[0]].sum())
        if L >= 4:
            out[i, 3] = int((xa2[y2[0]] * y2[1]).sum())

    hops_a, hops_b = (2 if L >= 3 else 1), (2 if L >= 4 else 1)
    own = np.zeros(idx.size, bool)             # pairs that get vectors of their own: their edge is removed
    if ignore_direct and col.size:
        keys = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr)) * n + col.astype(np.int64)
        q = a[idx] * n + b[idx]
        own = keys[np.minimum(np.searchsorted(keys, q), keys.size - 1)] == q
        for i in idx[own]:
            drop = (a[i], b[i])
            xa = vectors(a[i], drop, hops_a)
            counts(i, dense(xa[0]), dense(xa[1]), vectors(b[i], drop, hops_b))
    rest = idx[~own]
    order = rest[np.argsort(a[rest], kind="stable")]
    cuts = np.flatnonzero(np.diff(a[order])) + 1
    walked: dict = {}                          # walk-side vectors per distinct b
    for grp in np.split(order, cuts):
        if not grp.size:
            continue
        xa = vectors(a[grp[0]], None, hops_a)
        xa1, xa2 = dense(xa[0]), dense(xa[1])
        for i in grp:
            yb = walked.get(b[i])
            if yb is None:
                yb = walked[b[i]] = vectors(b[i], None, hops_b)
            counts(i, xa1, xa2, yb)
    return torch.from_numpy(out)


# ------------------------------------------------------------------------------------------------------ device path
def default_groups(n: int, pairs: int, workspace_mb=WORKSPACE_MB) -> int:
    """The largest number of workgroups whose workspace (16 bytes, then 8 n each) fits ``workspace_mb``, clamped to
    [1, min(pairs, MAX_GROUPS)]."""
    fit = (int(workspace_mb * (1 << 20)) - 16) // (8 * max(int(n), 1))
    return int(max(1, min(fit, int(pairs), MAX_GROUPS)))


def graph_tables(g: graph.DeviceCSR) -> dict:
    """Per graph object, next to ``heuristics.weight_tables``: ``max_deg`` (a Python int: the one host read),
    ``e2`` int64 [n + 1] with E2(u) = sum of deg(w) over w in N(u) -- the entries a two-hop walk from u reads -- and
    e2[n] = 0 for the stand-in id of a pair with an id outside [0, n)."""
    def make():
        deg = g.rowptr[1:] - g.rowptr[:-1]
        cs = torch.zeros(g.col.numel() + 1, dtype=torch.int64, device=g.col.device)
        torch.cumsum(deg[g.col.long()], 0, out=cs[1:])
        e2 = torch.zeros(g.n + 1, dtype=torch.int64, device=g.col.device)
        e2[:g.n] = cs[g.rowptr[1:]] - cs[g.rowptr[:-1]]
        return {"max_deg": int(deg.max()) if g.n else 0, "e2": e2}
    return sources.per_object(_GRAPH, g, make)


def _units(g: graph.DeviceCSR, a: torch.Tensor, b: torch.Tensor, ignore_direct: bool):
    """Orient, sort and cut one launch's pairs on the device (fixed shapes: nothing is read back): (pairs int64 [2, m]
    -- row 0 the spread endpoint, row 1 the walk endpoint, sorted --, unit_ptr int32 [m + 1], order int64 [m] with
    sorted position j holding the launch's pair order[j]).

    Orientation rule (the counts do not depend on it): spread the endpoint that occurs more often among the launch's
    endpoints, so that its spread is shared by more pairs; on a tie walk from the side with the smaller E2 (spread the
    larger; equal E2: spread the smaller id).  A pair with an id outside [0, n) becomes (n, n), which the kernel
    answers with zeros.  Sorted by (spread endpoint, stored edge under ignore_direct, walk endpoint); a unit is a run
    of one spread endpoint, cut every RUN_MAX pairs; under ignore_direct every pair that is a stored entry is a unit of
    its own (its spread differs: the pair's transitions are skipped), the others keep sharing."""
    n, m, dev = g.n, a.numel(), a.device
    ok = (a >= 0) & (a < n) & (b >= 0) & (b < n)
    a, b = torch.where(ok, a, n), torch.where(ok, b, n)
    occ = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    occ.index_add_(0, torch.cat([a, b]), torch.ones(2 * m, dtype=torch.int64, device=dev))
    e2 = graph_tables(g)["e2"]
    oa, ob, ea, eb = occ[a], occ[b], e2[a], e2[b]
    spread_a = (oa > ob) | ((oa == ob) & ((ea > eb) | ((ea == eb) & (a <= b))))
    s, t = torch.where(spread_a, a, b), torch.where(spread_a, b, a)
    own = torch.zeros(m, dtype=torch.bool, device=dev)
    if ignore_direct and g.col.numel():
        keys = g.structure.edge_keys()      # ascending (the CSR's own order), made once per structure
        q = s * n + t
        own = ok & (keys[torch.searchsorted(keys, q).clamp_(max=keys.numel() - 1)] == q)
    order = torch.argsort((s * 2 + own.long()) * (n + 1) + t)
    s, t, own = s[order], t[order], own[order]
    j = torch.arange(m, dtype=torch.int64, device=dev)
    first = torch.ones(m, dtype=torch.bool, device=dev)
    first[1:] = (s[1:] != s[:-1]) | own[1:] | own[:-1]
    run_start = torch.cummax(torch.where(first, j, torch.zeros_like(j)), 0).values
    start = first | ((j - run_start) % RUN_MAX == 0)
    uid = torch.cumsum(start.long(), 0) - 1
    unit_ptr = torch.full((m + 2,), m, dtype=torch.int32, device=dev)      # [m + 1]: where the non-starts write
    unit_ptr[torch.where(start, uid, torch.full_like(uid, m + 1))] = j.to(torch.int32)
    return torch.stack([s, t]).contiguous(), unit_ptr, order


@torch.no_grad()
def pair_walks(source, edges, *, test_set: bool = False, max_len=3, ignore_direct: bool = False,
               chunk: int = 1 << 20, groups=None, workspace_mb=WORKSPACE_MB) -> torch.Tensor:
    """Walk counts of ``edges`` ([P, 2] or [2, P], host or device) on the typing adjacency: int64 [P, max_len], column
    l - 1 = W_l, by the module docstring's contract.

    ``source``: a ``LinkTransformer`` (the typing adjacency of the split ``test_set`` selects, the same resident object
    the selection, ``pair_heuristics`` and ``pair_distance`` read), a ``graph.CSR`` or a ``graph.DeviceCSR`` (binary
    SYMMETRIC pattern: values are ignored, a non-symmetric pattern is outside the contract).  ``max_len``: 1 .. 4.
    ``ignore_direct``: leave each pair's own edge out of its walks.  ``chunk``: pairs per launch.  ``groups``:
    workgroups, each with 8 n bytes of dense state (default: as many as fit ``workspace_mb``, at most min(P, 2048)).
    The result depends on none of the last three.

    The result is a device tensor; nothing is read back per call (the graph's largest degree is read once per graph
    object, for the int64 range check).  A host ``graph.CSR`` with CPU ``edges`` and no GPU present goes through
    ``walks_reference`` and gives a CPU tensor."""
    L = _check_max_len(max_len)
    _check_launch(groups, workspace_mb)
    chunk = sources.clamp_chunk(chunk)
    batch = sources.as_pairs(edges)
    dev, adj, _, _ = sources.resolve(source, test_set, batch, who="pair_walks", host_ok=True)
    if dev is None:
        return walks_reference(adj, batch, max_len=L, ignore_direct=ignore_direct)
    batch = batch.to(dev, dtype=torch.int64).contiguous()
    P = batch.shape[1]
    with torch.cuda.device(dev):
        if P == 0 or adj.n <= 0:
            return torch.zeros((P, L), dtype=torch.int64, device=dev)
        check_range(graph_tables(adj)["max_deg"], L)
        walks = torch.empty((P, L), dtype=torch.int64, device=dev)
        hip = _lib.hip()
        m_max = min(P, chunk)
        n_groups = int(groups) if groups is not None else default_groups(adj.n, m_max, workspace_mb)
        nbytes = int(hip.lpf_pair_walks_workspace_bytes(adj.n, n_groups))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        st = ops.raw_stream(dev)
        for lo, m in sources.chunks(P, chunk):
            pairs, unit_ptr, order = _units(adj, batch[0, lo:lo + m], batch[1, lo:lo + m], bool(ignore_direct))
            part = torch.empty((m, L), dtype=torch.int64, device=dev)
            check(hip.lpf_pair_walks(m, adj.n, ptr(pairs), m, ptr(adj.rowptr), ptr(adj.col), L,
                                     1 if ignore_direct else 0, ptr(unit_ptr), ptr(ws), n_groups, ptr(part), st),
                  "lpf_pair_walks")
            walks[lo:lo + m].index_copy_(0, order, part)
    return walks


@torch.no_grad()
def pair_katz(source, edges, *, beta: float = 0.005, test_set: bool = False, max_len=3, ignore_direct: bool = False,
              chunk: int = 1 << 20, groups=None, workspace_mb=WORKSPACE_MB) -> torch.Tensor:
    """The truncated Katz index of ``edges``: float32 [P] = ``katz_from_walks(pair_walks(...), beta)``, on the device
    ``pair_walks`` answers on.  ``beta``: a finite float > 0 (default 0.005, HeaRT's); the other arguments are
    ``pair_walks``'."""
    beta = _check_beta(beta)
    return katz_from_walks(pair_walks(source, edges, test_set=test_set, max_len=max_len, ignore_direct=ignore_direct,
                                      chunk=chunk, groups=groups, workspace_mb=workspace_mb), beta)
