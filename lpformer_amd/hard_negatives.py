"""HeaRT-style hard negatives made on the device: K negatives of its own for every positive edge.

The reference's ``scripts/replicate_heart.sh`` ranks each positive against ``heart_{valid,test}_samples.npy``
([P, K, 2], src/util/read_datasets.py:132-146, scored by ``test_heart_negatives``, src/train/testing.py:96-121): files
that exist for seven public datasets only.  ``heart_negatives`` makes negatives of that layout for any graph
(definition: DESIGN.md section 5.10), so the protocol also runs on synthetic graphs and on a user's own data:

1. pool of an endpoint u: { c : CN(u, c) > 0 } united with the stored entries of u's PPR row, minus N(u), minus u
   (``lpf_twohop_count`` / ``lpf_twohop_fill``: one row of A diag(w) A; ``lpf_pool_extra_count`` / ``lpf_pool_fill``);
2. every requested heuristic values the pool members (cn / aa / ra from the two-hop row, ppr from the PPR row, feat =
   feature cosine through ``heuristics.feature_cosine``);
3. per heuristic the top k/2 by value, ties to the smaller id (``lpf_segment_topk_f32``), cut at the first value
   that is not > 0;
4. ``lpf_rank_interleave``: the first k/2 distinct nodes in rank-interleaved order, then hash-drawn padding;
5. ``negatives[p, :k/2] = (a, list(a))``, ``negatives[p, k/2:] = (list(b), b)``; where a positive is not an edge of
   the adjacency (held-out positives: the usual case) and b is in list(a), b is dropped and the list's spare entry
   (rank k/2 + 1) moves in, so no negative is the positive itself; likewise for a in list(b).

A node's list is a pure function of (graph, heuristics, k, seed, node): the same in any batch, chunking or split.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib, graph, heuristics
from ._lib import check, ptr
from .recommend import plan_chunks, segment_topk
from .ops import raw_stream
from .sources import as_pairs, node_ids, resolve

HEURISTICS = ("cn", "aa", "ra", "ppr", "feat")
TWOHOP_KINDS = ("cn", "aa", "ra")
MAX_K = min(_lib.CONST["LPF_TOPK_MAX_K"], _lib.CONST["LPF_INTERLEAVE_MAX_KH"])   # k / 2 + 1 must fit both
SPLIT_DEFAULT = _lib.CONST["LPF_TWOHOP_SPLIT_DEFAULT"]
WORKSPACE_BUDGET = 1 << 30            # bytes of dense two-hop state (24 bytes per node and resident workgroup)
MAX_GROUPS = 512


class HardNegatives(NamedTuple):
    negatives: torch.Tensor    # int64 [P, k, 2]: [:, :k/2] = (a, c), [:, k/2:] = (c, b)
    n_ranked: torch.Tensor     # int32 [P, 2]: how many of each half came from the heuristics (the rest is padding)
    nodes: torch.Tensor        # int64 [U]: the distinct endpoints, ascending
    lists: torch.Tensor        # int64 [U, k/2]: the negatives of each endpoint
    list_ranked: torch.Tensor  # int32 [U]
    spare: torch.Tensor        # int64 [U]: entry k/2 + 1 of each list, taken when a positive's other endpoint is listed


def _workspace(n: int, dev):
    groups = int(max(1, min(MAX_GROUPS, WORKSPACE_BUDGET // (24 * max(n, 1)))))
    nbytes = int(_lib.hip().lpf_twohop_workspace_bytes(n, groups))
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev), groups


class TwoHop:
    """The count pass of ``nodes`` (device int64 [S]) and ``fill(lo, hi)`` for ranges of whole sources."""

    def __init__(self, adj: graph.DeviceCSR, nodes: torch.Tensor, kinds, flags: int, split_threshold: int):
        self.adj, self.nodes, self.kinds, self.flags, self.thr = adj, nodes, kinds, int(flags), int(split_threshold)
        dev = nodes.device
        S = nodes.numel()
        self.scratch = torch.empty(S + 1, dtype=torch.int32, device=dev)
        self.ws, self.groups = _workspace(adj.n, dev)
        self.counts = torch.zeros(S, dtype=torch.int64, device=dev)
        if S:
            check(_lib.hip().lpf_twohop_count(S, adj.n, ptr(nodes), ptr(adj.rowptr), ptr(adj.col), self.thr, self.flags,
                                              ptr(self.scratch), ptr(self.ws), self.groups, ptr(self.counts),
                                              raw_stream(dev)), "lpf_twohop_count")

    def fill(self, lo: int, hi: int, total: int):
        """(seg_ptr int64 [hi - lo + 1], col int32 [total], cn int32, aa, ra float32 -- None where not asked for)."""
        adj, dev = self.adj, self.nodes.device
        seg = torch.zeros(hi - lo + 1, dtype=torch.int64, device=dev)
        torch.cumsum(self.counts[lo:hi], 0, out=seg[1:])
        col = torch.empty(total, dtype=torch.int32, device=dev)
        cn = torch.empty(total, dtype=torch.int32, device=dev) if "cn" in self.kinds else None
        aa = torch.empty(total, dtype=torch.float32, device=dev) if "aa" in self.kinds else None
        ra = torch.empty(total, dtype=torch.float32, device=dev) if "ra" in self.kinds else None
        if total and hi > lo:
            w_aa, w_ra = heuristics.weight_tables(adj) if (aa is not None or ra is not None) else (None, None)
            check(_lib.hip().lpf_twohop_fill(hi - lo, adj.n, self.nodes.data_ptr() + lo * 8, ptr(adj.rowptr),
                                             ptr(adj.col), ptr(w_aa), ptr(w_ra), self.thr, self.flags,
                                             ptr(self.scratch), ptr(self.ws), self.groups, ptr(seg), total, ptr(col),
                                             ptr(cn), ptr(aa), ptr(ra), raw_stream(dev)), "lpf_twohop_fill")
        return seg, col, cn, aa, ra


@torch.no_grad()
def twohop_rows(source, nodes, kinds=("cn", "ra"), *, test_set: bool = False, exclude: bool = False,
                split_threshold: int = -1):
    """Rows ``nodes`` (int [S], host or device; duplicates are independent rows) of ``A diag(w) A`` on the typing
    adjacency: ``(seg_ptr int64 [S + 1], col int64 [T], values...)`` with one value tensor [T] per entry of ``kinds``
    (``"cn"`` int32, ``"aa"`` / ``"ra"`` float32), row s at ``seg_ptr[s]:seg_ptr[s + 1]``, ascending ``col``.  The row
    of u holds every c with CN(u, c) > 0 -- u itself and members of N(u) included, unless ``exclude``.  ``aa`` / ``ra``
    are fp64 sums over the common neighbours in ascending id, rounded to fp32 once (bitwise reproducible).

    ``source`` as for ``pair_heuristics``.  ``split_threshold``: expansion (sum of deg(w) over w in N(u)) above which a
    row is built by a whole workgroup with dense state instead of one wavefront with an LDS hash (negative, or above
    ``SPLIT_DEFAULT``: the library default, which is also the capacity of the hash).  The row lengths are read back
    once to size the outputs."""
    if isinstance(kinds, str):
        kinds = (kinds,)
    kinds = tuple(kinds)
    if [k for k in kinds if k not in TWOHOP_KINDS] or len(set(kinds)) != len(kinds):
        raise ValueError(f"kinds must be distinct members of {TWOHOP_KINDS}; got {kinds!r}")
    src = node_ids(nodes, "nodes")
    if src.dim() != 1:
        raise ValueError("nodes must be a 1-D tensor [S]")
    dev, adj, _, _ = resolve(source, test_set, src, who="twohop_rows", pieces=True)
    with torch.cuda.device(dev):
        src = src.to(dev, torch.int64).contiguous()
        th = TwoHop(adj, src, kinds, 3 if exclude else 0, split_threshold)
        total = int(th.counts.sum()) if src.numel() else 0
        seg, col, cn, aa, ra = th.fill(0, src.numel(), total)
    vals = {"cn": cn, "aa": aa, "ra": ra}
    return (seg, col.to(torch.int64)) + tuple(vals[k] for k in kinds)


def _check_args(pos_edges, k, heur, seed, max_pairs):
    """Argument checks that need no device.  Returns (edges [2, P], heuristics tuple, seed as uint64)."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 2 <= int(k) <= MAX_K or int(k) % 2:
        raise ValueError(f"k must be an even integer in [2, {MAX_K}]; got {k!r}")
    if isinstance(heur, str):
        heur = (heur,)
    heur = tuple(heur)
    if not heur or [h for h in heur if h not in HEURISTICS] or len(set(heur)) != len(heur):
        raise ValueError(f"heuristics must be a non-empty ordered subset of {HEURISTICS}; got {heur!r}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise TypeError("seed must be an integer")
    if int(max_pairs) < 1:
        raise ValueError("max_pairs must be positive")
    edges = as_pairs(pos_edges, what="pos_edges", exc=TypeError)
    return edges, heur, int(seed) & 0xFFFFFFFFFFFFFFFF


def node_lists(adj: graph.DeviceCSR, ppr: Optional[graph.DeviceCSR], xd: Optional[torch.Tensor], nodes: torch.Tensor,
               kh: int, heur, seed: int, max_pairs: int = 1 << 24, split_threshold: int = -1, timings=None):
    """(lists int64 [U, kh], list_ranked int32 [U]) of device ``nodes`` (int64 [U], each inside [0, n) with at least
    ``kh`` non-neighbours).  ``timings``: a dict that collects (phase, start event, end event) when given."""
    dev = nodes.device
    hip = _lib.hip()
    n, U, H = adj.n, nodes.numel(), len(heur)
    lists = torch.empty((U, kh), dtype=torch.int64, device=dev)
    ranked = torch.zeros(U, dtype=torch.int32, device=dev)
    if U == 0:
        return lists, ranked

    def phase(name):
        return _Phase(timings, name, dev)

    want = tuple(h for h in TWOHOP_KINDS if h in heur)
    with phase("two-hop rows"):
        th = TwoHop(adj, nodes, want, 3, split_threshold)
    b = ppr if ppr is not None else graph.DeviceCSR(torch.zeros(n + 1, dtype=torch.int64, device=dev),
                                                    torch.zeros(0, dtype=torch.int32, device=dev),
                                                    torch.zeros(0, dtype=torch.float32, device=dev), n)
    # the one sizing read-back: the two-hop row lengths, plus the PPR row lengths as a bound on the pool sizes
    a_cnt = th.counts.cpu().numpy()
    bound = a_cnt + (b.rowptr[nodes + 1] - b.rowptr[nodes]).cpu().numpy()
    a_start = np.concatenate([[0], np.cumsum(a_cnt)])
    for lo, hi in plan_chunks(bound, int(max_pairs)):
        m = hi - lo
        TA = int(a_start[hi] - a_start[lo])
        nodes_c = nodes[lo:hi]
        with phase("two-hop rows"):
            a_ptr, a_col, a_cn, a_aa, a_ra = th.fill(lo, hi, TA)
        with phase("pool"):
            x_cnt = torch.zeros(m, dtype=torch.int64, device=dev)
            check(hip.lpf_pool_extra_count(m, n, ptr(nodes_c), ptr(a_ptr), ptr(a_col), ptr(b.rowptr), ptr(b.col),
                                           ptr(adj.rowptr), ptr(adj.col), ptr(x_cnt), raw_stream(dev)),
                  "lpf_pool_extra_count")
            x_ptr = torch.zeros(m + 1, dtype=torch.int64, device=dev)
            torch.cumsum(x_cnt, 0, out=x_ptr[1:])
            X = int(x_ptr[-1])                    # (sizes the chunk's pool)
            T = TA + X
            x_col = torch.empty(X, dtype=torch.int32, device=dev)
            x_val = torch.empty(X, dtype=torch.float32, device=dev)
            pairs = torch.empty((2, T), dtype=torch.int64, device=dev)
            vals = {h: torch.empty(T, dtype=torch.float32, device=dev) for h in heur if h != "feat"}
            if T:
                check(hip.lpf_pool_fill(m, n, ptr(nodes_c), ptr(a_ptr), ptr(a_col), ptr(a_cn), ptr(a_aa), ptr(a_ra),
                                        ptr(b.rowptr), ptr(b.col), ptr(b.val), ptr(adj.rowptr), ptr(adj.col),
                                        ptr(x_ptr), ptr(x_col), ptr(x_val), X, T, ptr(pairs), ptr(vals.get("cn")),
                                        ptr(vals.get("aa")), ptr(vals.get("ra")), ptr(vals.get("ppr")), raw_stream(dev)),
                      "lpf_pool_fill")
            pool_ptr = a_ptr + x_ptr
        if "feat" in heur:
            with phase("values (feat)"):
                vals["feat"] = heuristics.feature_cosine(xd, pairs)
        ids = torch.empty((H, m, kh), dtype=torch.int64, device=dev)
        top = torch.empty((H, m, kh), dtype=torch.float32, device=dev)
        cnt = torch.empty((H, m), dtype=torch.int64, device=dev)
        with phase("top-K x H"):
            for i, h in enumerate(heur):
                ids[i], top[i], cnt[i] = segment_topk(pool_ptr, vals[h], pairs[1], kh)
        with phase("interleave"):
            check(hip.lpf_rank_interleave(m, n, ptr(nodes_c), H, kh, ptr(ids), ptr(top), ptr(cnt), ptr(adj.rowptr),
                                          ptr(adj.col), seed, lists.data_ptr() + lo * kh * 8,
                                          ranked.data_ptr() + lo * 4, raw_stream(dev)), "lpf_rank_interleave")
    return lists, ranked


class _Phase:
    def __init__(self, timings, name, dev):
        self.t, self.name, self.dev = timings, name, dev

    def __enter__(self):
        if self.t is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record(torch.cuda.current_stream(self.dev))

    def __exit__(self, *exc):
        if self.t is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record(torch.cuda.current_stream(self.dev))
            self.t.setdefault(self.name, []).append((self.e0, e1))
        return False


@torch.no_grad()
def heart_negatives(source, pos_edges, k: int = 500, *, test_set: bool = False, heuristics=("ra", "ppr", "feat"),
                    seed: int = 0, max_pairs: int = 1 << 24, split_threshold: int = -1,
                    timings=None) -> HardNegatives:
    """``k`` hard negatives for every positive edge of ``pos_edges`` ([P, 2] or [2, P], host or device), HeaRT style:
    ``negatives[p, :k/2] = (a, c)`` corrupt the target, ``negatives[p, k/2:] = (c, b)`` the source, as
    ``evaluate.score_negatives`` takes them.

    ``source``: a ``LinkTransformer`` (typing adjacency, PPR matrix and ``data["x"]`` of the split ``test_set`` selects),
    a ``graph.CSR`` / ``graph.DeviceCSR`` adjacency, or the explicit pieces ``(adjacency, PPR or None, x or None)``.
    ``heuristics``: an ordered, non-empty subset of ``("cn", "aa", "ra", "ppr", "feat")``.  The c of a node u are the
    first k/2 distinct nodes when the heuristics' rankings of u's pool (two-hop neighbours and PPR row, minus N(u) and
    u) are walked rank by rank, heuristic by heuristic in the given order; only values > 0 rank.  What is missing is
    padded with nodes drawn from a hash of (``seed``, u, draw index), never u, a neighbour or a repeat.  Lists are per
    node (``nodes`` / ``lists`` / ``list_ranked`` / ``spare``) and do not depend on the batch; a positive whose other
    endpoint is in the list (possible when the positive is not an edge of the adjacency) skips it and takes ``spare``.  Nodes are processed in chunks of
    whole nodes whose pools stay within ``max_pairs`` entries; the pool sizes are read back to plan them."""
    from . import heuristics as _h
    edges, heur, seed = _check_args(pos_edges, k, heuristics, seed, max_pairs)
    kh = int(k) // 2

    def need(ppr, x):
        if "feat" in heur and x is None:
            raise ValueError("'feat' needs node features: this source has no x (a graph without features, such as "
                             "ogbl-ddi); leave 'feat' out of heuristics")
        if "ppr" in heur and ppr is None:
            raise ValueError("'ppr' needs a PPR matrix: pass a LinkTransformer or (adjacency, PPR, x)")
    if isinstance(source, (tuple, list)) and len(source) == 3:
        need(source[1], source[2])              # (before anything touches the device)
    elif isinstance(source, (graph.CSR, graph.DeviceCSR)):
        need(None, None)
    dev, adj, ppr, x = resolve(source, test_set, edges, who="heart_negatives", pieces=True)
    need(ppr, x)
    n = adj.n
    if edges.numel() and (int(edges.min()) < 0 or int(edges.max()) >= n):
        raise IndexError(f"heart_negatives: pos_edges holds node ids outside [0, {n})")
    with torch.cuda.device(dev):
        e = edges.to(dev, torch.int64).contiguous()
        P = e.shape[1]
        nodes, inv = torch.unique(e.reshape(-1), return_inverse=True)
        if nodes.numel():
            room = n - 1 - (adj.rowptr[nodes + 1] - adj.rowptr[nodes])
            if int(room.min()) < kh:
                u = int(nodes[int(room.argmin())])
                raise ValueError(f"node {u} has only {int(room.min())} non-neighbours; k / 2 = {kh} negatives need "
                                 "that many")
        xd = _h.device_features(x, dev) if "feat" in heur else None
        # one spare entry per node: a positive (a, b) that is not an edge of the adjacency may find b in list(a)
        full, ranked1 = node_lists(adj, ppr, xd, nodes, kh + 1, heur, seed, max_pairs, split_threshold, timings)
        inv = inv.reshape(2, P)

        def half(own, other):
            """The first kh entries of the own endpoint's list that are not the other endpoint, and how many of them
            a heuristic ranked."""
            rows, r1 = full[own], ranked1[own]
            hit = rows == other.unsqueeze(1)
            has = hit.any(dim=1)
            drop = torch.where(has, hit.to(torch.int8).argmax(dim=1), torch.full_like(other, kh))
            at = torch.arange(kh, device=dev).unsqueeze(0)
            picked = torch.gather(rows, 1, at + (at >= drop.unsqueeze(1)).to(torch.int64))
            nr = torch.clamp(r1 - (has & (drop < r1)).to(torch.int32), max=kh)
            return picked, nr
        la, ra_ = half(inv[0], e[1])
        lb, rb_ = half(inv[1], e[0])
        if P and int(room.min()) == kh and (bool((la < 0).any()) or bool((lb < 0).any())):
            raise ValueError(f"a positive's endpoint has only {kh} non-neighbours and the other endpoint is one of "
                             f"them: k / 2 = {kh} negatives need one more")
        neg = torch.empty((P, 2 * kh, 2), dtype=torch.int64, device=dev)
        neg[:, :kh, 0] = e[0].unsqueeze(1)
        neg[:, :kh, 1] = la
        neg[:, kh:, 0] = lb
        neg[:, kh:, 1] = e[1].unsqueeze(1)
        n_ranked = torch.stack([ra_, rb_], dim=1)
    return HardNegatives(neg, n_ranked, nodes, full[:, :kh].contiguous(), torch.clamp(ranked1, max=kh), full[:, kh])
