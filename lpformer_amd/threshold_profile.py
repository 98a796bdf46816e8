"""What a threshold triple selects: per-pair node counts for a whole grid of PPR thresholds.

``thresh_cn``, ``thresh_1hop`` and ``thresh_non1hop`` decide which nodes enter a pair's attention
(src/models/link_transformer.py:241-250, 478), hence what a model costs and what it sees; the reference tunes them per
dataset by grid search (src/run.py:199-201).  Here one pass over the UNFILTERED typing adjacency and PPR matrix answers
the question for every grid point at once, without building a model per point:

    threshold_profile(source, edges, thresholds)    counts per pair, type and threshold (``ThresholdProfile``)
    profile.entries(th_cn, th_1hop, th_non1hop)     total entries per type of a model with these thresholds
    suggest_thresholds(profile, budget)             the most permissive grid triple within a budget of entries per pair

For pair (a, b) a candidate node v has a type and two round-tripped PPR values (ra, rb):

    type 0  common neighbour: v in N(a) & N(b);                      ra = rt2(P[a, v]), rb = rt2(P[b, v])
    type 1  one-hop: v in exactly one of N(a), N(b);                 ra = rt1(P[a, v]), rb = rt1(P[b, v])
    type 2  >1-hop: v in neither, P[a, v] > 0 and P[b, v] > 0;       ra = rt1(P[a, v]), rb = rt1(P[b, v])

(P reads 0 where nothing is stored; rt1 / rt2 are the reference's fp32 round trips) and
``count[p, t, j] = #{v of type t: ra >= theta_j and rb >= theta_j}`` -- exactly the nodes of type t a model whose
threshold for that type is ``theta_j`` selects for the pair, boundary values included.  There is no special case for v
in {a, b} or a == b.  In mask mode ``"cn"`` type 0 uses rt1 and types 1 and 2 are empty.

Graphs on a GPU go through ``lpf_threshold_profile`` (csrc/thresh_profile.hip); host ``graph.CSR`` containers with CPU
edges and no GPU present through the numpy restatement ``profile_reference`` below, the pattern of
``evaluate.rank_counts`` and ``explain_from_scores``.  Both are integer counts: they agree exactly.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib, graph, ops, sources
from ._lib import check, ptr

MAX_T = _lib.CONST["LPF_THRESH_MAX_T"]
DEFAULT_GRID = (0, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1)
TYPE_NAMES = ("cn", "1-hop", ">1-hop")
_ARGS = ("thresh_cn", "thresh_1hop", "thresh_non1hop")
_HOST_CHUNK = 1 << 15                       # pairs per pass of the host restatement (bounds its temporaries)


class ThresholdProfile(NamedTuple):
    thresholds: torch.Tensor                # float32 [T], ascending
    total: torch.Tensor                     # int64 [3, T]: selected nodes over all pairs, per type and threshold
    max_per_pair: torch.Tensor              # int32 [3, T]: the most any one pair selects
    nonempty: torch.Tensor                  # int64 [3, T]: pairs that select at least one
    per_pair: Optional[torch.Tensor]        # int32 [P, 3, T] or None
    n_pairs: int

    def _index(self, value, name: str) -> int:
        th = self.thresholds.detach().cpu().numpy()
        hit = np.flatnonzero(th == np.float32(value))
        if hit.size != 1:
            raise ValueError(f"{name} = {value!r} is not a threshold of this profile's grid {th.tolist()}")
        return int(hit[0])

    def entries(self, thresh_cn, thresh_1hop, thresh_non1hop):
        """(cn, 1-hop, >1-hop) total entries a model with these thresholds selects over the profiled pairs.  Each value
        must be a threshold of the grid.  The value 1 where the model's constructor reads it as a mode switch
        (``thresh_non1hop == 1``: no >1-hop nodes; with ``thresh_1hop == 1`` too: common neighbours only) is accepted
        without being in the grid and gives 0 for the types it switches off.  (A ``"cn"``-mode model round-trips its
        common neighbours with rt1: profile it with a ``"cn"``-mode source, or ``mode_cn=True``, for exact counts.)"""
        total = self.total.detach().cpu()
        no_far = float(thresh_non1hop) == 1.0
        no_hop = no_far and float(thresh_1hop) == 1.0
        cn = int(total[0, self._index(thresh_cn, "thresh_cn")])
        hop = 0 if no_hop else int(total[1, self._index(thresh_1hop, "thresh_1hop")])
        far = 0 if no_far else int(total[2, self._index(thresh_non1hop, "thresh_non1hop")])
        return cn, hop, far

    def table(self) -> str:
        """Printable summary: per threshold and type the total, the mean per pair, the largest pair and the share of
        the pairs that select anything."""
        th = self.thresholds.detach().cpu().tolist()
        total, mx, ne = (t.detach().cpu().tolist() for t in (self.total, self.max_per_pair, self.nonempty))
        P = max(self.n_pairs, 1)
        lines = [f"{self.n_pairs} pairs", f"{'threshold':>12} " + " ".join(f"| {n + ': total':>16} {'mean':>9} {'max':>7} {'pairs':>6}"
                                                                            for n in TYPE_NAMES)]
        for j, t in enumerate(th):
            cells = [f"| {total[k][j]:>16d} {total[k][j] / P:>9.3f} {mx[k][j]:>7d} {100.0 * ne[k][j] / P:>5.1f}%"
                     for k in range(3)]
            lines.append(f"{t:>12.6g} " + " ".join(cells))
        return "\n".join(lines)


def suggest_thresholds(profile: ThresholdProfile, max_entries_per_pair: float, *, fixed: Optional[dict] = None) -> dict:
    """The smallest grid thresholds whose mean entries per pair, ``sum over types of total / n_pairs``, stay within
    ``max_entries_per_pair``.  The rule, plain host arithmetic over ``profile.total``:

    1. every type not named in ``fixed`` starts at the LARGEST threshold of the grid (its fewest entries);
    2. ``thresh_non1hop`` is relaxed first -- lowered one grid step at a time for as long as the mean stays within the
       budget --, then ``thresh_1hop``, then ``thresh_cn``: >1-hop nodes are what the other two types cannot see, and
       common neighbours are kept by every sensible setting, so they get what is left.

    ``fixed``: ``{"thresh_cn" | "thresh_1hop" | "thresh_non1hop": value}`` held where they are (grid values, or the mode
    switches ``entries`` accepts).  Returns the three thresholds, ``entries_per_pair`` (the mean they give) and
    ``within_budget`` (False when even the starting point exceeds the budget)."""
    fixed = dict(fixed or {})
    bad = [k for k in fixed if k not in _ARGS]
    if bad:
        raise ValueError(f"fixed may name {_ARGS}; got {bad}")
    if not max_entries_per_pair >= 0:
        raise ValueError("max_entries_per_pair must be >= 0")
    th = profile.thresholds.detach().cpu().tolist()
    P = max(int(profile.n_pairs), 1)
    top = th[-1]
    cur = {k: fixed.get(k, top) for k in _ARGS}

    def mean(c):
        return sum(profile.entries(c["thresh_cn"], c["thresh_1hop"], c["thresh_non1hop"])) / P

    for name in ("thresh_non1hop", "thresh_1hop", "thresh_cn"):
        if name in fixed:
            continue
        for t in reversed(th[:-1]):
            trial = dict(cur, **{name: t})
            if mean(trial) > max_entries_per_pair:
                break
            cur = trial
    m = mean(cur)
    return dict(cur, entries_per_pair=m, within_budget=bool(m <= max_entries_per_pair))


# ------------------------------------------------------------------------------------------------------- arguments
def check_thresholds(thresholds) -> np.ndarray:
    """The grid as ascending float32 [T]: 1 <= T <= 32, finite, >= 0, no duplicates (after the cast to float32)."""
    th = np.asarray(list(thresholds) if not isinstance(thresholds, (np.ndarray, torch.Tensor)) else thresholds,
                    dtype=np.float64).reshape(-1)
    if not 1 <= th.size <= MAX_T:
        raise ValueError(f"between 1 and {MAX_T} thresholds, got {th.size}")
    if not np.isfinite(th).all() or (th < 0).any():
        raise ValueError("thresholds must be finite and >= 0")
    with np.errstate(over="ignore"):
        th = np.sort(th.astype(np.float32))
    if not np.isfinite(th).all():
        raise ValueError("thresholds must be finite in float32")
    if (th[1:] == th[:-1]).any():
        raise ValueError(f"duplicate thresholds (as float32): {th.tolist()}")
    return th


# ------------------------------------------------------------------------------------------------- host restatement
def _rt1(x: np.ndarray) -> np.ndarray:
    one = np.float32(1)
    return (x + one) - one


def _rt2(x: np.ndarray) -> np.ndarray:
    two = np.float32(2)
    return ((x * two + two) - two) * np.float32(0.5)


def _row_keys(rowptr, col, nodes, n):
    """Keys position * n + column of the rows ``nodes`` (one row per position; ascending and unique), and the flat
    indexes of those entries."""
    flat, pos = sources.csr_rows(rowptr, nodes)
    return pos * np.int64(n) + col[flat].astype(np.int64), flat


def _lookup(keys, vals, query):
    out = np.zeros(query.size, np.float32)
    if keys.size and query.size:
        i = np.minimum(np.searchsorted(keys, query), keys.size - 1)
        hit = keys[i] == query
        out[hit] = vals[i[hit]]
    return out


def _host_counts(a, b, adj: graph.CSR, ppr: graph.CSR, th: np.ndarray, mode_cn: bool) -> np.ndarray:
    """count int32 [P, 3, T] of the pairs (a[p], b[p]): the module docstring's definition in numpy."""
    n, T, P = int(adj.n), th.size, a.size
    hist = np.zeros((P, 3, T + 1), np.int64)          # [p, t, k]: candidates that pass exactly k thresholds
    idx = np.flatnonzero((a >= 0) & (a < n) & (b >= 0) & (b < n))   # a pair with an id outside [0, n) counts nothing
    a, b = a[idx], b[idx]
    ka, _ = _row_keys(adj.rowptr, adj.col, a, n)
    kb, _ = _row_keys(adj.rowptr, adj.col, b, n)
    qa, fa = _row_keys(ppr.rowptr, ppr.col, a, n)
    qb, fb = _row_keys(ppr.rowptr, ppr.col, b, n)
    va, vb = ppr.val[fa].astype(np.float32), ppr.val[fb].astype(np.float32)

    def add(t, keys, ra, rb):
        k = ((ra[:, None] >= th[None, :]) & (rb[:, None] >= th[None, :])).sum(axis=1)
        np.add.at(hist, (idx[keys // n], t, k), 1)

    cn = np.intersect1d(ka, kb, assume_unique=True)
    rt = _rt1 if mode_cn else _rt2
    add(0, cn, rt(_lookup(qa, va, cn)), rt(_lookup(qb, vb, cn)))
    if not mode_cn:
        hop = np.setxor1d(ka, kb, assume_unique=True)
        add(1, hop, _rt1(_lookup(qa, va, hop)), _rt1(_lookup(qb, vb, hop)))
        both, ia, ib = np.intersect1d(qa, qb, assume_unique=True, return_indices=True)
        wa, wb = va[ia], vb[ib]
        far = ~np.isin(both, np.union1d(ka, kb)) & (wa > 0) & (wb > 0)
        add(2, both[far], _rt1(wa[far]), _rt1(wb[far]))
    # count[p, t, j] = candidates that pass more than j thresholds (ascending thresholds: they pass theta_0 .. theta_j)
    return hist[:, :, ::-1].cumsum(axis=2)[:, :, ::-1][:, :, 1:].astype(np.int32)


def profile_reference(adj: graph.CSR, ppr: graph.CSR, edges, thresholds=DEFAULT_GRID, *, mode_cn: bool = False,
                      per_pair: bool = False) -> ThresholdProfile:
    """``threshold_profile`` of host CSR containers in numpy (CPU tensors out): the restatement the device kernel is
    tested against, and what ``threshold_profile`` runs when there is no GPU."""
    th = check_thresholds(thresholds)
    batch = sources.as_pairs(edges).cpu().to(torch.int64).numpy()
    if ppr.val is None:
        raise ValueError("the PPR matrix needs values")
    if int(adj.n) != int(ppr.n):
        raise ValueError("the adjacency and the PPR matrix must describe the same nodes")
    P, T = batch.shape[1], th.size
    total = np.zeros((3, T), np.int64)
    mx = np.zeros((3, T), np.int32)
    ne = np.zeros((3, T), np.int64)
    parts = []
    for lo in range(0, P, _HOST_CHUNK):
        c = _host_counts(batch[0, lo:lo + _HOST_CHUNK], batch[1, lo:lo + _HOST_CHUNK], adj, ppr, th, bool(mode_cn))
        total += c.sum(axis=0, dtype=np.int64)
        mx = np.maximum(mx, c.max(axis=0))
        ne += (c > 0).sum(axis=0)
        if per_pair:
            parts.append(c)
    pp = None
    if per_pair:
        pp = torch.from_numpy(np.concatenate(parts) if parts else np.zeros((0, 3, T), np.int32))
    return ThresholdProfile(torch.from_numpy(th), torch.from_numpy(total), torch.from_numpy(mx), torch.from_numpy(ne),
                            pp, int(P))


# ------------------------------------------------------------------------------------------------------ device path
@torch.no_grad()
def threshold_profile(source, edges, thresholds=DEFAULT_GRID, *, test_set: bool = False, per_pair: bool = False,
                      chunk: int = 1 << 20, split_threshold: int = -1, mode_cn: Optional[bool] = None) -> ThresholdProfile:
    """Selected-node counts of ``edges`` ([P, 2] or [2, P], host or device) per type and threshold (module docstring).

    ``source``: a ``LinkTransformer`` -- its typing adjacency, the raw PPR matrix of the split ``test_set`` selects (the
    objects ``pair_heuristics`` resolves) and its mask mode; the model's own thresholds play no part -- or a pair
    ``(adj, ppr)`` of ``graph.CSR`` / ``graph.DeviceCSR`` with ``mode_cn`` (default False).  ``thresholds``: 1 to 32
    values, cast to float32, sorted; finite, >= 0, no duplicates.  ``per_pair``: also return the counts int32 [P, 3, T].
    ``chunk``: pairs per launch.  ``split_threshold``: walked length above which a pair gets a whole workgroup
    (negative: ``LPF_THRESH_SPLIT_DEFAULT``); the result does not depend on it.

    The profile describes the RESIDENT graphs: adjacency overrides (``adj_mask=``, ``RemovedEdges``) are not applied.
    Results are device tensors and nothing is read back to the host during the sweep; host ``graph.CSR`` containers
    with CPU edges and no GPU present go through ``profile_reference`` and give CPU tensors."""
    th = check_thresholds(thresholds)
    chunk = sources.clamp_chunk(chunk)
    batch = sources.as_pairs(edges)
    dev, adj, ppr, _ = sources.resolve(source, test_set, batch, who="threshold_profile", pieces=True, host_ok=True)
    if ppr is None:
        raise TypeError("source must be a LinkTransformer or a pair (adj, ppr) of graph.CSR / graph.DeviceCSR")
    cn_mode = getattr(source, "mask", None) == "cn" if mode_cn is None else bool(mode_cn)
    if dev is None:
        return profile_reference(adj, ppr, batch, th, mode_cn=cn_mode, per_pair=per_pair)
    batch = batch.to(dev, dtype=torch.int64).contiguous()
    P, T = batch.shape[1], int(th.size)
    th_host = (C.c_float * T)(*th.tolist())
    with torch.cuda.device(dev):
        total = torch.zeros(3, T, dtype=torch.int64, device=dev)
        mx = torch.zeros(3, T, dtype=torch.int32, device=dev)
        ne = torch.zeros(3, T, dtype=torch.int64, device=dev)
        pp = torch.empty(P, 3, T, dtype=torch.int32, device=dev) if per_pair else None
        if P:
            st = ops.raw_stream(dev)
            scratch = torch.empty(min(P, chunk) + 1, dtype=torch.int32, device=dev)
            for lo, m in sources.chunks(P, chunk):
                check(_lib.hip().lpf_threshold_profile(
                    m, adj.n, batch.data_ptr() + lo * 8, P, ptr(adj.rowptr), ptr(adj.col), ptr(ppr.rowptr),
                    ptr(ppr.col), ptr(ppr.val), T, C.cast(th_host, C.c_void_p), 1 if cn_mode else 0,
                    int(split_threshold), ptr(scratch), None if pp is None else pp.data_ptr() + lo * 3 * T * 4,
                    ptr(total), ptr(mx), ptr(ne), st), "lpf_threshold_profile")
        return ThresholdProfile(torch.from_numpy(th).to(dev), total, mx, ne, pp, int(P))
