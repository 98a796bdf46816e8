"""Nearest nodes by embedding similarity: for each query the ``m`` nodes whose rows of a table -- the encoder's output,
the raw features or any float tensor -- have the largest inner product or cosine with it.

``recommend`` proposes a source's candidates from its PPR row, its two-hop row or every node, and
``heuristics.feature_cosine`` values the pairs it is handed; neither answers "which nodes are most similar to u?".  This
is the retrieval stage: one HIP entry point (``lpf_similar_topm_f32``, csrc/similar.hip) multiplies the queries with the
table on the fp32 matrix cores and keeps the top ``m`` per query in LDS, so no [S, n] score matrix exists; the exclusion
row (by default the model's typing adjacency) and the query's own node are dropped inside the kernel; the ranking key is
the one of ``lpf_segment_topk_f32`` with the node id in place of the position: score descending, ties to the smaller
id, -0.0 == +0.0, NaN below -inf.  The result is a pure function of the inputs.

``similar_reference`` restates it in numpy (dot products in fp64, rounded to fp32 once): the kernel's equal bit for bit
wherever the dot products are exactly representable, its fp64-side reference otherwise.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import NamedTuple

import numpy as np
import torch

from . import _lib, graph, ops
from ._lib import check, ptr
from .sources import model_graphs, node_ids

MAX_M = _lib.CONST["LPF_SIMILAR_MAX_M"]
METRICS = ("dot", "cosine")
TABLES = ("embedding", "x")


class Similar(NamedTuple):
    ids: torch.Tensor       # int64 [S, m]: node ids, most similar first; -1 past counts
    scores: torch.Tensor    # float32 [S, m]: their scores; -inf past counts
    counts: torch.Tensor    # int64 [S]: min(m, eligible nodes)


# ------------------------------------------------------------------------------------------------- numpy restatement
def order_key(score) -> np.ndarray:
    """The ranking key of float32 scores as uint32: ascending float order, -0.0 -> +0.0, every NaN below -inf."""
    s = np.asarray(score, np.float32)
    b = s.view(np.uint32).copy()
    b[b == 0x80000000] = 0
    key = np.where(b & 0x80000000, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    key[np.isnan(s)] = 0
    return key


def _host_rows(exclude):
    """(rowptr, col) numpy arrays of an exclusion graph: None, a graph.CSR / graph.DeviceCSR or a (rowptr, col) pair."""
    if exclude is None:
        return None
    if isinstance(exclude, graph.DeviceCSR):
        exclude = exclude.to_host()
    if isinstance(exclude, graph.CSR):
        return np.asarray(exclude.rowptr, np.int64), np.asarray(exclude.col, np.int64)
    rowptr, col = exclude
    return np.asarray(rowptr, np.int64), np.asarray(col, np.int64)


def similar_reference(Q, T, m: int, *, q_scale=None, t_scale=None, src_ids=None, exclude=None,
                      exclude_self: bool = True):
    """``lpf_similar_topm_f32`` in numpy: (ids int64 [S, m], scores float32 [S, m], counts int64 [S]).

    score(s, v) = fl32(sum_k Q[s][k] T[v][k]) with the sum taken in fp64, then -- with ``q_scale`` [S] and ``t_scale``
    [n] -- (score * q_scale[s]) * t_scale[v] as two fp32 multiplies.  Eligible: every v, except (only with ``src_ids``)
    the exclusion row of src_ids[s] (``exclude``: a graph.CSR, a graph.DeviceCSR or (rowptr, col)) and, with
    ``exclude_self``, src_ids[s]; a src_ids[s] outside [0, n) has no eligible node.  Ranked by (``order_key`` of the
    score) << 32 | ~v, descending; padding -1 / -inf.  A returned -0.0 reads +0.0 and a NaN the canonical quiet NaN,
    as from the kernel (the scores are decoded from the keys)."""
    Q = np.asarray(Q, np.float32)
    T = np.asarray(T, np.float32)
    if Q.ndim != 2 or T.ndim != 2 or Q.shape[1] != T.shape[1]:
        raise ValueError("Q [S, D] and T [n, D] must share D")
    if not 1 <= int(m) <= MAX_M:
        raise ValueError(f"m must be in [1, {MAX_M}]")
    if (q_scale is None) != (t_scale is None):
        raise ValueError("give both scales or neither")
    S, n = Q.shape[0], T.shape[0]
    m = int(m)
    ids = np.full((S, m), -1, np.int64)
    out = np.full((S, m), -np.inf, np.float32)
    counts = np.zeros(S, np.int64)
    rows = _host_rows(exclude) if src_ids is not None else None
    src = None if src_ids is None else np.asarray(src_ids, np.int64).reshape(-1)
    Td = T.astype(np.float64)
    node = np.arange(n, dtype=np.int64)
    with np.errstate(all="ignore"):
        for s in range(S):
            ok = np.ones(n, bool)
            if src is not None:
                u = int(src[s])
                if not 0 <= u < n:
                    continue
                if rows is not None:
                    ex = rows[1][rows[0][u]:rows[0][u + 1]]
                    ok[ex[(ex >= 0) & (ex < n)]] = False
                if exclude_self:
                    ok[u] = False
            sc = (Td @ Q[s].astype(np.float64)).astype(np.float32)
            if q_scale is not None:
                sc = (sc * np.float32(np.asarray(q_scale, np.float32)[s])).astype(np.float32)
                sc = (sc * np.asarray(t_scale, np.float32)).astype(np.float32)
            key = (order_key(sc).astype(np.uint64) << np.uint64(32)) | (~node.astype(np.uint32)).astype(np.uint64)
            key = key[ok]
            top = np.sort(key)[::-1][:m]
            c = top.size
            o = (top >> np.uint64(32)).astype(np.uint32)
            bits = np.where(o & 0x80000000, o & np.uint32(0x7fffffff), ~o).astype(np.uint32)
            bits[o == 0] = 0x7fc00000
            ids[s, :c] = (~(top & np.uint64(0xffffffff)).astype(np.uint32)).astype(np.int64)
            out[s, :c] = bits.view(np.float32)
            counts[s] = c
    return ids, out, counts


# ------------------------------------------------------------------------------------------------------ entry point
def _check_args(source, nodes, m, queries, table, metric, exclude):
    """The argument checks that need no device.  Returns (nodes as a 1-D integer tensor or None, queries or None)."""
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 1 <= int(m) <= MAX_M:
        raise ValueError(f"m must be an integer in [1, {MAX_M}]; got {m!r}")
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}; got {metric!r}")
    if isinstance(table, str):
        if table not in TABLES:
            raise ValueError(f"table must be one of {TABLES} or a float tensor [n, D]; got {table!r}")
    elif not (torch.is_tensor(table) and table.dtype.is_floating_point and table.dim() == 2):
        raise TypeError(f"table must be one of {TABLES} or a float tensor [n, D]")
    if nodes is None and queries is None:
        raise ValueError("give nodes (int [S]), queries (float [S, D]) or both")
    if nodes is not None:
        nodes = node_ids(nodes, "nodes")
        if nodes.dim() != 1:
            raise ValueError("nodes must be a 1-D tensor [S]")
    if queries is not None:
        queries = torch.as_tensor(queries)
        if not queries.dtype.is_floating_point or queries.dim() != 2:
            raise TypeError("queries must be a float tensor [S, D]")
        if nodes is not None and nodes.shape[0] != queries.shape[0]:
            raise ValueError("nodes and queries must have one entry per query: equal S")
        if torch.is_tensor(table) and table.shape[1] != queries.shape[1]:
            raise ValueError("queries and the table must share D")
    if isinstance(exclude, str) and exclude != "adj":
        raise ValueError("exclude must be 'adj', None, a graph.CSR or a graph.DeviceCSR")
    if exclude is not None and not isinstance(exclude, (str, graph.CSR, graph.DeviceCSR)):
        raise TypeError("exclude must be 'adj', None, a graph.CSR or a graph.DeviceCSR")
    if source is None and (isinstance(table, str) or isinstance(exclude, str)):
        raise ValueError("without a model, table must be a tensor and exclude None, a graph.CSR or a graph.DeviceCSR")
    return nodes, queries


def _inv_norm(rows: torch.Tensor) -> torch.Tensor:
    """1 / ||row||_2 in fp32; 0 for a zero row, so its cosines are 0 and not NaN."""
    nrm = torch.linalg.vector_norm(rows, dim=1)
    return torch.where(nrm > 0, 1.0 / nrm, torch.zeros_like(nrm)).contiguous()


def topm(Q: torch.Tensor, T: torch.Tensor, m: int, *, q_scale=None, t_scale=None, src_ids=None, exclude=None,
         exclude_self: bool = True, n_ranges: int = -1) -> Similar:
    """``lpf_similar_topm_f32`` on device tensors: ``Q`` [S, D] and ``T`` [n, D] as ``ops.f32_rows`` leaves them,
    ``src_ids`` int64 [S] or None, ``exclude`` a ``graph.DeviceCSR`` or None.  Nothing is read back."""
    dev = T.device
    S, D = Q.shape
    n = T.shape[0]
    ids = torch.full((S, m), -1, dtype=torch.int64, device=dev)
    out = torch.full((S, m), float("-inf"), dtype=torch.float32, device=dev)
    counts = torch.zeros(S, dtype=torch.int64, device=dev)
    if S == 0 or n == 0:
        return Similar(ids, out, counts)
    hip = _lib.hip()
    nbytes = hip.lpf_similar_workspace_bytes(S, int(m), int(n_ranges))
    if nbytes < 0:
        check(int(nbytes), "lpf_similar_workspace_bytes")
    with torch.cuda.device(dev):
        ws = torch.empty(max(int(nbytes) // 8, 1), dtype=torch.int64, device=dev)
        exc = (ptr(exclude.rowptr), ptr(exclude.col)) if exclude is not None else (None, None)
        check(hip.lpf_similar_topm_f32(S, n, D, ptr(Q), Q.stride(0), ptr(T), T.stride(0), ptr(q_scale), ptr(t_scale),
                                       ptr(src_ids), *exc, int(bool(exclude_self)), int(m), int(n_ranges), ptr(ws),
                                       ptr(ids), ptr(out), ptr(counts), ops.raw_stream(dev)), "lpf_similar_topm_f32")
    return Similar(ids, out, counts)


@torch.no_grad()
def similar_nodes(source, nodes=None, m: int = 64, *, queries=None, table="embedding", metric: str = "cosine",
                  exclude="adj", exclude_self: bool = True, test_set: bool = False, h=None,
                  n_ranges: int = -1) -> Similar:
    """The ``m`` nodes most similar to each query, most similar first (ties to the smaller id; NaN scores last).

    ``source``: a ``LinkTransformer`` (evaluation mode), or None when ``table`` is a tensor and ``exclude`` is None or a
    CSR.  ``table``: ``"embedding"`` -- ``h``, or ``model.propagate(test_set=...)``; ``"x"`` -- the raw node features;
    or a float tensor [n, D].  Queries: ``nodes`` (int [S]; duplicates are independent rows) are gathered from the
    table; ``queries`` (float [S, D]) are free vectors, such as a cold-start node's features -- they have no node, so
    nothing is excluded for them unless ``nodes`` names one per query as well.  ``metric``: ``"dot"``, or ``"cosine"``
    (the dot product times 1 / ||row||_2 of both rows, computed by torch in fp32; a zero row scores 0).  ``exclude``:
    ``"adj"`` (the model's typing adjacency of the split), None, a ``graph.CSR`` or a ``graph.DeviceCSR``;
    ``exclude_self`` drops the query's own node.  A node id outside [0, n) gets no result (count 0).
    ``n_ranges``: node ranges the kernel's grid splits the table into (negative: the library default); the result does
    not depend on it.  Nothing is read back to the host.  CPU tensors without a model go through
    ``similar_reference``."""
    nodes, queries = _check_args(source, nodes, m, queries, table, metric, exclude)
    m = int(m)
    if source is None:
        if not table.is_cuda:
            Q = queries if queries is not None else table[nodes.clamp(0, max(table.shape[0] - 1, 0)).long()]
            Tn = table.detach().float().numpy()
            Qn = Q.detach().float().numpy()
            if Tn.shape[0] == 0:
                return Similar(torch.full((Qn.shape[0], m), -1, dtype=torch.int64),
                               torch.full((Qn.shape[0], m), float("-inf")), torch.zeros(Qn.shape[0], dtype=torch.int64))
            sc = {}
            if metric == "cosine":
                sc = {"q_scale": _inv_norm(torch.from_numpy(Qn)).numpy(), "t_scale": _inv_norm(torch.from_numpy(Tn)).numpy()}
            got = similar_reference(Qn, Tn, m, src_ids=None if nodes is None else nodes.numpy(), exclude=exclude,
                                    exclude_self=exclude_self, **sc)
            return Similar(*(torch.from_numpy(a) for a in got))
        dev, adj = table.device, None
        model = SimpleNamespace(num_nodes=int(table.shape[0]))
    else:
        if source.training:
            raise NotImplementedError("similar_nodes needs model.eval(), as recommend does")
        model = source
        dev, adj, _ = model_graphs(model, test_set, "similar_nodes")
    from .recommend import _exclusion
    with torch.cuda.device(dev):
        if isinstance(table, str):
            if table == "embedding":
                T = h if h is not None else model.propagate(test_set=test_set)
            else:
                from .heuristics import device_features
                T = device_features(model.data["x"], dev)
        else:
            T = table.detach().to(dev)
        T = ops.f32_rows(T)
        n, D = T.shape
        if D < 1:
            raise ValueError("the table has no columns")
        if source is not None and n != int(model.num_nodes):
            raise ValueError(f"the table has {n} rows, the model {model.num_nodes} nodes")
        exc = _exclusion(model, exclude, adj, dev)
        src = None if nodes is None else nodes.to(dev, torch.int64).contiguous()
        if queries is not None:
            if queries.shape[1] != D:
                raise ValueError("queries and the table must share D")
            Q = ops.f32_rows(queries.detach().to(dev))
        else:
            Q = ops.f32_rows(T[src.clamp(0, max(n - 1, 0))])      # (an id outside [0, n) gets no result whatever its row)
        qs = ts = None
        if metric == "cosine":
            qs, ts = _inv_norm(Q), _inv_norm(T)
        return topm(Q, T, m, q_scale=qs, t_scale=ts, src_ids=src, exclude=exc if src is not None else None,
                    exclude_self=exclude_self, n_ranges=n_ranges)
