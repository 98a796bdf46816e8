"""The front end the pair-analysis entry points share: where a call gets its pairs, its graphs and
its chunks from.  Nothing here belongs to one feature.

    as_pairs / node_ids         edges -> [2, P] / 1-D integer ids, the caller's exception type on a wrong dtype
    clamp_chunk / chunks        pairs per launch, and the (lo, m) of each launch
    per_object / uploaded       per-object state kept while the object lives; the cached upload of a host CSR
    model_graphs / resolve      source -> (device, adjacency, PPR matrix, node features)
    csr_rows                    the entries of some rows of a host CSR, for the numpy restatements
"""
from __future__ import annotations

import weakref

import numpy as np
import torch

from . import _lib, graph


# ------------------------------------------------------------------------------------------------------------ pairs
def _integer_ids(t: torch.Tensor, what: str, exc) -> None:
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise exc(f"{what} must hold integer node ids")


def as_pairs(edges, *, what: str = "edges", exc=ValueError) -> torch.Tensor:
    """``edges`` ([P, 2], the reference's split layout, or [2, P]; a [2, 2] input reads as [2, P]) as a [2, P] view: no
    copy.  A floating, complex or bool dtype raises ``exc`` (``exc=None``: any dtype passes)."""
    edges = torch.as_tensor(edges)
    if edges.dim() != 2 or 2 not in edges.shape:
        raise ValueError(f"{what} must be [P, 2] (the reference's split layout) or [2, P]")
    if exc is not None:
        _integer_ids(edges, what, exc)
    return edges.t() if edges.shape[1] == 2 and edges.shape[0] != 2 else edges


def node_ids(t, what: str, exc=TypeError) -> torch.Tensor:
    """``t`` as a tensor of integer ids; a floating, complex or bool dtype raises ``exc``."""
    t = torch.as_tensor(t)
    _integer_ids(t, what, exc)
    return t


def clamp_chunk(chunk) -> int:
    """Pairs per launch: at least 1, at most what the int32 pair counters of the kernels hold."""
    if int(chunk) < 1:
        raise ValueError("chunk must be positive")
    return min(int(chunk), (1 << 31) - 2)


def chunks(P: int, chunk: int):
    """(lo, m) of each launch over ``P`` pairs, ``chunk`` at a time."""
    for lo in range(0, P, chunk):
        yield lo, min(chunk, P - lo)


# ----------------------------------------------------------------------------------------------------------- caches
def per_object(cache: dict, obj, make):
    """``make()`` once per live ``obj``: ``cache`` maps id(obj) -> (weak reference to it, value), checked by identity
    like the model's (kind, id(obj)) -> (obj, ...) caches; the entry goes when the object does."""
    hit = cache.get(id(obj))
    if hit is not None and hit[0]() is obj:
        return hit[1]
    val = make()
    key = id(obj)
    cache[key] = (weakref.ref(obj), val)
    weakref.finalize(obj, cache.pop, key, None)
    return val


_UPLOADS = ({}, {})            # [pattern_only]: host CSR -> its device copy


def uploaded(csr: graph.CSR, dev, pattern_only: bool = False) -> graph.DeviceCSR:
    """The device copy of a host CSR (``pattern_only``: without its values), uploaded once per object.  Where the cached
    copy lives on another device, this call gets an upload of its own and the cache stays."""
    def make():
        return (graph.CSR(csr.rowptr, csr.col, None, csr.n) if pattern_only else csr).to_device(dev)
    up = per_object(_UPLOADS[bool(pattern_only)], csr, make)
    return up if up.rowptr.device == dev else make()


# ---------------------------------------------------------------------------------------------------------- sources
def model_graphs(model, test_set: bool, who: str):
    """(device, typing adjacency, PPR matrix) of the split ``test_set`` selects: the resident ``DeviceCSR`` objects the
    model's selection reads."""
    dev = model.device
    if dev.type != "cuda":
        raise _lib.LpfError(f"{who}: the model must live on an MI355X; lpformer_amd has no CPU fallback")
    with torch.cuda.device(dev):
        return (dev, model._device_graph("mask", model._data_obj("mask", test_set)),
                model._device_graph("ppr", model._data_obj("ppr", test_set)))


def resolve(source, test_set: bool, like: torch.Tensor, *, who: str, pieces: bool = False, host_ok: bool = False):
    """(device, adjacency, PPR matrix or None, node features or None) of ``source``: a ``LinkTransformer``, a
    ``graph.CSR`` / ``graph.DeviceCSR`` adjacency or, with ``pieces``, the explicit (adjacency, PPR or None) or
    (adjacency, PPR or None, x or None).  Host containers are uploaded (``uploaded``) to the device of the resident
    pieces, else of ``like``, else the current one.  ``host_ok``: host containers, a CPU ``like`` and no GPU present
    give device None and the host containers themselves; otherwise that is an ``LpfError``."""
    from .link_transformer import LinkTransformer
    if isinstance(source, LinkTransformer):
        return model_graphs(source, test_set, who) + (source.data["x"],)
    adj, ppr, x = source, None, None
    if pieces and isinstance(source, (tuple, list)) and len(source) in (2, 3):
        adj, ppr, x = (tuple(source) + (None,))[:3]
    csr = (graph.CSR, graph.DeviceCSR)
    if not isinstance(adj, csr) or not (ppr is None or isinstance(ppr, csr)):
        raise TypeError(f"{who}: source must be a LinkTransformer, a graph.CSR or a graph.DeviceCSR" +
                        (", or explicit pieces (adjacency, PPR[, x]) of these" if pieces else ""))
    if ppr is not None and ppr.val is None:
        raise ValueError("the PPR matrix needs values")
    if ppr is not None and int(adj.n) != int(ppr.n):
        raise ValueError("the adjacency and the PPR matrix must describe the same nodes")
    resident = [g.rowptr.device for g in (adj, ppr) if isinstance(g, graph.DeviceCSR)]
    if any(d.type != "cuda" for d in resident):
        raise _lib.LpfError(f"{who}: a DeviceCSR must live on an MI355X (pass host graphs as graph.CSR)")
    if len(set(resident)) > 1:
        raise ValueError("the adjacency and the PPR matrix must live on the same device")
    if resident:
        dev = resident[0]
    elif like.is_cuda:
        dev = like.device
    elif torch.cuda.is_available():
        dev = torch.device("cuda", torch.cuda.current_device())
    elif host_ok:
        return None, adj, ppr, x
    else:
        raise _lib.LpfError(f"{who} needs an MI355X; lpformer_amd has no CPU fallback")
    if isinstance(adj, graph.CSR):
        adj = uploaded(adj, dev, pattern_only=True)      # (the adjacency is a binary pattern to every consumer)
    if isinstance(ppr, graph.CSR):
        ppr = uploaded(ppr, dev)
    return dev, adj, ppr, x


# ------------------------------------------------------------------------------------------------- host restatements
def csr_rows(rowptr, nodes):
    """The rows ``nodes`` (int64 array, repeats allowed) of a host CSR, concatenated: (flat, pos) int64 -- the index of
    each entry in the CSR's col / val, and the position in ``nodes`` of the row it belongs to."""
    start = rowptr[nodes]
    cnt = rowptr[nodes + 1] - start
    pos = np.repeat(np.arange(nodes.size, dtype=np.int64), cnt)
    flat = np.arange(int(cnt.sum()), dtype=np.int64) + np.repeat(start - (np.cumsum(cnt) - cnt), cnt)
    return flat, pos
