"""Common-neighbour pooling on the device and the NCN predictor on top of it.

    cn_pool(source, edges, table, weights=...)        [P, D]: the sum of the table's rows over each pair's common neighbours
    cn_entries(source, edges)                         CnEntries(seg, node): the common neighbours themselves
    cn_pool_reference / cn_entries_reference          the contract in fp64 / numpy on the host
    NCNPredictor, ncn_scores                          logit = Linear(MLP(h[a] * h[b]) + beta MLP(cn_pool)); chunked scorer

NCN (Wang, Yang, Zhang: "Neural Common Neighbor with Completion for Link Prediction") scores a pair from
``h[a] * h[b]`` and the sum of the encoder's rows over the pair's common neighbours.  It is also LPFormer's ablation:
with the attention replaced by uniform weights on the common neighbours only, LPFormer's pairwise stage is that sum.

Contract (shared by the kernels in csrc/cn_pool.hip and the restatements here).  The graph is the typing adjacency as
``pair_heuristics`` reads it: sorted, unique int32 columns, a binary pattern.  For a pair p = (a, b),
``C(p) = N(a) & N(b)`` in ascending node id, u_1 < ... < u_k.  A pair with an id outside [0, n) has k = 0; a == b gives
``C = N(a)`` (what ``pair_heuristics`` counts).  A node is in its own neighbourhood only where the graph stores a
self-loop, so a positive pair's own edge never enters its pool: NCN's target-link question -- does the edge being
predicted leak into its own features? -- is answered by the definition, whether or not the edge is in the graph.

    pool[p] = sum_j ( sum_{i in chunk j} w[u_i] T[u_i] )

with chunk j the entries [j CHUNK, (j + 1) CHUNK) of C(p), ``CHUNK = LPF_CN_POOL_CHUNK`` = 64: each chunk is summed
from zero in ascending order, one fp32 fused multiply-add per element and entry, and the chunks' rows are added in chunk
order.  Every row of ``pool`` is written, zeros where k = 0.  ``w`` is float32 [n] or absent (1.0) and is not
differentiated.  The result is a pure function of ({a, b}, graph, T, w): not of the pair's position in the batch, of
(a, b) versus (b, a), of ``chunk`` (pairs per launch), of ``split_threshold``, of the launch shape or of timing.  No
float atomics anywhere.

Backward, for T only: ``dT[u] = sum over the entries with node u, by ascending pair position, of w[u] g[p]``, evaluated
by ``lpf_skipgram_grad_rows_f32`` as it stands (table := g, coef := w or ones, occ_other := the pair position,
occ_pair := the node), so its order is that kernel's chunk-of-128 rule.  The entries come from ``lpf_cn_entries``; their
sort by node is built with torch (a stable sort, ``unique_consecutive``, a cumulative sum: the plumbing of
``skipgram.occurrence_list``).  Sizing the entry list reads ``seg[P]`` back: the one host read of the path, made only
where the list is needed (training, ``cn_entries``); ``unique_consecutive`` waits for the device a second time.  The
inference path reads nothing back.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch
from torch import nn

from . import _lib, graph, heuristics, ops, skipgram, sources
from ._lib import check, ptr

CHUNK = _lib.CONST["LPF_CN_POOL_CHUNK"]
MAX_DIM = _lib.CONST["LPF_CN_POOL_MAX_DIM"]
WEIGHTS = ("none", "aa", "ra")
_MAX = (1 << 31) - 2


class CnEntries(NamedTuple):
    seg: torch.Tensor                  # int64 [P + 1]: pair p's common neighbours are node[seg[p] : seg[p + 1]]
    node: torch.Tensor                 # int32 [E], ascending inside a pair


# ------------------------------------------------------------------------------------------------------------ checks
def _check_table(table) -> int:
    if not (isinstance(table, torch.Tensor) and table.dim() == 2 and table.dtype.is_floating_point):
        raise ValueError("cn_pool: table must be a floating tensor [n, D]")
    dim = int(table.shape[1])
    if dim % 4 or not 4 <= dim <= MAX_DIM:
        raise ValueError(f"cn_pool needs D % 4 == 0 and 4 <= D <= {MAX_DIM}; got {dim}")
    return dim


def _check_weights(weights, n: int):
    if isinstance(weights, str):
        if weights not in WEIGHTS:
            raise ValueError(f"weights must be one of {WEIGHTS} or a float32 tensor [n]; got {weights!r}")
        return weights
    if weights is None:
        return "none"
    if not (isinstance(weights, torch.Tensor) and weights.dim() == 1 and weights.dtype == torch.float32):
        raise ValueError(f"weights must be one of {WEIGHTS} or a float32 tensor [n]")
    if weights.numel() != n:
        raise ValueError(f"weights must hold one value per node: {n}; got {weights.numel()}")
    return weights.detach()


def _host_weights(csr: graph.CSR, weights):
    """float32 [n] on the host, or None: the values ``heuristics.weight_tables`` caches for a device graph."""
    if isinstance(weights, torch.Tensor):
        return weights.cpu()
    if weights == "none":
        return None
    deg = torch.from_numpy(np.diff(csr.rowptr)).to(torch.float64)
    if weights == "aa":
        w = torch.where(deg > 1, 1.0 / torch.log(deg.clamp_min(2.0)), torch.zeros_like(deg))
    else:
        w = torch.where(deg > 0, 1.0 / deg.clamp_min(1.0), torch.zeros_like(deg))
    return w.to(torch.float32)


# ------------------------------------------------------------------------------------------------- host restatement
def cn_entries_reference(csr: graph.CSR, pairs) -> CnEntries:
    """``C(p)`` of every pair by the contract, in numpy on the host: the row of a is walked and each column looked up
    among the (row, column) keys of the whole graph, which are ascending because the rows are."""
    a, b = (np.asarray(t, dtype=np.int64) for t in sources.as_pairs(pairs).cpu())
    n, P = int(csr.n), a.size
    rowptr, col = np.asarray(csr.rowptr, dtype=np.int64), np.asarray(csr.col, dtype=np.int64)
    ok = np.nonzero((a >= 0) & (a < n) & (b >= 0) & (b < n))[0]
    flat, pos = sources.csr_rows(rowptr, a[ok])
    keys = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr)) * n + col
    want = b[ok][pos] * n + col[flat]
    at = np.searchsorted(keys, want)
    hit = (at < keys.size) & (keys[np.minimum(at, max(keys.size - 1, 0))] == want) if keys.size else np.zeros(0, bool)
    cn = np.bincount(ok[pos[hit]], minlength=P) if P else np.zeros(0, np.int64)
    seg = np.zeros(P + 1, dtype=np.int64)
    np.cumsum(cn, out=seg[1:])
    return CnEntries(torch.from_numpy(seg), torch.from_numpy(col[flat][hit].astype(np.int32)))


def _pool_torch(ent: CnEntries, table: torch.Tensor, w, chunk: int) -> torch.Tensor:
    """The contract's sum in ``table``'s dtype, with the chunk order written out (``skipgram._segment_sums``: on the
    CPU ``index_add_`` adds in index order); differentiable in ``table`` by ordinary autograd."""
    node = ent.node.to(torch.int64)
    contrib = table[node]
    if w is not None:
        contrib = w.to(table.dtype)[node, None] * contrib
    return skipgram._segment_sums(contrib, ent.seg[1:] - ent.seg[:-1], int(chunk))


@torch.no_grad()
def cn_pool_reference(csr: graph.CSR, pairs, table, w=None, chunk: int = CHUNK) -> torch.Tensor:
    """``cn_pool`` by the module docstring's contract in fp64 on the host: [P, D] float64.  ``w``: float32 [n] or None;
    its fp32 values are what the sum uses.  ``chunk``: the entries per chunk (in fp64 it moves the last bits only)."""
    t = table.detach().cpu().to(torch.float64)
    return _pool_torch(cn_entries_reference(csr, pairs), t, None if w is None else w.detach().cpu().to(torch.float32),
                       chunk)


# ------------------------------------------------------------------------------------------------------ device path
def _device_weights(adj, weights):
    if isinstance(weights, torch.Tensor):
        return weights.to(adj.rowptr.device).contiguous()
    if weights == "none":
        return None
    return heuristics.weight_tables(adj)[0 if weights == "aa" else 1]


def _kernel_table(table: torch.Tensor) -> torch.Tensor:
    """``table`` as the kernels read it: unit stride along D, a row stride that is a multiple of 4 floats, a 16-byte
    aligned base -- itself where it already is, a contiguous copy otherwise."""
    t = table.detach()
    if t.stride(1) != 1 or t.stride(0) % 4 or t.stride(0) < t.shape[1] or t.data_ptr() % 16:
        t = t.contiguous()
    return t


def _pool_device(adj, batch, w, table, chunk, thr, want_cn):
    """The fused kernel over the chunks: (pool float32 [P, D], cn int32 [P] or None).  Nothing is read back."""
    dev, P, D = batch.device, batch.shape[1], table.shape[1]
    pool = torch.empty((P, D), dtype=torch.float32, device=dev)
    cn = torch.empty(P, dtype=torch.int32, device=dev) if want_cn else None
    if P:
        st = ops.raw_stream(dev)
        scratch = torch.empty(min(P, chunk) + 1, dtype=torch.int32, device=dev)
        for lo, m in sources.chunks(P, chunk):
            check(_lib.hip().lpf_cn_pool_f32(
                m, adj.n, batch.data_ptr() + lo * 8, P, ptr(adj.rowptr), ptr(adj.col), ptr(w), D, ptr(table),
                table.stride(0), thr, ptr(scratch), pool.data_ptr() + lo * D * 4, D,
                None if cn is None else cn.data_ptr() + lo * 4, st), "lpf_cn_pool_f32")
    return pool, cn


def _segments(cn: torch.Tensor):
    """(seg int64 [P + 1], E): the exclusive scan of the counts and its last value, READ BACK to size the list."""
    seg = torch.zeros(cn.numel() + 1, dtype=torch.int64, device=cn.device)
    torch.cumsum(cn, 0, out=seg[1:])
    total = int(seg[-1])
    if total > _MAX:
        raise ValueError("cn_pool: a call holds fewer than 2^31 - 1 common-neighbour entries; pass fewer pairs")
    return seg, total


def _entries_device(adj, batch, seg, total, chunk, thr) -> torch.Tensor:
    dev, P = batch.device, batch.shape[1]
    node = torch.empty(total, dtype=torch.int32, device=dev)
    if P and total:
        st = ops.raw_stream(dev)
        scratch = torch.empty(min(P, chunk) + 1, dtype=torch.int32, device=dev)
        for lo, m in sources.chunks(P, chunk):
            check(_lib.hip().lpf_cn_entries(m, adj.n, batch.data_ptr() + lo * 8, P, ptr(adj.rowptr), ptr(adj.col), thr,
                                            ptr(scratch), seg.data_ptr() + lo * 8, total, ptr(node), st),
                  "lpf_cn_entries")
    return node


class CnPoolFn(torch.autograd.Function):
    """``cn_pool`` with a gradient for the table: the fused kernel forward; backward the entry list, its stable sort by
    node and ``lpf_skipgram_grad_rows_f32``, the compact rows written into a zero [n, D] gradient."""

    @staticmethod
    def forward(ctx, table, adj, batch, w, chunk, thr):
        with torch.cuda.device(batch.device):
            pool, cn = _pool_device(adj, batch, w, _kernel_table(table), chunk, thr, True)
        ctx.adj, ctx.batch, ctx.w, ctx.chunk, ctx.thr = adj, batch, w, chunk, thr
        ctx.shape = tuple(table.shape)
        ctx.mark_non_differentiable(cn)
        ctx.save_for_backward(cn)
        return pool, cn

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _):
        adj, batch, (cn,) = ctx.adj, ctx.batch, ctx.saved_tensors
        dev, P, (n, D) = batch.device, batch.shape[1], ctx.shape
        with torch.cuda.device(dev):
            dT = torch.zeros((n, D), dtype=torch.float32, device=dev)
            seg, total = _segments(cn)                         # the forward's count is reused
            if total == 0:
                return dT, None, None, None, None, None
            node = _entries_device(adj, batch, seg, total, ctx.chunk, ctx.thr)
            pos = torch.repeat_interleave(torch.arange(P, dtype=torch.int32, device=dev), cn.to(torch.int64),
                                          output_size=total)
            by_node, perm = torch.sort(node, stable=True)      # a node's entries keep their pair positions' order
            rows, counts = torch.unique_consecutive(by_node, return_counts=True)
            U = rows.numel()
            seg_u = torch.zeros(U + 1, dtype=torch.int64, device=dev)
            torch.cumsum(counts, 0, out=seg_u[1:])
            occ_other = pos[perm].contiguous()
            g = _kernel_table(g.to(torch.float32))
            coef = ctx.w if ctx.w is not None else torch.ones(n, dtype=torch.float32, device=dev)
            grad = torch.empty((U, D), dtype=torch.float32, device=dev)
            scratch = torch.empty((-(-total // skipgram.CHUNK), D), dtype=torch.float32, device=dev)
            check(_lib.hip().lpf_skipgram_grad_rows_f32(P, D, ptr(g), g.stride(0), n, ptr(coef), total, ptr(occ_other),
                                                        ptr(by_node), U, ptr(seg_u), ptr(grad), D, ptr(scratch),
                                                        scratch.shape[0], 0, ops.raw_stream(dev)),
                  "lpf_skipgram_grad_rows_f32")
            dT.index_copy_(0, rows.to(torch.int64), grad)
        return dT, None, None, None, None, None


def _host_source(source, *tensors) -> bool:
    return isinstance(source, graph.CSR) and all(t.device.type == "cpu" for t in tensors)


def cn_pool(source, edges, table, *, weights="none", test_set: bool = False, chunk: int = 1 << 20,
            split_threshold: int = -1, return_count: bool = False):
    """``pool`` float32 [P, D] on the device: for each pair of ``edges`` ([P, 2] or [2, P]) the sum of ``table``'s rows
    ([n, D] float32, ``D % 4 == 0``, ``4 <= D <= 512``) over the pair's common neighbours on the typing adjacency, by the
    module docstring's contract.  ``return_count``: also ``cn`` int32 [P].

    ``source``: a ``LinkTransformer`` (the typing adjacency of the split ``test_set`` selects), a ``graph.CSR`` or a
    ``graph.DeviceCSR``.  ``weights``: ``"none"``, ``"aa"`` (1 / ln deg), ``"ra"`` (1 / deg) -- the cached
    ``heuristics.weight_tables`` -- or a float32 [n] tensor; weights take no gradient.  ``chunk``: pairs per launch;
    ``split_threshold``: walked-row length above which a pair gets a whole workgroup (negative: the library default);
    neither changes a bit of the result.

    A pair's own edge is never in its pool (a node is its own neighbour only through a stored self-loop), so positives
    and negatives are pooled alike whether or not the positives are edges of the graph.

    Without a gradient nothing is read back.  Where ``table.requires_grad`` the call goes through ``CnPoolFn``: its
    backward reads the number of entries back once and builds their sort by node with torch.  CPU tensors with a host
    ``graph.CSR`` go through the torch restatement (in ``table``'s dtype, differentiable by ordinary autograd)."""
    chunk = sources.clamp_chunk(chunk)
    batch = sources.as_pairs(edges)
    dim = _check_table(table)
    if _host_source(source, table, batch):
        w = _host_weights(source, _check_weights(weights, int(source.n)))
        if table.shape[0] != source.n:
            raise ValueError(f"cn_pool: table must hold one row per node: {source.n}; got {table.shape[0]}")
        ent = cn_entries_reference(source, batch)
        pool = _pool_torch(ent, table, w, CHUNK)
        return (pool, (ent.seg[1:] - ent.seg[:-1]).to(torch.int32)) if return_count else pool
    if table.device.type != "cuda":
        raise ValueError(f"cn_pool: table lives on {table.device}, not on the graph's device (CPU tensors go with a "
                         "host graph.CSR)")
    dev, adj, _, _ = sources.resolve(source, test_set, table, who="cn_pool")
    if table.device != dev:
        raise ValueError(f"cn_pool: table lives on {table.device}, the graph on {dev}")
    if table.dtype != torch.float32:
        raise ValueError("cn_pool: on the device the table must be float32")
    if table.shape[0] != adj.n:
        raise ValueError(f"cn_pool: table must hold one row per node: {adj.n}; got {table.shape[0]}")
    w = _device_weights(adj, _check_weights(weights, int(adj.n)))
    batch = batch.to(dev, dtype=torch.int64).contiguous()
    thr = int(split_threshold)
    if table.requires_grad and torch.is_grad_enabled():
        pool, cn = CnPoolFn.apply(table, adj, batch, w, chunk, thr)
    else:
        with torch.no_grad(), torch.cuda.device(dev):
            pool, cn = _pool_device(adj, batch, w, _kernel_table(table), chunk, thr, return_count)
    return (pool, cn) if return_count else pool


@torch.no_grad()
def cn_entries(source, edges, *, test_set: bool = False, split_threshold: int = -1) -> CnEntries:
    """The common neighbours themselves, ``CnEntries(seg int64 [P + 1], node int32 [E])``: pair p's are
    ``node[seg[p] : seg[p + 1]]``, ascending -- for ``explain``-style listings.  Sizing ``node`` reads one number back.
    A host ``graph.CSR`` with CPU ``edges`` goes through ``cn_entries_reference``."""
    batch = sources.as_pairs(edges)
    if _host_source(source, batch):
        return cn_entries_reference(source, batch)
    dev, adj, _, _ = sources.resolve(source, test_set, batch, who="cn_entries")
    batch = batch.to(dev, dtype=torch.int64).contiguous()
    P, chunk, thr = batch.shape[1], 1 << 20, int(split_threshold)
    with torch.cuda.device(dev):
        cn = torch.empty(P, dtype=torch.int32, device=dev)
        if P:
            scratch = torch.empty(min(P, chunk) + 1, dtype=torch.int32, device=dev)
            for lo, m in sources.chunks(P, chunk):
                check(_lib.hip().lpf_pair_heuristics_f32(
                    m, adj.n, batch.data_ptr() + lo * 8, P, ptr(adj.rowptr), ptr(adj.col), None, None, thr,
                    ptr(scratch), cn.data_ptr() + lo * 4, None, None, ops.raw_stream(dev)), "lpf_pair_heuristics_f32")
        seg, total = _segments(cn)
        return CnEntries(seg, _entries_device(adj, batch, seg, total, chunk, thr))


# -------------------------------------------------------------------------------------------------------- predictor
def _mlp(dim_in: int, hidden: int, layers: int, dropout: float) -> nn.Sequential:
    mods, d = [], dim_in
    for i in range(layers):
        mods.append(nn.Linear(d, hidden))
        if i + 1 < layers:
            mods += [nn.ReLU()] + ([nn.Dropout(dropout)] if dropout > 0 else [])
        d = hidden
    return nn.Sequential(*mods)


class NCNPredictor(nn.Module):
    """NCN's link predictor: ``logit = Linear( MLP_ij(h[a] * h[b]) + beta MLP_cn(cn_pool(source, edges, h)) )``, with
    ``beta`` a learnable scalar.  The dense part is a few small GEMMs in plain ``nn.Linear`` / ReLU; the pooling is
    ``cn_pool`` (``weights`` as there), differentiable in ``h``.

    Written from the NCN paper's equation.  The authors' code is not available to this project, so this module is
    pinned against nothing of theirs: layer counts, where the nonlinearities sit and the initialisation are this
    module's own.  NCNC's completion step is not implemented.

    ``forward(source, h, edges, test_set=False)`` -> logits [P].  ``h``: [n, dim], e.g. ``model.propagate()`` for
    scoring or ``train.encoder_train(model)`` for joint training; every id of ``edges`` must lie in [0, n)."""

    def __init__(self, dim: int, hidden=None, layers: int = 2, beta: float = 1.0, dropout: float = 0.0, weights="none"):
        super().__init__()
        if int(layers) < 1:
            raise ValueError("NCNPredictor: layers must be at least 1")
        if isinstance(weights, str) and weights not in WEIGHTS:
            raise ValueError(f"weights must be one of {WEIGHTS} or a float32 tensor [n]; got {weights!r}")
        hidden = int(dim if hidden is None else hidden)
        self.weights = weights
        self.mlp_ij = _mlp(int(dim), hidden, int(layers), float(dropout))
        self.mlp_cn = _mlp(int(dim), hidden, int(layers), float(dropout))
        self.beta = nn.Parameter(torch.tensor(float(beta)))
        self.out = nn.Linear(hidden, 1)

    def forward(self, source, h, edges, test_set: bool = False):
        batch = sources.as_pairs(edges).to(h.device, dtype=torch.int64)
        pool = cn_pool(source, batch, h, weights=self.weights, test_set=test_set)
        z = self.mlp_ij(h[batch[0]] * h[batch[1]]) + self.beta * self.mlp_cn(pool.to(h.dtype))
        return self.out(z).squeeze(-1)


@torch.no_grad()
def ncn_scores(source, predictor: NCNPredictor, h, edges, chunk: int = 1 << 16, test_set: bool = False) -> torch.Tensor:
    """Logits [P] of ``edges`` from ``predictor`` in evaluation mode, ``chunk`` pairs at a time, without a gradient:
    ready for ``evaluate.link_metrics`` / ``compare_metrics``.  Nothing is read back."""
    chunk = sources.clamp_chunk(chunk)
    batch = sources.as_pairs(edges).to(h.device, dtype=torch.int64)
    was = predictor.training
    predictor.eval()
    try:
        out = [predictor(source, h, batch[:, lo:lo + m], test_set) for lo, m in sources.chunks(batch.shape[1], chunk)]
    finally:
        predictor.train(was)
    return torch.cat(out) if out else torch.zeros(0, dtype=h.dtype, device=h.device)
