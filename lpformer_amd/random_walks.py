"""Biased random walks on the typing adjacency, drawn on the device, and Node2Vec embeddings from them.

The heuristic columns of a HeaRT / OGB comparison table are here (``pair_heuristics``, ``pair_distance``,
``pair_katz``, PPR); the next rows are the embedding methods, Node2Vec first -- also what a featureless graph gets
concatenated to ``x`` on the OGB link leaderboards.  PyG's ``Node2Vec`` takes its walks from CUDA extensions
(torch-cluster / pyg-lib) that a ROCm install does not have.  Here

    random_walks(source, starts, length=..., p=..., q=..., seed=...)   Walks(walks int32 [W, length+1], forced int32 [W])
    walks_reference(csr, starts, ...)                                  the numpy restatement, what a host CSR without a GPU runs
    walk_thresholds(p, q)                                              the three integer acceptance thresholds
    walk_pairs(walks, context)                                         int64 [2, M] (centre, context) pairs, as PyG cuts them
    node2vec_embeddings(source, dim, ...)                              (emb float32 [n, dim], losses): skip-gram in torch,
                                                                       or on the device with trainer="device" (skipgram.py)

Contract (shared by the kernel, ``lpf_random_walks`` in csrc/random_walk.hip, and ``walks_reference``, which are equal
integer for integer).  The graph is a CSR with sorted, unique int32 columns and a SYMMETRIC pattern, the typing
adjacency; values are ignored; a walk moves along stored entries and a stored self-loop is an entry like any other.
The draws are those of ``negatives`` with no new definition::

    key_w = key(seed, walk id);  u(j) = mix64(key_w + G (j + 1));  node(u, d) = (u * d) >> 64

Walk w has the id ``walk_base + w`` and the start ``starts[w]``.  ``walk[0] = start``; a start outside [0, n) gives a
row of -1 and a forced count of 0.  Step t = 1 .. L, with ``cur = walk[t-1]``, d the stored entries of row cur and
T = ``max_tries``:

1. ``d == 0``: ``walk[t] = cur`` (the walk stays, as PyG pads);
2. otherwise attempt a = 0, 1, ... draws the candidate ``x = col[rowptr[cur] + node(u(2 ((t-1) T + a)), d)]``;
3. the first candidate is taken without a test if ``t == 1``, ``d == 1`` or ``p == q == 1``;
4. otherwise, with ``prev = walk[t-2]``, x is of class *return* (``x == prev``, weight 1/p; this class wins over the
   next), *common* (x is stored in row prev, weight 1) or *out* (anything else, weight 1/q),
5. and is accepted iff ``(u(2 ((t-1) T + a) + 1) >> 1) < thr[class]``,
6. ``thr[class] = floor(2^63 weight / max weight)`` (``walk_thresholds``: exact, from the doubles p and q as
   fractions); the heaviest class has 2^63 and always accepts;
7. after T refused attempts the last candidate is taken and ``forced[w]`` is incremented.

So a class of weight ratio r is taken with probability r per attempt up to 2^-63, which is the node2vec distribution
by rejection; ``forced`` counts the steps where the bound T cut the rejection short (their draw is the plain uniform
one).  A walk is a pure function of (seed, walk id, start, graph, L, p, q, T): not of W, of chunking by ``walk_base``,
of the launch shape, of ``form`` or of timing.  No floats on the device, no atomics.

Leakage.  Embeddings used to score validation or test pairs must be computed on the TRAINING graph: a model source
with ``test_set=False``, or the adjacency of ``link_split``'s ``data["adj_mask"]`` -- never an edge list that still
holds validation or test edges, whose walks would hand the answer to the embedding.
"""
from __future__ import annotations

from fractions import Fraction
from typing import NamedTuple

import numpy as np
import torch

from . import _lib, graph, negatives, ops, skipgram, sources
from ._lib import check, ptr

MAX_LENGTH = _lib.CONST["LPF_WALK_MAX_LENGTH"]
MAX_TRIES = _lib.CONST["LPF_WALK_MAX_TRIES"]
TRIES = _lib.CONST["LPF_WALK_TRIES_DEFAULT"]
FORMS = {"default": _lib.CONST["LPF_WALK_FORM_DEFAULT"], "lane": _lib.CONST["LPF_WALK_FORM_LANE"],
         "group8": _lib.CONST["LPF_WALK_FORM_GROUP8"]}
_MAX = (1 << 31) - 2                   # n, nnz, W < 2^31 - 1
_ALWAYS = 1 << 63
_EPS = 1e-15                           # PyG's Node2Vec.loss


class Walks(NamedTuple):
    walks: torch.Tensor                # int32 [W, length + 1]; a bad start: -1 throughout
    forced: torch.Tensor               # int32 [W]: steps that took their last candidate after max_tries refusals


# ---------------------------------------------------------------------------------------------------------- options
def walk_thresholds(p, q) -> tuple:
    """(thr_return, thr_common, thr_out) as Python ints: ``floor(2^63 w / max w)`` for the weights (1/p, 1, 1/q), in
    exact arithmetic on the doubles p and q.  The heaviest class gets 2^63: it always accepts."""
    p, q = float(p), float(q)
    if not (0.0 < p < float("inf") and 0.0 < q < float("inf")):
        raise ValueError(f"p and q must be positive and finite; got {p!r}, {q!r}")
    w = (1 / Fraction(p), Fraction(1), 1 / Fraction(q))
    top = max(w)
    return tuple(int(_ALWAYS * x / top) for x in w)       # int() of a positive Fraction floors


def _check_walk(length, max_tries, walks_per_node, walk_base):
    L = negatives._check_count(length, "length", 1, MAX_LENGTH)
    T = negatives._check_count(max_tries, "max_tries", 1, MAX_TRIES)
    r = negatives._check_count(walks_per_node, "walks_per_node", 1, _MAX)
    base = negatives._check_count(walk_base, "walk_base", 0, (1 << 63) - 1)
    return L, T, r, base


def _start_list(starts, n: int, r: int) -> torch.Tensor:
    """The starts of a call, 1-D: ``starts`` (None: every node) ``r`` times, repeat-major."""
    if starts is None:
        ids = torch.arange(int(n), dtype=torch.int64)
    else:
        ids = sources.node_ids(starts, "starts", ValueError).reshape(-1)
    if ids.numel() * r > _MAX:
        raise ValueError("random_walks: a call holds fewer than 2^31 - 1 walks; cut it with walk_base")
    return ids.repeat(r) if r > 1 else ids


def _check_graph(adj) -> None:
    if int(adj.n) > _MAX or int(adj.nnz) > _MAX:
        raise ValueError("random_walks: the graph must have fewer than 2^31 - 1 nodes and stored entries")


# ------------------------------------------------------------------------------------------------- host restatement
def _mulhi(u: np.ndarray, d: np.ndarray) -> np.ndarray:
    """``(u * d) >> 64`` element by element as int64, exact for d < 2^31: ``negatives.draw_node``'s two-halves form with
    an array d."""
    s32, d = np.uint64(32), d.astype(np.uint64)
    return (((u >> s32) * d + (((u & np.uint64(0xFFFFFFFF)) * d) >> s32)) >> s32).astype(np.int64)


def walks_reference(csr: graph.CSR, starts=None, *, length, walks_per_node=1, p=1.0, q=1.0, seed, max_tries=TRIES,
                    walk_base=0) -> Walks:
    """``random_walks`` of a host CSR in numpy, vectorised over the walks (CPU tensors out): per step, the walks that
    still look for a candidate draw attempt a together; membership in row prev is a search in the ascending entry keys
    ``row * n + col``.  The restatement the kernel is tested against, and what ``random_walks`` runs when there is no
    GPU."""
    if not isinstance(csr, graph.CSR):
        raise TypeError("walks_reference takes a host graph.CSR")
    _check_graph(csr)
    L, T, r, base = _check_walk(length, max_tries, walks_per_node, walk_base)
    seed = negatives._check_seed(seed)
    thr = np.array(walk_thresholds(p, q), dtype=np.uint64)
    second = any(int(t) != _ALWAYS for t in thr)
    n = int(csr.n)
    start = _start_list(starts, n, r).cpu().to(torch.int64).numpy()
    W = start.size
    walks = np.full((W, L + 1), -1, np.int32)
    forced = np.zeros(W, np.int32)
    live = np.flatnonzero((start >= 0) & (start < n))
    if live.size:
        rowptr, col = np.asarray(csr.rowptr, np.int64), np.asarray(csr.col).astype(np.int64)
        keys = negatives._entry_keys(csr)
        key = negatives.draw_key(seed, (live.astype(np.uint64) + np.uint64(base)))
        cur = start[live].copy()
        prev = np.full(live.size, -1, np.int64)
        walks[live, 0] = cur
        for t in range(1, L + 1):
            r0 = rowptr[cur]
            d = rowptr[cur + 1] - r0
            nxt = cur.copy()                                   # d == 0: the walk stays
            todo = np.flatnonzero(d > 0)
            for a in range(T):
                if not todo.size:
                    break
                j = np.uint64(2 * ((t - 1) * T + a))
                x = col[r0[todo] + _mulhi(negatives.draw_u(key[todo], j), d[todo])]
                nxt[todo] = x                                  # (a refused candidate is overwritten by the next)
                if t == 1 or not second:
                    break
                cls = np.where(x == prev[todo], 0, np.where(negatives._stored(keys, n, prev[todo], x), 1, 2))
                ok = (d[todo] == 1) | ((negatives.draw_u(key[todo], j + np.uint64(1)) >> np.uint64(1)) < thr[cls])
                todo = todo[~ok]
                if a == T - 1:
                    forced[live[todo]] += 1
            prev, cur = cur, nxt
            walks[live, t] = cur
    return Walks(torch.from_numpy(walks), torch.from_numpy(forced))


# ------------------------------------------------------------------------------------------------------ device path
@torch.no_grad()
def random_walks(source, starts=None, *, length, walks_per_node=1, p=1.0, q=1.0, seed, max_tries=TRIES,
                 test_set: bool = False, walk_base=0, form: str = "default") -> Walks:
    """``walks_per_node`` walks of ``length`` steps from each of ``starts`` by the module docstring's contract:
    ``Walks(walks int32 [W, length + 1], forced int32 [W])`` on the device.  ``walks`` is the transposed view of the
    kernel's step-major buffer (``.contiguous()`` where rows must be contiguous).

    ``source``: a ``LinkTransformer`` (the typing adjacency of the split ``test_set`` selects), a ``graph.DeviceCSR`` or
    a ``graph.CSR`` (uploaded once per object): a binary SYMMETRIC pattern.  ``starts``: node ids, any shape, host or
    device (None: every node); the list is repeated ``walks_per_node`` = r times, repeat-major, so with S starts the
    walk of repeat ``rep`` from ``starts[i]`` has the id ``walk_base + rep * S + i``.  ``p``, ``q``: node2vec's return
    and in-out parameters (1, 1: the first-order uniform walk, no test at all).  ``max_tries``: attempts per step
    before the last candidate is forced.  ``walk_base``: the id of walk 0, so that a caller cuts a long list into
    calls without changing a walk.  ``form``: ``"default"``, ``"lane"`` (a lane per walk) or ``"group8"`` (eight lanes
    per walk probe row prev together), for measurement: the result is the same.

    Nothing is read back.  A host ``graph.CSR`` with CPU ``starts`` and no GPU present goes through
    ``walks_reference`` and gives CPU tensors."""
    L, T, r, base = _check_walk(length, max_tries, walks_per_node, walk_base)
    seed = negatives._check_seed(seed)
    thr = walk_thresholds(p, q)
    if form not in FORMS:
        raise ValueError(f"form must be one of {tuple(FORMS)}; got {form!r}")
    like = torch.empty(0) if starts is None else sources.node_ids(starts, "starts", ValueError)
    dev, adj, _, _ = sources.resolve(source, test_set, like, who="random_walks", host_ok=True)
    if dev is None:
        return walks_reference(adj, starts, length=L, walks_per_node=r, p=p, q=q, seed=seed, max_tries=T,
                               walk_base=base)
    _check_graph(adj)
    n = int(adj.n)
    ids = _start_list(starts, n, r).to(dev, dtype=torch.int64).contiguous()
    W = ids.numel()
    with torch.cuda.device(dev):
        if W == 0 or n == 0:
            return Walks(torch.full((W, L + 1), -1, dtype=torch.int32, device=dev),
                         torch.zeros(W, dtype=torch.int32, device=dev))
        buf = torch.empty((L + 1, W), dtype=torch.int32, device=dev)
        forced = torch.empty(W, dtype=torch.int32, device=dev)
        second = 1 if any(t != _ALWAYS for t in thr) else 0
        check(_lib.hip().lpf_random_walks(n, int(adj.nnz), ptr(adj.rowptr), ptr(adj.col), W, ptr(ids), base, L, seed,
                                          thr[0], thr[1], thr[2], second, T, FORMS[form], ptr(buf), W, ptr(forced),
                                          ops.raw_stream(dev)), "lpf_random_walks")
    return Walks(buf.t(), forced)


# ------------------------------------------------------------------------------------------------------- skip-gram
def _windows(walks: torch.Tensor, context: int) -> torch.Tensor:
    """[W, length + 2 - context, context]: every run of ``context`` consecutive positions of every walk (a view)."""
    if walks.dim() != 2 or walks.dtype.is_floating_point or walks.dtype == torch.bool:
        raise ValueError("walks must be an integer tensor [W, length + 1]")
    context = negatives._check_count(context, "context", 2, max(int(walks.shape[1]), 2))
    if context > walks.shape[1]:
        raise ValueError(f"context ({context}) must be at most the walk's positions ({walks.shape[1]})")
    return walks.unfold(1, context, 1)


def walk_pairs(walks: torch.Tensor, context: int) -> torch.Tensor:
    """The (centre, context) pairs of skip-gram training, int64 [2, M] on the walks' device: every window of ``context``
    consecutive positions of a walk gives the pairs (window[0], window[k]), k = 1 .. context - 1 -- the first position
    is the centre, as PyG's Node2Vec cuts its walks.  Windows that hold a -1 (a bad start) are dropped.  Order: by
    walk, then by window, then by k.  Plain torch."""
    win = _windows(walks, context)
    win = win[(win >= 0).all(dim=2)].to(torch.int64)              # [windows, context]
    centre = win[:, :1].expand(-1, win.shape[1] - 1)
    return torch.stack([centre.reshape(-1), win[:, 1:].reshape(-1)])


def _skipgram_loss(emb: torch.nn.Embedding, pos: torch.Tensor, neg: torch.Tensor) -> torch.Tensor:
    """PyG's Node2Vec.loss on windows [*, context]: -log sigmoid(<start, rest>) over the positive windows plus
    -log(1 - sigmoid(<start, rest>)) over the negative ones, each a mean."""
    def logits(win):
        h = emb(win)                                              # [*, context, dim]
        return (h[:, :1] * h[:, 1:]).sum(dim=-1).reshape(-1)
    return (-torch.log(torch.sigmoid(logits(pos)) + _EPS).mean()
            - torch.log(1 - torch.sigmoid(logits(neg)) + _EPS).mean())


def node2vec_embeddings(source, dim: int = 128, *, walk_length: int = 20, context: int = 10, walks_per_node: int = 10,
                        p=1.0, q=1.0, num_neg: int = 1, epochs: int = 1, batch_walks: int = 1280, lr: float = 0.01,
                        seed: int = 0, test_set: bool = False, max_tries=TRIES, trainer: str = "torch",
                        max_steps=None):
    """Node2Vec embeddings of the typing adjacency: ``(emb float32 [n, dim] on the device, losses)``, ``losses`` the mean
    loss of each epoch's steps.

    An epoch walks from every node ``walks_per_node`` times, ``walk_length`` steps each (``random_walks``: the kernel,
    in chunks of ``batch_walks`` walks cut with ``walk_base``; epoch e uses the walk ids from ``e * n * walks_per_node``
    on, so epochs see different walks), in a node order shuffled per epoch.  A chunk is one optimiser step: its walks
    are cut into windows of ``context`` positions, and each positive walk gets ``num_neg`` negative ones -- its start
    followed by uniform random nodes -- cut the same way.  The skip-gram update with negative sampling stays in torch:
    ``nn.Embedding(sparse=True)`` + ``SparseAdam(lr)`` with PyG's loss (``Node2Vec.loss``); no kernel of this package
    is in it.

    The WALKS are a pure function of their arguments; the embeddings are NOT bitwise repeatable, because torch's sparse
    gradient accumulation adds in no fixed order.  The shuffle, the initial table (standard normal, as
    ``nn.Embedding``) and the negatives come from one ``torch.Generator`` seeded with ``seed``.

    ``trainer="device"`` runs the same step -- the same loss, the same ``SparseAdam`` -- through
    ``skipgram.skipgram_step``: no gathered blocks, no float atomics, one summation order.  It needs a
    GPU source and ``dim % 4 == 0 and dim <= 512`` (``ValueError`` otherwise), takes the walks straight from the
    kernel's step-major buffer, and draws the table, the shuffle and the noise nodes from the same generator in the
    same order, so both trainers see the same walks and negatives.  With ``trainer="device"`` the embeddings ARE
    bitwise repeatable on one machine: two calls with equal arguments give equal bits.  The default stays ``"torch"``.
    The two trainers differ in VALUE where torch's fp32 ``1 - sigmoid(l)`` is exactly 0 (l above about 17: loss 34.5,
    gradient 0); the device evaluates the same expression in fp64 from its fp32 logit.
    ``max_steps``: stop after this many optimiser steps in all (None: whole epochs); ``losses`` then holds the mean
    over the steps taken of every epoch begun.

    Leakage: compute the embeddings on the TRAINING graph -- ``test_set=False`` for a model source, or the adjacency of
    ``link_split``'s ``data["adj_mask"]`` -- never on an edge list that still holds validation or test edges.  Use them
    as a column (``(emb[a] * emb[b]).sum(-1)`` into ``evaluate.link_metrics``, set against the model with
    ``compare_metrics``) or as input (``torch.cat([x, emb], 1)``).

    A host ``graph.CSR`` with no GPU present runs the restatement's walks and the same torch loop on the CPU."""
    dim = negatives._check_count(dim, "dim", 1, 1 << 16)
    L = negatives._check_count(walk_length, "walk_length", 1, MAX_LENGTH)
    context = negatives._check_count(context, "context", 2, L + 1)
    r = negatives._check_count(walks_per_node, "walks_per_node", 1, _MAX)
    num_neg = negatives._check_count(num_neg, "num_neg", 1, 1 << 10)
    epochs = negatives._check_count(epochs, "epochs", 1, 1 << 20)
    chunk = negatives._check_count(batch_walks, "batch_walks", 1, _MAX)
    seed = negatives._check_seed(seed)
    walk_thresholds(p, q)
    if trainer not in ("torch", "device"):
        raise ValueError(f'trainer must be "torch" or "device"; got {trainer!r}')
    if max_steps is not None:
        max_steps = negatives._check_count(max_steps, "max_steps", 1, 1 << 62)
    if trainer == "device" and (dim % 4 or dim > skipgram.MAX_DIM):
        raise ValueError(f'trainer="device" needs dim % 4 == 0 and dim <= {skipgram.MAX_DIM}; got {dim}')
    dev, adj, _, _ = sources.resolve(source, test_set, torch.empty(0), who="node2vec_embeddings", host_ok=True)
    if trainer == "device" and dev is None:
        raise ValueError('trainer="device" needs a source on a GPU; a host graph.CSR without one trains with "torch"')
    where = torch.device("cpu") if dev is None else dev
    n = int(adj.n)
    if n <= 0:
        return torch.zeros((0, dim), dtype=torch.float32, device=where), []
    gen = torch.Generator(device=where)
    gen.manual_seed(seed & ((1 << 63) - 1))
    table = torch.randn((n, dim), generator=gen, device=where, dtype=torch.float32)
    if trainer == "device":
        return _train_on_device(table, adj, gen, L=L, context=context, r=r, num_neg=num_neg, epochs=epochs,
                                chunk=chunk, lr=lr, p=p, q=q, seed=seed, max_tries=max_tries, max_steps=max_steps)
    emb = torch.nn.Embedding(n, dim, sparse=True, _weight=table)
    opt = torch.optim.SparseAdam(list(emb.parameters()), lr=lr)
    # a host source without a GPU walks through the restatement; with one, `adj` is the resident device copy
    walk_source = source if dev is None else adj
    per_epoch = n * r
    losses, done = [], 0
    for epoch in range(epochs):
        order = torch.randperm(n, generator=gen, device=where).repeat(r)
        total = torch.zeros((), dtype=torch.float32, device=where)
        steps = 0
        for lo, m in sources.chunks(per_epoch, chunk):
            start = order[lo:lo + m]
            walks = random_walks(walk_source, start, length=L, p=p, q=q, seed=seed, max_tries=max_tries,
                                 walk_base=epoch * per_epoch + lo).walks
            pos = _windows(walks, context).reshape(-1, context).to(torch.int64)
            noise = torch.randint(n, (m * num_neg, L), generator=gen, device=where)
            neg = _windows(torch.cat([start.repeat(num_neg)[:, None], noise], dim=1), context).reshape(-1, context)
            opt.zero_grad()
            loss = _skipgram_loss(emb, pos, neg)
            loss.backward()
            opt.step()
            total += loss.detach()
            steps += 1
            done += 1
            if done == max_steps:
                break
        losses.append(float(total) / steps)
        if done == max_steps:
            break
    return emb.weight.detach(), losses


def _train_on_device(table, adj, gen, *, L, context, r, num_neg, epochs, chunk, lr, p, q, seed, max_tries, max_steps):
    """``node2vec_embeddings``' loop with ``skipgram.skipgram_step`` as the step: the same draws from ``gen`` in the
    same order as the torch trainer.  The walks are handed over as the kernel's step-major buffer (the base of the
    transposed view, no copy); the negative walks are written step-major as well: the starts, then the noise."""
    dev, n = table.device, int(adj.n)
    state = skipgram.skipgram_state(table)
    per_epoch = n * r
    losses, done = [], 0
    for epoch in range(epochs):
        order = torch.randperm(n, generator=gen, device=dev).repeat(r)
        total = torch.zeros((), dtype=torch.float64, device=dev)
        steps = 0
        for lo, m in sources.chunks(per_epoch, chunk):
            start = order[lo:lo + m]
            walks = random_walks(adj, start, length=L, p=p, q=q, seed=seed, max_tries=max_tries,
                                 walk_base=epoch * per_epoch + lo).walks
            noise = torch.randint(n, (m * num_neg, L), generator=gen, device=dev)
            neg = torch.empty((L + 1, m * num_neg), dtype=torch.int32, device=dev)
            neg[0] = start.repeat(num_neg)
            neg[1:] = noise.t()
            total += skipgram.skipgram_step(table, state, walks.t(), neg, context, lr=lr)
            steps += 1
            done += 1
            if done == max_steps:
                break
        losses.append(float(total) / steps)                        # the one read per epoch
        if done == max_steps:
            break
    return table, losses
