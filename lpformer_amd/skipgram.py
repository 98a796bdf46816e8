"""Node2Vec's skip-gram update with negative sampling as one device step.

    skipgram_state(table)                                         SkipGramState(exp_avg, exp_avg_sq, step): zeros, 0
    skipgram_step(table, state, pos, neg, context, lr=...)        one step on the device: the loss, a 0-d fp64 tensor
    skipgram_reference(table, state, pos, neg, context, lr=...)   the same step in fp64 torch on the CPU, no autograd

The mathematics is what ``node2vec_embeddings(trainer="torch")`` does: PyG's ``Node2Vec.loss`` and
``torch.optim.SparseAdam``.  Only the evaluation differs: no ``[windows, context, dim]`` block, no float atomics, one
fixed summation order, so a step is a pure function of its inputs and two runs give the same bits.

Contract (shared by the kernels in csrc/skipgram.hip and ``skipgram_reference``).  The step is synchronous: every
gradient is taken at the table as it stands when the step begins.  ``pos`` and ``neg`` are STEP-MAJOR walk buffers,
int32 ``[L + 1, W]`` with row stride ``ld >= W`` (what ``lpf_random_walks`` writes: the base of ``random_walks``'
transposed view), holding Wp and Wn walks; neither is unfolded in memory.

* A walk has ``nwin = L + 2 - context`` windows; window (w, o) gives the pairs (c, x) = (walk[o][w], walk[o + k][w]),
  k = 1 .. context - 1; pair id = ``(w nwin + o)(context - 1) + (k - 1)``, the negative buffer's ids following the
  positive buffer's.
* logit l = <E[c], E[x]>, s = sigmoid(l).  A positive pair adds ``-log(s + 1e-15) / Mp`` to the loss, a negative pair
  ``-log((1 - s) + 1e-15) / Mn``; ``Mp = Wp nwin (context - 1)`` and Mn come from the shapes, so nothing is read back.
  The coefficient of a pair is g = dloss/dl: ``-s (1 - s) / (s + 1e-15) / Mp`` and ``s (1 - s) / ((1 - s) + 1e-15) / Mn``.
* A pair that holds an id outside [0, n) has coefficient 0 and loss 0 but still counts in Mp or Mn.  This differs from
  ``random_walks.walk_pairs``, which DROPS every window that holds a -1, so that its mean runs over fewer pairs;
  ``node2vec_embeddings`` never produces such a pair.
* A pair with c == x (a walk back at its start, an isolated node) is an ordinary pair: both of its occurrences land on
  the same row.
* The gradient of row r is the sum over its occurrences of g[pair] E[other]: pair i gives the occurrences (c_i, x_i, i)
  with id i and (x_i, c_i, i) with id M + i, a row's occurrences are taken by ascending id, cut into chunks of
  ``CHUNK`` (``LPF_SKIPGRAM_CHUNK``), each chunk summed from zero in order and the chunks added in order.
* ``SparseAdam`` as torch has it: only the touched rows change ``exp_avg``, ``exp_avg_sq`` and the table, one global
  step count gives the bias corrections, ``denom = sqrt(v) + eps``.

On the device the logit is an fp32 sum in one order; sigmoid, quotient and logarithm are fp64 from that logit and the
coefficient is rounded to fp32 once; the loss is fp64 throughout.  The occurrence list is built with torch (a stable
sort of the 2 M row keys, ``unique_consecutive``, a cumulative sum): plumbing, and the one place a step waits for the
device (``unique_consecutive`` sizes its result).  Ill-conditioning that belongs to the loss as PyG writes it, not to
the kernels: ``(1 - s) + 1e-15`` loses its digits once l passes about 25 (1 - s nears the spacing of doubles at 1).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple

import torch

from . import _lib, negatives, ops
from ._lib import check, ptr

MAX_DIM = _lib.CONST["LPF_SKIPGRAM_MAX_DIM"]
CHUNK = _lib.CONST["LPF_SKIPGRAM_CHUNK"]
BLOCK_WINDOWS = _lib.CONST["LPF_SKIPGRAM_BLOCK_WINDOWS"]
_EPS = 1e-15                           # PyG's Node2Vec.loss
_MAX = (1 << 31) - 2


@dataclass
class SkipGramState:
    """SparseAdam's state of one table: ``exp_avg`` and ``exp_avg_sq`` like the table, ``step`` the steps taken."""
    exp_avg: torch.Tensor
    exp_avg_sq: torch.Tensor
    step: int = 0


class SkipGramReference(NamedTuple):
    loss: torch.Tensor                 # 0-d fp64
    coef: torch.Tensor                 # fp64 [M]: dloss/dlogit per pair, 0 for a bad pair
    centre: torch.Tensor               # int64 [M]; -1 for a bad pair
    other: torch.Tensor                # int64 [M]; -1 for a bad pair
    rows: torch.Tensor                 # int64 [U]: the touched rows, ascending
    grad: torch.Tensor                 # fp64 [U, dim]
    table: torch.Tensor                # fp64 [n, dim]: the table after the step
    exp_avg: torch.Tensor              # fp64 [n, dim]
    exp_avg_sq: torch.Tensor           # fp64 [n, dim]
    step: int


def skipgram_state(table: torch.Tensor) -> SkipGramState:
    """The state before the first step: zeros like ``table``, step 0."""
    return SkipGramState(torch.zeros_like(table), torch.zeros_like(table), 0)


# ------------------------------------------------------------------------------------------------------------ checks
def _check_options(lr, betas, eps):
    lr, eps = float(lr), float(eps)
    b1, b2 = (float(b) for b in betas)
    if not (lr >= 0.0 and eps >= 0.0 and 0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(f"skipgram: lr and eps must be >= 0 and the betas in [0, 1); got {lr}, {(b1, b2)}, {eps}")
    return lr, b1, b2, eps


def _check_buffer(buf, name):
    if not (isinstance(buf, torch.Tensor) and buf.dim() == 2 and buf.dtype == torch.int32):
        raise ValueError(f"skipgram: {name} must be a step-major int32 tensor [L + 1, W]")
    if buf.shape[1] > 1 and buf.stride(1) != 1 or buf.shape[0] > 1 and buf.stride(0) < buf.shape[1]:
        raise ValueError(f"skipgram: {name} must have unit stride along the walks and a row stride >= W "
                         "(the base of random_walks' transposed view, not the view)")


def _check_shapes(table, pos, neg, context):
    if not (isinstance(table, torch.Tensor) and table.dim() == 2):
        raise ValueError("skipgram: table must be a tensor [n, dim]")
    _check_buffer(pos, "pos")
    _check_buffer(neg, "neg")
    if pos.shape[0] != neg.shape[0] or pos.shape[0] < 2:
        raise ValueError("skipgram: pos and neg must hold the same number of positions, at least two")
    L = int(pos.shape[0]) - 1
    context = negatives._check_count(context, "context", 2, L + 1)
    nwin = L + 2 - context
    Mp, Mn = (int(b.shape[1]) * nwin * (context - 1) for b in (pos, neg))
    if Mp + Mn > _MAX:
        raise ValueError("skipgram: a step holds fewer than 2^31 - 1 pairs")
    return L, context, nwin, Mp, Mn


def _ld(buf) -> int:
    return int(buf.stride(0)) if buf.shape[0] > 1 else int(buf.shape[1])


# ------------------------------------------------------------------------------------------------- host restatement
def _pairs(buf: torch.Tensor, context: int):
    """(centre, other) int64 [W nwin (context - 1)] of one step-major buffer, in pair-id order."""
    win = buf.to(torch.int64).t().unfold(1, context, 1)            # [W, nwin, context]
    centre = win[:, :, :1].expand(-1, -1, context - 1)
    return centre.reshape(-1), win[:, :, 1:].reshape(-1)


@torch.no_grad()
def skipgram_reference(table, state: SkipGramState, pos, neg, context, *, lr=0.01, betas=(0.9, 0.999), eps=1e-8,
                       chunk: int = CHUNK) -> SkipGramReference:
    """``skipgram_step`` in fp64 torch on the CPU, written out from the module docstring's contract with no autograd;
    ``table`` and ``state`` are left as they are.  ``chunk``: the occurrences per chunk of a row's sum (in fp64 it
    moves the last bits only)."""
    lr, b1, b2, eps = _check_options(lr, betas, eps)
    pos, neg = pos.cpu(), neg.cpu()
    L, context, nwin, Mp, Mn = _check_shapes(table, pos, neg, context)
    E = table.detach().cpu().to(torch.float64)
    n, dim = E.shape
    cp, xp = _pairs(pos, context)
    cn, xn = _pairs(neg, context)
    c, x = torch.cat([cp, cn]), torch.cat([xp, xn])
    M = Mp + Mn
    ok = (c >= 0) & (c < n) & (x >= 0) & (x < n)
    cs, xs = torch.where(ok, c, 0), torch.where(ok, x, 0)           # nothing is indexed with a bad id
    logit = (E[cs] * E[xs]).sum(dim=1) if n else torch.zeros(M, dtype=torch.float64)
    s = torch.sigmoid(logit)
    om = 1.0 - s
    isneg = torch.arange(M) >= Mp
    f64 = lambda v: torch.tensor(v, dtype=torch.float64)
    scale = torch.where(isneg, f64(1.0 / max(Mn, 1)), f64(1.0 / max(Mp, 1)))
    coef = torch.where(isneg, s * om / (om + _EPS), -(s * om) / (s + _EPS)) * scale
    coef = torch.where(ok, coef, 0.0)
    loss = (torch.where(ok, -torch.log(torch.where(isneg, om, s) + _EPS), 0.0) * scale).sum()
    # occurrences: (c_i, x_i, i) with id i, (x_i, c_i, i) with id M + i; by row, then by id
    keys = torch.cat([torch.where(ok, c, -1), torch.where(ok, x, -1)])
    order = torch.sort(keys, stable=True).indices
    order = order[keys[order] >= 0]
    row_of = keys[order]
    other = torch.cat([xs, cs])[order]
    contrib = coef.repeat(2)[order, None] * E[other] if n else torch.zeros((0, dim), dtype=torch.float64)
    rows, counts = torch.unique_consecutive(row_of, return_counts=True)
    grad = _segment_sums(contrib, counts, int(chunk))
    # SparseAdam
    step = int(state.step) + 1
    m = state.exp_avg.detach().cpu().to(torch.float64).clone()
    v = state.exp_avg_sq.detach().cpu().to(torch.float64).clone()
    new = E.clone()
    m[rows] = m[rows] + (grad - m[rows]) * (1.0 - b1)
    v[rows] = v[rows] + (grad * grad - v[rows]) * (1.0 - b2)
    step_size = lr * (1.0 - b2 ** step) ** 0.5 / (1.0 - b1 ** step)
    new[rows] = new[rows] - step_size * (m[rows] / (v[rows].sqrt() + eps))
    return SkipGramReference(loss, coef, torch.where(ok, c, -1), torch.where(ok, x, -1), rows, grad, new, m, v, step)


def _segment_sums(contrib: torch.Tensor, counts: torch.Tensor, chunk: int) -> torch.Tensor:
    """[U, dim]: per segment of ``counts`` consecutive rows of ``contrib``, chunks of ``chunk`` rows summed from zero
    in order, the chunks' sums added in order (``index_add_`` on the CPU adds in index order)."""
    U, dim = counts.numel(), contrib.shape[1]
    start = torch.cumsum(counts, 0) - counts
    seg = torch.repeat_interleave(torch.arange(U), counts)
    within = torch.arange(contrib.shape[0]) - start[seg]
    nchunk = (counts + chunk - 1) // chunk
    first = torch.cumsum(nchunk, 0) - nchunk
    part = torch.zeros((int(nchunk.sum()), dim), dtype=contrib.dtype)
    part.index_add_(0, first[seg] + within // chunk, contrib)
    out = torch.zeros((U, dim), dtype=contrib.dtype)
    out.index_add_(0, torch.repeat_interleave(torch.arange(U), nchunk), part)
    return out


# ------------------------------------------------------------------------------------------------------ device path
def _check_table(t, name, n, dim, dev):
    if not (isinstance(t, torch.Tensor) and t.dim() == 2 and t.dtype == torch.float32 and t.device == dev
            and tuple(t.shape) == (n, dim)):
        raise ValueError(f"skipgram: {name} must be a float32 tensor [{n}, {dim}] on {dev}")
    if n and (t.stride(1) != 1 and dim > 1 or t.stride(0) % 4 or t.stride(0) < dim or t.data_ptr() % 16):
        raise ValueError(f"skipgram: {name} needs unit stride along dim, a row stride that is a multiple of 4 floats "
                         "and a 16-byte aligned base")


def occurrence_list(keys: torch.Tensor):
    """``(rows int32 [U], seg int64 [U + 1], occ_other int32 [2 M], occ_pair int32 [2 M])`` from ``keys`` int32 [2 M],
    the pairs' ids as ``lpf_skipgram_coef_f32`` wrote them (centres in the first half, others in the second): a stable
    sort of the 2 M row keys, so a row's occurrences keep their ids' order.  Bad pairs (-1, -1) make up a leading
    segment of row -1, which the kernels skip.  Plain torch; ``unique_consecutive`` waits for the device."""
    M = keys.numel() // 2
    skeys, perm = torch.sort(keys, stable=True)
    rows, counts = torch.unique_consecutive(skeys, return_counts=True)
    seg = torch.zeros(rows.numel() + 1, dtype=torch.int64, device=keys.device)
    torch.cumsum(counts, 0, out=seg[1:])
    occ_other = keys[torch.where(perm < M, perm + M, perm - M)]
    occ_pair = torch.where(perm < M, perm, perm - M).to(torch.int32)
    return rows, seg, occ_other, occ_pair


@torch.no_grad()
def skipgram_step(table: torch.Tensor, state: SkipGramState, pos: torch.Tensor, neg: torch.Tensor, context: int, *,
                  lr=0.01, betas=(0.9, 0.999), eps=1e-8) -> torch.Tensor:
    """One skip-gram step by the module docstring's contract, on the device: ``table`` (float32 [n, dim],
    ``dim % 4 == 0``, ``dim <= 512``) and ``state`` are updated in place, the loss comes back as a 0-d fp64 tensor on
    the device; no value is read back.  ``pos``, ``neg``: step-major int32 walk buffers [L + 1, W] with row stride
    >= W -- hand in the base of ``random_walks(...).walks.t()``, not a copy.  A pure function of its inputs: two runs
    from equal copies give the same bits."""
    lr, b1, b2, eps = _check_options(lr, betas, eps)
    L, context, nwin, Mp, Mn = _check_shapes(table, pos, neg, context)
    dev = table.device
    if dev.type != "cuda" or pos.device != dev or neg.device != dev:
        raise ValueError("skipgram_step runs on the device: table, pos and neg must be on one GPU")
    n, dim = (int(s) for s in table.shape)
    if dim % 4 or not 4 <= dim <= MAX_DIM:
        raise ValueError(f"skipgram_step needs dim % 4 == 0 and 4 <= dim <= {MAX_DIM}; got {dim}")
    _check_table(table, "table", n, dim, dev)
    _check_table(state.exp_avg, "state.exp_avg", n, dim, dev)
    _check_table(state.exp_avg_sq, "state.exp_avg_sq", n, dim, dev)
    if state.exp_avg.stride(0) != state.exp_avg_sq.stride(0):
        raise ValueError("skipgram: state.exp_avg and state.exp_avg_sq must share their row stride")
    M = Mp + Mn
    hip = _lib.hip()
    with torch.cuda.device(dev):
        loss = torch.zeros((), dtype=torch.float64, device=dev)
        if M == 0:
            return loss
        stream = ops.raw_stream(dev)
        coef = torch.empty(M, dtype=torch.float32, device=dev)
        ids = torch.empty(2 * M, dtype=torch.int32, device=dev)
        windows = (int(pos.shape[1]) + int(neg.shape[1])) * nwin
        partial = torch.empty(-(-windows // BLOCK_WINDOWS), dtype=torch.float64, device=dev)
        check(hip.lpf_skipgram_coef_f32(n, dim, ptr(table), table.stride(0), L, context, ptr(pos), pos.shape[1],
                                        _ld(pos), ptr(neg), neg.shape[1], _ld(neg), ptr(coef), ptr(ids[:M]),
                                        ptr(ids[M:]), ptr(partial), partial.numel(), ptr(loss), stream),
              "lpf_skipgram_coef_f32")
        rows, seg, occ_other, occ_pair = occurrence_list(ids)
        U = rows.numel()
        grad = torch.empty((U, dim), dtype=torch.float32, device=dev)
        scratch = torch.empty((-(-2 * M // CHUNK), dim), dtype=torch.float32, device=dev)
        check(hip.lpf_skipgram_grad_rows_f32(n, dim, ptr(table), table.stride(0), M, ptr(coef), 2 * M, ptr(occ_other),
                                             ptr(occ_pair), U, ptr(seg), ptr(grad), dim, ptr(scratch),
                                             scratch.shape[0], 0, stream), "lpf_skipgram_grad_rows_f32")
        step = int(state.step) + 1
        check(hip.lpf_sparse_adam_rows_f32(n, dim, ptr(table), table.stride(0), ptr(state.exp_avg),
                                           ptr(state.exp_avg_sq), state.exp_avg.stride(0), U, ptr(rows), ptr(grad),
                                           dim, lr, b1, b2, eps, step, 1.0 - b1 ** step, 1.0 - b2 ** step, stream),
              "lpf_sparse_adam_rows_f32")
        state.step = step
    return loss
