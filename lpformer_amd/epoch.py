"""The training EPOCH: exact per-batch edge masks made on the device, ``train_epoch`` and a thin ``fit``.

The reference's loop (src/train/train_model.py:23-83) removes the ROWS of ``train_pos`` a batch holds and builds the
typing adjacency of the batch from the rows that are left (:40-45).  An undirected edge is therefore absent from that
adjacency iff EVERY row holding it -- as (u, v) or (v, u), any number of times -- is in the batch: ogbl-collab repeats a
pair once per year, and a list may hold a pair in both directions.  ``RemovedEdges(edges)`` removes each named edge
unconditionally and so differs from the reference exactly on such rows.  Here

    te = TrainEdges(train_pos, num_nodes)     rows grouped by their undirected edge, once per dataset
    te.covered(perm)                          [2, B]: (min, max) of the rows whose edge the batch removes, else (-1, -1)
    te.mask(perm)                             RemovedEdges(te.covered(perm)): the reference's mask, as a difference
    train_epoch(model, score_func, data, optimizer, ...)      the loop itself;  fit(...): epochs, evaluation, early stop

``covered`` runs ``lpf_batch_cover`` (csrc/batch_cover.hip) on device tensors -- three small launches, no read-back, a
fixed output shape -- and the torch restatement inside the same method on CPU tensors; both are integer arithmetic and
agree position by position.
"""
from __future__ import annotations

import copy
from typing import Callable, Optional

import torch

from . import _lib, evaluate, graph, ops
from ._lib import check, ptr

_CACHE_KEY = "_lpf_train_edges"          # data[...] = (the train_pos object it was built from, TrainEdges)
_UNIT_KEY = "_lpf_adj_t_unit"            # data[...] = (the adj_t object, True / False)


class TrainEdges:
    """The rows of ``train_pos`` [E, 2] grouped by the undirected edge they hold.

    key[e] = min(u, v) * n + max(u, v) (a self-loop row is a group like any other); ``gkey`` int64 [G] the distinct keys
    in ascending order, ``gid`` int32 [E] the group of each row, ``mult`` int32 [G] the rows per group, ``cnt`` int32 [G]
    the counters of ``covered`` -- all zero between calls.  Built with torch ops on ``device`` (default: where
    ``train_pos`` lives), once: a sort and a read-back.

    ``cnt`` and the statistics belong to the object: use one ``TrainEdges`` from one stream at a time."""

    def __init__(self, train_pos, num_nodes: int, device=None):
        tp = torch.as_tensor(train_pos)
        if tp.dim() != 2 or tp.shape[1] != 2:
            raise ValueError(f"train_pos must be [E, 2], got {tuple(tp.shape)}")
        if tp.dtype.is_floating_point or tp.dtype == torch.bool:
            raise ValueError("train_pos must hold integer node ids")
        dev = tp.device if device is None else torch.device(device)
        n = int(num_nodes)
        tp = tp.to(dev, dtype=torch.int64).contiguous()
        if tp.shape[0] >= 2 ** 31 - 1:
            raise ValueError("at most 2^31 - 2 rows")
        if tp.numel() and (int(tp.min()) < 0 or int(tp.max()) >= n):
            raise IndexError(f"train_pos holds node ids outside [0, {n})")
        self.train_pos, self.num_nodes, self.device = tp, n, dev
        lo, hi = torch.minimum(tp[:, 0], tp[:, 1]), torch.maximum(tp[:, 0], tp[:, 1])
        self.gkey, inv, counts = torch.unique(lo * n + hi, return_inverse=True, return_counts=True)
        self.gid = inv.to(torch.int32).contiguous()
        self.mult = counts.to(torch.int32).contiguous()
        self.cnt = torch.zeros(self.gkey.numel(), dtype=torch.int32, device=dev)
        self._stats = torch.zeros(4, dtype=torch.int32, device=dev)
        self._checked = []               # adjacency key tensors ``check_against`` has accepted

    @property
    def num_rows(self) -> int:
        return int(self.train_pos.shape[0])

    @property
    def num_groups(self) -> int:
        return int(self.gkey.numel())

    def directed_keys(self) -> torch.Tensor:
        """Sorted, distinct int64 keys row * n + col of the symmetrised edges of ``train_pos``."""
        n = self.num_nodes
        lo = torch.div(self.gkey, n, rounding_mode="floor")
        hi = self.gkey - lo * n
        return torch.unique(torch.cat([self.gkey, hi * n + lo]))

    def check_against(self, model, test_set: bool = False) -> None:
        """Raise ``ValueError`` unless the symmetrised distinct pairs of ``train_pos`` are EXACTLY the model's resident
        typing adjacency (``data['adj_mask']``; ``test_set``: ``data['full_adj_mask']``).  The masks of ``mask`` are
        differences to that adjacency: they state the reference's per-batch adjacency only when the two agree.  The
        sorted keys are compared on the device, one read-back; an adjacency that passed is remembered."""
        own = model._own_mask_keys(test_set)
        if any(k is own for k in self._checked):
            return
        if int(model.num_nodes) != self.num_nodes:
            raise ValueError(f"train_pos was indexed for {self.num_nodes} nodes, the model has {int(model.num_nodes)}")
        mine = self.directed_keys().to(own.device)
        if mine.numel() != own.numel() or not bool((mine == own).all()):
            raise ValueError(
                f"the symmetrised pairs of train_pos ({mine.numel()} directed entries) are not the model's resident typing "
                f"adjacency ({own.numel()} entries): the per-batch masks of TrainEdges are differences to that adjacency. "
                "Build data['adj_mask'] from train_pos, or pass the masked tensor as adj_mask= yourself.")
        self._checked = (self._checked + [own])[-4:]

    def _perm(self, perm) -> torch.Tensor:
        p = torch.as_tensor(perm)
        if p.dtype.is_floating_point or p.dtype == torch.bool:
            raise ValueError("perm must hold integer row ids")
        return p.reshape(-1).to(self.device, dtype=torch.int64).contiguous()

    @torch.no_grad()
    def covered(self, perm) -> torch.Tensor:
        """int64 [2, len(perm)]: position i holds (min, max) of row ``perm[i]`` iff every row of ``train_pos`` with that
        undirected edge is in ``perm``, else (-1, -1).  ``perm``: DISTINCT row ids (a slice of a permutation); an id
        outside [0, E) gives (-1, -1), touches nothing and is counted (``stats``).  A group with several rows in the
        batch appears at each of them -- the consumer takes the unique set.  On the current stream, nothing read back."""
        p = self._perm(perm)
        B, E, G = p.numel(), self.num_rows, self.num_groups
        out = torch.empty(2, B, dtype=torch.int64, device=self.device)
        if B == 0:
            return out
        if self.device.type == "cuda":
            with torch.cuda.device(self.device):
                check(_lib.hip().lpf_batch_cover(ptr(self.gid), ptr(self.mult), ptr(self.train_pos), E, G, ptr(p), B,
                                                 ptr(self.cnt), ptr(out), ptr(self._stats),
                                                 ops.raw_stream(self.device)), "lpf_batch_cover")
            return out
        # the same three phases in torch (CPU tensors): count, emit, reset
        ok = (p >= 0) & (p < E)
        rows = p[ok]
        g = self.gid[rows].long()
        self.cnt.index_add_(0, g, torch.ones(g.numel(), dtype=torch.int32))
        full = self.cnt[g] == self.mult[g]
        emit = torch.zeros(B, dtype=torch.bool)
        emit[ok] = full
        out.fill_(-1)
        tp = self.train_pos[rows[full]]
        out[0, emit], out[1, emit] = tp.min(dim=1).values, tp.max(dim=1).values
        self.cnt[g] = 0
        n_emit, n_ok = int(emit.sum()), int(ok.sum())
        self._stats += torch.tensor([n_emit, n_ok - n_emit, B - n_ok, 0], dtype=torch.int32)
        return out

    def mask(self, perm) -> graph.RemovedEdges:
        """The reference's per-batch adjacency (train_model.py:40-45) as a difference to the resident one: usable as
        ``adj_mask=`` and, for an unweighted propagation matrix, as ``adj_prop=``."""
        return graph.RemovedEdges(self.covered(perm))

    def stats(self, check_range: bool = True) -> list:
        """``[emitted, held back, out of range, spare]`` positions, summed over every ``covered`` call since the object
        was built or ``reset_stats()``.  Synchronises (one read-back).  Raises ``IndexError`` when a ``perm`` held ids
        outside [0, E) (``check_range=False``: returns the words instead)."""
        words = [int(v) for v in self._stats.tolist()]
        if check_range and words[2] != 0:
            raise IndexError(f"{words[2]} row ids outside [0, {self.num_rows}) were passed to TrainEdges.covered")
        return words

    def reset_stats(self) -> None:
        self._stats.zero_()


# ------------------------------------------------------------------------------------------------------- the loop
def _device_of(model, fallback) -> torch.device:
    dev = getattr(model, "device", None)
    if dev is not None:
        return torch.device(dev)
    for p in model.parameters():
        return p.device
    return fallback


def _train_edges_of(data, dev) -> TrainEdges:
    hit = data.get(_CACHE_KEY)
    if hit is not None and hit[0] is data["train_pos"] and hit[1].device == dev:
        return hit[1]
    te = TrainEdges(data["train_pos"], int(data["num_nodes"]), device=dev)
    data[_CACHE_KEY] = (data["train_pos"], te)
    return te


def _require_unit_weights(data) -> None:
    """``mask_input=True`` states the reference's masked propagation matrix, which is UNWEIGHTED
    (train_model.py:51-52: ``SparseTensor.from_edge_index`` without values): a difference to a weighted ``adj_t`` would
    be another matrix."""
    adj_t = data["adj_t"]
    hit = data.get(_UNIT_KEY)
    if hit is None or hit[0] is not adj_t:
        val = adj_t.val if isinstance(adj_t, (graph.CSR, graph.DeviceCSR)) else graph.as_coo_numpy(adj_t)[2]
        unit = val is None or bool((torch.as_tensor(val) == 1).all())
        hit = data[_UNIT_KEY] = (adj_t, unit)
    if not hit[1]:
        raise ValueError("mask_input=True: data['adj_t'] carries non-unit weights, but the reference's masked propagation "
                         "matrix is unweighted (src/train/train_model.py:51-52).  Pass the masked tensor yourself: "
                         "model(edges, adj_prop=masked_adjt, adj_mask=...) takes it as the reference builds it.")


def train_epoch(model, score_func, data, optimizer, *, batch_size: int = 1024, num_negative: int = 1,
                mask_input: bool = False, clip: Optional[float] = 1.0, train_edges: Optional[TrainEdges] = None,
                generator: Optional[torch.Generator] = None, batches=None, negatives: Optional[Callable] = None,
                on_step: Optional[Callable] = None) -> float:
    """One epoch over ``data['train_pos']`` [E, 2] with the semantics of the reference's ``train_epoch``
    (src/train/train_model.py:23-83); returns the epoch loss ``sum(loss_i * B_i) / sum(B_i)``.

    Batches: slices of a device ``torch.randperm(E, generator=generator)``, the last one short; ``batches``: an explicit
    sequence of row-id tensors instead.  Positives: ``model(edges, adj_mask=te.mask(perm))`` -- the batch's rows removed
    from the typing adjacency exactly as the reference removes them, repeated pairs included -- and, with
    ``mask_input``, the same difference as ``adj_prop`` (raises ``ValueError`` for a weighted ``data['adj_t']``).
    Negatives: ``torch.randint(0, n, (2, B * num_negative))`` on the device, or ``negatives(step, edges)`` -> [2, K].
    Loss: ``-log(p + 1e-6).mean() - log(1 - q + 1e-6).mean()``; backward; ``clip_grad_norm_`` of both modules with
    ``clip`` (None: off); optimiser step; ``zero_grad``.  ``on_step(step, loss)`` receives the detached loss TENSOR of
    each step: the epoch itself reads the device once, at its end (the loss sum and ``te.stats()``).

    ``train_edges``: a ``TrainEdges`` of ``data['train_pos']``; None builds one and keeps it in ``data``.  Its pairs must
    be the model's typing adjacency (``check_against``, once)."""
    model.train()
    score_func.train()
    dev = _device_of(model, torch.as_tensor(data["train_pos"]).device)
    te = train_edges if train_edges is not None else _train_edges_of(data, dev)
    te.check_against(model, False)
    if mask_input:
        _require_unit_weights(data)
    n, E = int(data["num_nodes"]), te.num_rows
    explicit = batches is not None
    if not explicit:
        if int(batch_size) < 1:
            raise ValueError("batch_size must be positive")
        order = torch.randperm(E, generator=generator, device=te.device)
        batches = [order[lo:lo + int(batch_size)] for lo in range(0, E, int(batch_size))]
    total = torch.zeros((), dtype=torch.float64, device=dev)
    examples = 0
    for step, perm in enumerate(batches):
        perm = te._perm(perm)
        if perm.numel() == 0:
            continue
        # (a caller's row id outside [0, E) must not fault the gather: it reads a row in range, the mask skips and counts
        # it, and the epoch ends with IndexError)
        edges = te.train_pos[perm.clamp(0, max(E - 1, 0)) if explicit else perm].t()
        removed = te.mask(perm)
        h = model(edges, adj_prop=removed if mask_input else None, adj_mask=removed)
        pos_out = score_func(h)
        pos_loss = -torch.log(pos_out + 1e-6).mean()
        if negatives is not None:
            neg_edges = negatives(step, edges)
        else:
            neg_edges = torch.randint(0, n, (2, edges.shape[1] * int(num_negative)), dtype=torch.long, device=edges.device,
                                      generator=generator)
        neg_loss = -torch.log(1 - score_func(model(neg_edges)) + 1e-6).mean()
        loss = pos_loss + neg_loss
        loss.backward()
        if clip is not None:
            torch.nn.utils.clip_grad_norm_(model.parameters(), clip)
            torch.nn.utils.clip_grad_norm_(score_func.parameters(), clip)
        optimizer.step()
        optimizer.zero_grad()
        b = int(pos_out.shape[0])
        total += loss.detach().to(total.device, torch.float64) * b
        examples += b
        if on_step is not None:
            on_step(step, loss.detach())
    try:
        te.stats()                        # raises for row ids outside [0, E)
    except IndexError:
        te.reset_stats()
        raise
    return float(total) / examples if examples else float("nan")


def fit(model, score_func, data, optimizer, *, epochs: int, eval_steps: int = 5, metric: str = "Hits@100",
        k_list=(20, 50, 100), kill_cnt: int = 100, decay: float = 1.0, heart: bool = False,
        eval_batch_size: int = 32768, **epoch_kw) -> dict:
    """``train_loop`` of the reference (src/train/train_model.py:87-140) as glue: per epoch ``train_epoch(**epoch_kw)``;
    every ``eval_steps`` epochs ``evaluate.evaluate_model`` (``k_list``, ``heart``); the learning rate of epoch e is the
    optimiser's times ``decay ** (e - 1)`` (``LambdaLR``).  The run is judged by the VALIDATION entry of ``metric``
    (``results[metric][1]``): an evaluation that beats the best so far (which starts at 0) keeps a copy of both
    ``state_dict``s and clears the counter, any other raises it, and the run stops when the counter EXCEEDS
    ``kill_cnt`` -- the reference's count (:125-136): ``kill_cnt + 1`` evaluations in a row without improvement.

    Returns ``{"history": [{"epoch", "loss", "lr", "results" (evaluated epochs)}], "best_valid", "best_epoch",
    "model_state", "score_state" (None before the first improvement), "stopped_early"}``."""
    sched = torch.optim.lr_scheduler.LambdaLR(optimizer, lr_lambda=lambda e: float(decay) ** e)
    history = []
    best = {"best_valid": 0.0, "best_epoch": None, "model_state": None, "score_state": None, "stopped_early": False}
    stale = 0
    for epoch in range(1, int(epochs) + 1):
        lr = optimizer.param_groups[0]["lr"]
        entry = {"epoch": epoch, "loss": train_epoch(model, score_func, data, optimizer, **epoch_kw), "lr": lr}
        history.append(entry)
        if epoch % int(eval_steps) == 0:
            results = evaluate.evaluate_model(model, score_func, data, batch_size=eval_batch_size, k_list=tuple(k_list),
                                              heart=heart)
            if metric not in results:
                raise KeyError(f"metric {metric!r} is not among the evaluated ones: {sorted(results)}")
            entry["results"] = results
            valid = float(results[metric][1])
            if valid > best["best_valid"]:
                stale = 0
                best.update(best_valid=valid, best_epoch=epoch, model_state=copy.deepcopy(model.state_dict()),
                            score_state=copy.deepcopy(score_func.state_dict()))
            else:
                stale += 1
                if stale > int(kill_cnt):
                    best["stopped_early"] = True
                    break
        sched.step()
    return dict(best, history=history)
