"""Evaluation sweep over many candidate pairs: the reference's ``test_edge`` /
``test_heart_negatives`` / ``test_edge_citation2`` loops (src/train/testing.py:14-121) restructured for the device:

* the encoder runs ONCE per sweep (``test_edge`` re-runs it for every batch through ``model(edge)``,
  testing.py:87 -> link_transformer.py:100);
* batches are issued round-robin over a few HIP streams, so the selection kernels of one batch run underneath the
  matrix-core kernels of the previous one (per-stream workspaces in ``LinkTransformer``);
* a very long sweep (hundreds of batches: HeaRT / citation2 negatives) replays RECORDED steps
  (``lpformer_amd.PlannedScorer``, one per stream): ``score_pairs`` spends ~0.13 ms of host time per batch between its
  launches, more than the device needs at D = 64;
* scores stay on the device -- no ``.cpu()`` per batch (testing.py:88,117); the ranking metrics below
  (src/train/evaluation.py:23-50 and the OGB ``hits@K`` rule) are a few reductions over them.

The metric helpers are plain tensor reductions over at most a few million scores (host-layer plumbing, any device).
"""
from __future__ import annotations

from typing import Optional

import torch


def _as_2xp(edges: torch.Tensor) -> torch.Tensor:
    edges = torch.as_tensor(edges)
    if edges.dim() != 2 or 2 not in edges.shape:
        raise ValueError("edges must be [P, 2] (the reference's split layout) or [2, P]")
    return edges.t() if edges.shape[1] == 2 and edges.shape[0] != 2 else edges


# Full batches per stream from which recording the step pays.  Measured (tools/sweep_rate.py, 8 streams): recording the
# eight plans costs ~10 ms per sweep; a replayed batch saves 0.015 ms (collab-like: the device needs 0.19 of the 0.206 ms
# an eager batch takes), 0.04 ms (ppa-like), 0.08 ms (citation2-like) -- break-even at 700 / 260 / 130 batches.  Sweeps
# of that length are the HeaRT and citation2 negatives (testing.py:95-121), not the few batches of an ogbl-collab split.
PLAN_MIN_BATCHES = 64


def _planned_sweep(model, score_func, batch, out, h, batch_size, n_full, test_set, streams, logits) -> bool:
    """The first ``n_full`` full batches of a sweep through recorded steps, one ``PlannedScorer`` per stream.  Returns
    False (nothing written) when the step of this configuration cannot be recorded."""
    from .graphed import PlannedScorer
    nl = max(1, min(streams, n_full))
    main = torch.cuda.current_stream(model.device)
    lanes = model.lanes(nl)   # the model's persistent streams: every sweep finds the workspaces of the one before
    try:
        plans = [PlannedScorer(model, score_func, h, batch[:, k * batch_size:(k + 1) * batch_size], test_set=test_set,
                               logits=logits, adopt_input=True, stream=lanes[k]) for k in range(nl)]
    except RuntimeError:
        return False
    jobs = [[] for _ in plans]
    for p in plans:
        p.stream.wait_stream(main)   # h, batch and out are ready
    for i in range(n_full):
        lo, p = i * batch_size, plans[i % nl]
        jobs[i % nl].append(lo)
        res = p(batch[:, lo:lo + batch_size], validate=False, ordered=False)
        with torch.cuda.stream(p.stream):
            out[lo:lo + batch_size].copy_(res, non_blocking=True)
    # as below: one status read per stream at the end; a stream that reports an overflow scores its batches again, one at
    # a time with the status checked after each (check() re-records with a workspace sized for the offending batch)
    for p, lane_jobs in zip(plans, jobs):
        if p.check():
            continue
        for lo in lane_jobs:
            for _attempt in range(4):
                res = p(batch[:, lo:lo + batch_size], validate=False, ordered=False)
                with torch.cuda.stream(p.stream):
                    out[lo:lo + batch_size].copy_(res, non_blocking=True)
                if p.check():
                    break
            else:
                raise RuntimeError("score_edges: the selection workspace could not be sized")
    for p in plans:
        main.wait_stream(p.stream)
    return True


@torch.no_grad()
def score_edges(model, score_func, edges, batch_size: int = 32768, *, h: Optional[torch.Tensor] = None,
                test_set: bool = False, streams: int = 4, logits: bool = False, plans: Optional[bool] = None) -> torch.Tensor:
    """Probabilities (or pre-sigmoid logits) for every pair of ``edges``, as one device tensor of shape [P].

    Same arithmetic per pair as ``score_func(model(edge, test_set=test_set))`` of the reference loop; ``h`` (the encoder
    output, ``model.propagate(test_set=...)``) is computed once if not given.  ``plans``: replay recorded steps for the
    full batches (default: when the sweep has at least ``PLAN_MIN_BATCHES`` of them per stream); the scores are bitwise
    the ones of the eager loop."""
    dev = model.device
    batch = _as_2xp(edges).to(dev)
    if batch.dtype != torch.int64:
        batch = batch.long()
    batch = batch.contiguous()
    total = batch.shape[1]
    if h is None:
        h = model.propagate(test_set=test_set)
    out = torch.empty(total, dtype=torch.float32, device=dev)
    if total == 0:
        return out
    main = torch.cuda.current_stream(dev)
    start = 0
    n_full = total // batch_size
    if getattr(model, "_multi_head", False):
        # (num_heads > 1 / two attention layers: layer by layer, head by head through train.py's pair_stage -- no recorded
        #  plan exists for it, and its selection reads its status back per batch: one lane)
        plans, streams = False, 1
    if plans is None:
        plans = n_full >= PLAN_MIN_BATCHES * max(1, min(streams, n_full))
    if plans and n_full > 0 and _planned_sweep(model, score_func, batch, out, h, batch_size, n_full, test_set, streams,
                                               logits):
        start = n_full * batch_size
        if start == total:
            return out
    lanes = model.lanes(max(1, min(streams, (total - start + batch_size - 1) // batch_size)))  # persistent: workspaces are per stream
    for s in lanes:
        s.wait_stream(main)  # h, batch and out are ready
    jobs = [[] for _ in lanes]
    for i, lo in enumerate(range(start, total, batch_size)):
        hi = min(lo + batch_size, total)
        jobs[i % len(lanes)].append((lo, hi))
        with torch.cuda.stream(lanes[i % len(lanes)]):
            out[lo:hi] = model.score_pairs(batch[:, lo:hi], h, score_func, test_set=test_set, logits=logits)
    # The selection of a batch is sized from EARLIER batches of its lane and nothing is read back while the sweep is
    # queued: a batch that outgrows its workspace (hub-heavy negatives after a sparse start) comes back as NaN and
    # leaves a sticky status on the lane.  Read every lane's status once, at the end, and score the batches of a lane
    # that reports an overflow again, one at a time with the status checked after each (the first of them re-sizes
    # the workspace) -- never a NaN, or a silently wrong metric, out of this function.
    for lane, lane_jobs in zip(lanes, jobs):
        if model.check_selection(lane):
            continue
        with torch.cuda.stream(lane):
            for lo, hi in lane_jobs:
                for _attempt in range(4):
                    out[lo:hi] = model.score_pairs(batch[:, lo:hi], h, score_func, test_set=test_set, logits=logits)
                    if model.check_selection(lane):
                        break
                else:
                    raise RuntimeError("score_edges: the selection workspace could not be sized")
    for s in lanes:
        main.wait_stream(s)
    return out


@torch.no_grad()
def score_negatives(model, score_func, negatives, batch_size: int = 32768, **kw) -> torch.Tensor:
    """HeaRT-style negatives [P, K, 2] -> scores [P, K] (``test_heart_negatives``, testing.py:95-121)."""
    negatives = torch.as_tensor(negatives)
    p, k = negatives.shape[0], negatives.shape[1]
    return score_edges(model, score_func, negatives.reshape(-1, 2), batch_size, **kw).view(p, k)


def hits_at_k(pos: torch.Tensor, neg: torch.Tensor, k: int) -> float:
    """OGB ``hits@K`` (what ``evaluate_hits`` asks the ogb Evaluator for, evaluation.py:7-18): the fraction of
    positive scores strictly above the K-th largest negative score; 1.0 when there are fewer than K negatives."""
    pos, neg = pos.reshape(-1), neg.reshape(-1)
    if neg.numel() < k:
        return 1.0
    kth = torch.topk(neg, k).values[-1]
    return float((pos > kth).float().mean().item()) if pos.numel() else float("nan")


def ranking_metrics(pos: torch.Tensor, neg: torch.Tensor) -> dict:
    """``evaluate_mrr`` (evaluation.py:23-50): per positive, rank among its own K negatives as the mean of the
    optimistic and the pessimistic rank; MRR and Hits@{10,50,100} averaged over the positives.
    pos [P], neg [P, K]."""
    pos = pos.reshape(-1, 1)
    optimistic = (neg >= pos).sum(dim=1)
    pessimistic = (neg > pos).sum(dim=1)
    rank = 0.5 * (optimistic + pessimistic).to(torch.float32) + 1.0
    return {"Hits@10": float((rank <= 10).float().mean().item()), "Hits@50": float((rank <= 50).float().mean().item()),
            "Hits@100": float((rank <= 100).float().mean().item()), "MRR": float((1.0 / rank).mean().item())}


# Metrics by heuristic bin (src/train/eval.py:44-77 ``test_by_metric``, behind run.py's --bymetric / --percentile,
# src/run.py:195-196).  The reference's function is unfinished: its predictions are ``...`` placeholders (eval.py:64,66),
# and it overwrites its bin list with the per-edge counts (``cn_vals = compute_edge_cn(...)``, eval.py:68) before
# looping over ``cn_vals`` as bins.  What follows is the intended logic: the bins of eval.py:62, half-open [lo, hi)
# (eval.py:70), each bin's positives against ALL negatives with the OGB hits@K rule (eval.py:71-73).
CN_BINS = ((0, 1), (1, 3), (3, 10), (10, 1_000_000))


def metrics_by_bin(pos: torch.Tensor, neg: torch.Tensor, values: torch.Tensor, bins=CN_BINS,
                   k_list=(20, 50, 100)) -> list:
    """Ranking metrics of the positives split by a per-positive value (a pair heuristic: CN, AA, RA, PPR ...).

    pos [P] scores of the positives, values [P] the value each is binned by, bins a sequence of half-open [lo, hi).
    ``neg`` 1-D (the OGB Hits layout): every bin's positives against ALL negatives, ``Hits@K`` for K in ``k_list``
    (``hits_at_k``).  ``neg`` [P, K] (HeaRT / citation2: each positive's own negatives): ``ranking_metrics`` over the
    rows of the bin.  Returns one dict per bin: ``bin`` (lo, hi), ``count`` and the metrics -- NaN for an empty bin."""
    pos = torch.as_tensor(pos).reshape(-1)
    neg = torch.as_tensor(neg)
    values = torch.as_tensor(values).reshape(-1).to(pos.device)
    if values.numel() != pos.numel():
        raise ValueError(f"values has {values.numel()} entries, pos {pos.numel()}")
    per_row = neg.dim() == 2
    if per_row and neg.shape[0] != pos.numel():
        raise ValueError(f"neg [P, K] must have one row per positive ({pos.numel()}), got {tuple(neg.shape)}")
    if neg.dim() > 2:
        raise ValueError("neg must be 1-D (shared negatives) or [P, K] (per-positive negatives)")
    neg = neg.to(pos.device)
    keys = ("Hits@10", "Hits@50", "Hits@100", "MRR") if per_row else tuple(f"Hits@{k}" for k in k_list)
    out = []
    for lo, hi in bins:
        m = (values >= lo) & (values < hi)
        count = int(m.sum().item())
        res = {"bin": (lo, hi), "count": count}
        if count == 0:
            res.update({k: float("nan") for k in keys})
        elif per_row:
            res.update(ranking_metrics(pos[m], neg[m]))
        else:
            res.update({f"Hits@{k}": hits_at_k(pos[m], neg, k) for k in k_list})
        out.append(res)
    return out


def quantile_bins(values: torch.Tensor, qs=(0.25, 0.5, 0.75)) -> tuple:
    """Bins for ``metrics_by_bin`` cut at quantiles of the positives' own values (the --percentile style of split,
    run.py:196): edges e_i = quantile(values, q_i) (linear interpolation, torch.quantile), bins
    (-inf, e_1), [e_1, e_2), ..., [e_k, inf).  Repeated edges give empty bins (NaN metrics), not merged ones."""
    v = torch.as_tensor(values).reshape(-1).to(torch.float64)
    if v.numel() == 0:
        raise ValueError("quantile_bins needs at least one value")
    q = torch.as_tensor(list(qs), dtype=torch.float64)
    if q.numel() and (bool((q < 0).any()) or bool((q > 1).any()) or bool((q[1:] < q[:-1]).any())):
        raise ValueError("qs must be ascending and lie in [0, 1]")
    edges = [float("-inf")] + [float(e) for e in torch.quantile(v.cpu(), q)] + [float("inf")]
    return tuple((edges[i], edges[i + 1]) for i in range(len(edges) - 1))


def recommendation_metrics(rec, sources, held_out, ks=(10, 20, 50, 100)) -> dict:
    """Mean recall@k and hit-rate@k of top-K recommendations (``lpformer_amd.recommend``) against held-out links.

    ``rec``: a ``Recommendations`` (or anything with ``ids`` int [S, K], best first, -1 padding); ``sources`` [S] the
    source of each row; ``held_out`` [P, 2] directed edges (u, v), duplicates counted once.  For a row whose source has
    T >= 1 held-out targets: recall@k = |top-k ids that are targets| / T (an id repeated in a row counts once),
    hit@k = 1 if any of them is a target.  Both are averaged over those rows only; rows without targets are left out.
    A k above K uses all K columns.  Returns ``{"recall@k": ..., "hit@k": ..., "n_sources": rows counted}`` (NaN
    metrics when no row has a target).  Pure torch, on the device of ``rec.ids``."""
    ids = torch.as_tensor(getattr(rec, "ids", rec))
    dev = ids.device
    ids = ids.to(torch.int64)
    src = torch.as_tensor(sources).to(dev, torch.int64).reshape(-1)
    ho = torch.as_tensor(held_out).to(dev, torch.int64)
    if ids.dim() != 2 or ids.shape[0] != src.numel():
        raise ValueError("rec.ids must be [S, K] with one row per source")
    if ho.dim() != 2 or ho.shape[1] != 2:
        raise ValueError("held_out must be [P, 2] directed edges")
    S, K = ids.shape
    parts = [src, ids.reshape(-1), ho.reshape(-1)]
    N = int(max(int(t.max()) for t in parts if t.numel()) + 1) if any(t.numel() for t in parts) else 1
    N = max(N, 1)
    keys = torch.unique(ho[:, 0] * N + ho[:, 1]) if ho.numel() else torch.empty(0, dtype=torch.int64, device=dev)
    n_t = torch.searchsorted(keys, src * N + N) - torch.searchsorted(keys, src * N)
    # first occurrence of each id in its row: a stable sort puts repeats after the first
    srt, order = torch.sort(ids, dim=1, stable=True)
    first_sorted = torch.ones_like(srt, dtype=torch.bool)
    first_sorted[:, 1:] = srt[:, 1:] != srt[:, :-1]
    first = torch.empty_like(first_sorted).scatter_(1, order, first_sorted)
    q = src[:, None] * N + ids.clamp_min(0)
    pos = torch.searchsorted(keys, q.reshape(-1)).reshape(S, K).clamp_max(max(keys.numel() - 1, 0))
    hit = (ids >= 0) & first & (keys.numel() > 0) & (keys[pos] == q if keys.numel() else torch.zeros_like(first))
    rows = n_t > 0
    n_rows = int(rows.sum())
    out = {}
    for k in ks:
        kk = min(int(k), K)
        h = hit[:, :kk].sum(dim=1).to(torch.float64)
        if n_rows == 0:
            out[f"recall@{k}"] = out[f"hit@{k}"] = float("nan")
            continue
        out[f"recall@{k}"] = float((h[rows] / n_t[rows].to(torch.float64)).mean())
        out[f"hit@{k}"] = float((h[rows] > 0).to(torch.float64).mean())
    out["n_sources"] = n_rows
    return out
