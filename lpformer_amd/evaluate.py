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

from .ops import raw_stream
from .sources import as_pairs


def _as_2xp(edges) -> torch.Tensor:
    return as_pairs(edges, exc=None)        # score_edges takes ids of any dtype, as it always has


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


# ------------------------------------------------------------------------------------------------ rank counts
# Everything below follows from two integers per positive: ge = #{negatives >= it} and gt = #{negatives > it}
# (DESIGN 5.12).  Tensors on a GPU go through lpf_rank_rows_f32 / lpf_rank_shared_f32 (csrc/rank_metrics.hip); tensors
# on the CPU through the torch restatement in the same functions.  Comparisons are IEEE on both paths: a NaN negative
# is never counted, a NaN positive gets ge = gt = 0, -0.0 == +0.0, +-inf are ordinary values.
INT32_MAX = 2 ** 31 - 1


def _scores(t, what: str) -> torch.Tensor:
    t = torch.as_tensor(t)
    if not t.is_floating_point():
        raise TypeError(f"{what} must be floating-point scores, got {t.dtype}")
    return t if t.dtype == torch.float32 else t.to(torch.float32)


class SortedNegatives:
    """One shared set of negatives, sorted once (``sort_negatives``): rank any number of positive sets against it.
    On a GPU ``keys`` are the ordered uint32 keys lpf_rank_shared_f32 left (stored as int32); on the CPU the sorted
    scores without their NaNs.  ``numel`` counts every negative, NaNs included."""

    def __init__(self, keys: torch.Tensor, numel: int):
        self.keys, self.numel = keys, int(numel)

    @property
    def device(self):
        return self.keys.device


def _shared_call(pos: torch.Tensor, neg: Optional[torch.Tensor], keys: torch.Tensor, m: int):
    """lpf_rank_shared_f32 on the current stream of the tensors' device.  ``neg`` None: ``keys`` are already sorted."""
    from . import _lib
    dev = keys.device
    p = pos.numel()
    ge = torch.empty(p, dtype=torch.int32, device=dev)
    gt = torch.empty(p, dtype=torch.int32, device=dev)
    nan = torch.empty(2, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        hip = _lib.hip()
        ws, nbytes = None, 0
        if neg is not None and m > 0:
            nbytes = int(hip.lpf_rank_shared_workspace_bytes(p, m))
            if nbytes <= 0:
                raise _lib.LpfError("lpf_rank_shared_workspace_bytes: no size for this many negatives")
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.check(hip.lpf_rank_shared_f32(p, _lib.ptr(pos), m, _lib.ptr(neg) if m > 0 else None, _lib.ptr(keys),
                                           _lib.ptr(ws), nbytes, _lib.ptr(ge), _lib.ptr(gt), _lib.ptr(nan),
                                           raw_stream(dev)), "lpf_rank_shared_f32")
    return ge, gt, nan


def sort_negatives(neg) -> SortedNegatives:
    """Sort one shared set of negatives (any shape, flattened) for ``rank_counts`` / ``ranks`` / ``link_metrics``."""
    if isinstance(neg, SortedNegatives):
        return neg
    neg = _scores(neg, "neg").reshape(-1).contiguous()
    m = neg.numel()
    if m > INT32_MAX:
        raise ValueError(f"at most 2^31 - 1 shared negatives, got {m}")
    if not neg.is_cuda:
        return SortedNegatives(torch.sort(neg[~torch.isnan(neg)]).values, m)
    keys = torch.empty(m, dtype=torch.int32, device=neg.device)
    _shared_call(torch.empty(0, dtype=torch.float32, device=neg.device), neg, keys, m)
    return SortedNegatives(keys, m)


def _counts_shared(pos: torch.Tensor, sn: SortedNegatives):
    """(ge, gt int32 [P], nan int64 [2]: NaNs among the positives and among the negatives) on the device of pos."""
    if sn.device != pos.device:
        raise ValueError(f"pos is on {pos.device}, the negatives on {sn.device}")
    if pos.is_cuda:
        return _shared_call(pos, None, sn.keys, sn.numel)
    srt = sn.keys
    mv = srt.numel()
    bad = torch.isnan(pos)
    q = torch.where(bad, torch.zeros_like(pos), pos)
    ge = mv - torch.searchsorted(srt, q, right=False)
    gt = mv - torch.searchsorted(srt, q, right=True)
    ge, gt = ge.masked_fill(bad, 0).to(torch.int32), gt.masked_fill(bad, 0).to(torch.int32)
    return ge, gt, torch.stack([bad.sum(), torch.as_tensor(sn.numel - mv)]).to(torch.int64)


def _counts_rows(pos: torch.Tensor, neg: torch.Tensor):
    p, k = neg.shape
    if not pos.is_cuda:
        col = pos.reshape(-1, 1)
        ge = (neg >= col).sum(dim=1).to(torch.int32)
        gt = (neg > col).sum(dim=1).to(torch.int32)
        return ge, gt, torch.stack([torch.isnan(pos).sum(), torch.isnan(neg).sum()]).to(torch.int64)
    from . import _lib
    if p > INT32_MAX - 1 or k > INT32_MAX - 1:
        raise ValueError("at most 2^31 - 2 rows and columns")
    if k > 1 and neg.stride(1) != 1:
        neg = neg.contiguous()
    ld = neg.stride(0) if p > 1 else k          # (a row stride of a view is used as it is: no copy)
    if ld < 0:
        neg, ld = neg.contiguous(), k
    dev = pos.device
    ge = torch.empty(p, dtype=torch.int32, device=dev)
    gt = torch.empty(p, dtype=torch.int32, device=dev)
    nan = torch.empty(2, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.hip().lpf_rank_rows_f32(p, k, _lib.ptr(pos), _lib.ptr(neg) if k > 0 else None, ld, _lib.ptr(ge),
                                                _lib.ptr(gt), _lib.ptr(nan), raw_stream(dev)), "lpf_rank_rows_f32")
    return ge, gt, nan


def _prepare(pos, neg):
    """(pos float32 [P] contiguous, rows [P, K] or None, SortedNegatives or None) after the shape checks."""
    pos = _scores(pos, "pos").reshape(-1).contiguous()
    if isinstance(neg, SortedNegatives):
        if neg.device != pos.device:
            raise ValueError(f"pos is on {pos.device}, the negatives on {neg.device}")
        return pos, None, neg
    neg = _scores(neg, "neg")
    if neg.device != pos.device:
        raise ValueError(f"pos is on {pos.device}, neg on {neg.device}")
    if neg.dim() == 1:
        return pos, None, sort_negatives(neg)
    if neg.dim() != 2:
        raise ValueError("neg must be 1-D (shared negatives) or [P, K] (per-positive negatives)")
    if neg.shape[0] != pos.numel():
        raise ValueError(f"neg [P, K] must have one row per positive ({pos.numel()}), got {tuple(neg.shape)}")
    return pos, neg, None


def _counts(pos, neg):
    pos, rows, sn = _prepare(pos, neg)
    return _counts_rows(pos, rows) if rows is not None else _counts_shared(pos, sn)


def rank_counts(pos, neg):
    """``(ge, gt)`` int32 [P]: per positive the number of negatives ``>=`` it and ``>`` it.  ``neg`` 1-D (or a
    ``SortedNegatives``): one shared set, sorted once, two bound searches per positive -- the [P, M] comparison the
    reference builds with ``neg.repeat(P, 1)`` (evaluation.py:121-125) never exists.  ``neg`` [P, K]: each positive
    against its own row, one pass over the negatives."""
    ge, gt, _ = _counts(pos, neg)
    return ge, gt


def _rank_f32(ge: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    return 0.5 * (ge.to(torch.int64) + gt).to(torch.float32) + 1.0   # ranking_metrics' expression


def ranks(pos, neg) -> torch.Tensor:
    """``get_ranking_list`` (evaluation.py:74-90): the mean of the optimistic and the pessimistic rank,
    ``0.5 * (ge + gt) + 1`` as float32 [P]; shared negatives need no ``repeat``."""
    ge, gt, _ = _counts(pos, neg)
    return _rank_f32(ge, gt)


def sample_hits(pos, neg, ks=(20, 50, 100)) -> dict:
    """``sample_level_hits`` (evaluation.py:53-71): ``{"Hits@K": float32 [P] of 0/1}``, 1 where the rank is <= K."""
    rank = ranks(pos, neg)
    return {f"Hits@{k}": (rank <= k).to(torch.float32) for k in ks}


def _check_ks(k_list):
    ks = [int(k) for k in k_list]
    if any(k < 1 for k in ks):
        raise ValueError(f"every K must be >= 1, got {list(k_list)}")
    return ks


def _link_metrics(pos, rows, sn, ks, mrr, auc, accumulate) -> dict:
    if accumulate not in (torch.float64, torch.float32):
        raise ValueError("accumulate must be torch.float64 or torch.float32")
    p = pos.numel()
    ge, gt, nan = _counts_rows(pos, rows) if rows is not None else _counts_shared(pos, sn)
    per_row = rows is not None
    m = rows.shape[1] if per_row else sn.numel
    rank32 = _rank_f32(ge, gt)
    # Hits: the OGB rule for one shared set (ge < K  <=>  pos > K-th largest negative; all ones when M < K), the
    # reference's rank <= K for per-row negatives (evaluate_mrr)
    hit = [(rank32 <= k) if per_row else (ge < k) for k in ks]
    ints = [h.sum() for h in hit] + [nan[0], nan[1]]
    flts = []
    f32 = accumulate == torch.float32
    if f32:       # the reference's own reductions: float32 means (evaluate_mrr / hits_at_k to the bit on one device)
        flts += [h.float().mean().double() if p else torch.full((), float("nan"), dtype=torch.float64, device=pos.device)
                 for h in hit]
    if mrr:
        if f32:
            flts.append((1.0 / rank32).mean().double())
        else:
            rank64 = 0.5 * (ge.to(torch.int64) + gt).to(torch.float64) + 1.0   # exact: half-integers below 2^32
            flts.append((1.0 / rank64).sum())
    m_all = 0
    if auc:
        if per_row:   # over the flattened negatives: every positive against all P * K of them
            if rows.numel() > INT32_MAX:
                raise ValueError("AUC / AP over [P, K] negatives need P * K <= 2^31 - 1")
            sn = sn if sn is not None else sort_negatives(rows)
            ge_a, gt_a, _ = _counts_shared(pos, sn)
        else:
            ge_a, gt_a = ge, gt
        m_all = sn.numel
        # twice the AUC numerator, an exact integer: sum_i 2 (M - ge_i) + (ge_i - gt_i)
        ints.append((2 * m_all - ge_a.to(torch.int64) - gt_a).sum())
        tp, _, _ = _counts_shared(pos, sort_negatives(pos))          # tp_i = #{positives >= pos_i}
        den = (tp.to(torch.int64) + ge_a).to(torch.float64)
        flts.append(torch.where(den > 0, tp.to(torch.float64) / den.clamp_min(1.0), torch.zeros_like(den)).sum())
    ints = [int(v) for v in torch.stack([torch.as_tensor(v, device=pos.device).to(torch.int64) for v in ints]).tolist()]
    flts = [float(v) for v in torch.stack(flts).tolist()] if flts else []
    out = {}
    nanv = float("nan")
    for i, k in enumerate(ks):
        if not per_row and m < k:
            out[f"Hits@{k}"] = 1.0
        elif f32:
            out[f"Hits@{k}"] = flts[i]
        else:
            out[f"Hits@{k}"] = ints[i] / p if p else nanv
    j = len(ks) if f32 else 0
    if mrr:
        out["MRR"] = (flts[j] if f32 else (flts[j] / p if p else nanv))
        j += 1
    if auc:
        num2 = ints[len(ks) + 2]
        out["AUC"] = num2 / (2 * p * m_all) if p and m_all else nanv
        out["AP"] = flts[j] / p if p else nanv
    out["nan_pos"], out["nan_neg"] = ints[len(ks)], ints[len(ks) + 1]
    return out


def link_metrics(pos, neg, k_list=(20, 50, 100), mrr: bool = True, auc: bool = True,
                 accumulate: torch.dtype = torch.float64) -> dict:
    """Ranking metrics of positives against negatives from the two count vectors of ``rank_counts``.

    ``neg`` 1-D or a ``SortedNegatives`` (one shared set, the OGB layout): ``Hits@K = mean(ge < K)``, which is
    ``mean(pos > K-th largest negative)`` and 1.0 when M < K (``hits_at_k``).  ``neg`` [P, K] (HeaRT / citation2):
    ``Hits@K = mean(rank <= K)`` (``evaluate_mrr``).  ``MRR = mean(1 / rank)``, rank = 0.5 (ge + gt) + 1.
    ``AUC = sum_i ((M - ge_i) + 0.5 (ge_i - gt_i)) / (P M)`` from an exact int64 numerator, and
    ``AP = mean_i tp_i / (tp_i + ge_i)`` with tp_i = #{positives >= pos_i}: sklearn's ``roc_auc_score`` and
    ``average_precision_score`` on the concatenated labels (``evaluate_auc``, evaluation.py:93-104, unrounded); for
    [P, K] they are taken over the flattened negatives.  ``nan_pos`` / ``nan_neg`` count the NaN scores seen (an
    overflowed selection batch scores NaN): a NaN negative ranks below everything, a NaN positive has rank 1 and
    contributes 0 to AP.  ``accumulate``: float64 (default) sums counts as integers and reciprocal ranks in fp64;
    float32 takes the float32 means the reference and ``ranking_metrics`` / ``hits_at_k`` take, to the bit."""
    ks = _check_ks(k_list)
    pos, rows, sn = _prepare(pos, neg)
    return _link_metrics(pos, rows, sn, ks, mrr, auc, accumulate)


def split_metrics(pos_train, pos_valid, neg_valid, pos_test, neg_test, k_list=(100,), layout: str = "shared",
                  mrr: bool = True, auc: bool = True) -> dict:
    """``get_metric_score`` / ``get_metric_score_citation2`` (evaluation.py:108-148):
    ``{"Hits@K": (train, valid, test), "MRR": (...), "AUC": (...), "AP": (...), "nan_pos": (...), "nan_neg": (...)}``.
    Train positives are ranked against the VALID negatives, as the reference does.  ``layout="shared"``: the negatives
    of a split are one set (flattened), sorted once for the train and the valid positives.  ``layout="rows"``:
    ``neg_*`` [P, K], each positive against its own row (the train positives against the rows of the valid negatives,
    so there must be as many of them)."""
    if layout not in ("shared", "rows"):
        raise ValueError("layout must be 'shared' or 'rows'")
    ks = _check_ks(k_list)
    if layout == "shared":
        nv = sort_negatives(_scores(neg_valid, "neg_valid").reshape(-1))
        nt = sort_negatives(_scores(neg_test, "neg_test").reshape(-1))
        parts = [_link_metrics(*_prepare(p, n), ks, mrr, auc, torch.float64)
                 for p, n in ((pos_train, nv), (pos_valid, nv), (pos_test, nt))]
    else:
        parts = []
        flat = {}
        for p, n in ((pos_train, neg_valid), (pos_valid, neg_valid), (pos_test, neg_test)):
            pos, rows, _ = _prepare(p, n)
            if rows is None:
                raise ValueError("layout='rows' needs [P, K] negatives")
            if auc and id(n) not in flat:       # the flattened negatives of a split are sorted once as well
                flat[id(n)] = sort_negatives(rows)
            parts.append(_link_metrics(pos, rows, flat.get(id(n)), ks, mrr, auc, torch.float64))
    return {key: tuple(part[key] for part in parts) for key in parts[0]}


def target_negatives(pos, neg) -> torch.Tensor:
    """ogbl-citation2's negatives -- K candidate TARGETS per positive, ``neg`` [P, K] -- as the [P, K, 2] pairs
    (source of positive p, neg[p, k]) that ``test_edge_citation2`` scores (testing.py:21-27).  ``pos`` [P, 2]."""
    pos, neg = torch.as_tensor(pos), torch.as_tensor(neg)
    if pos.dim() != 2 or pos.shape[1] != 2 or neg.dim() != 2 or neg.shape[0] != pos.shape[0]:
        raise ValueError(f"target-only negatives need pos [P, 2] and neg [P, K], got {tuple(pos.shape)} and {tuple(neg.shape)}")
    return torch.stack((pos[:, :1].to(neg.device).expand_as(neg), neg), dim=-1)


def _target_only(data, heart: bool) -> bool:
    """Whether ``data`` takes the reference's ``test_citation2`` path (train_model.py:114-117: a citation dataset without
    ``--heart``): its negatives are target ids [P, K], not pairs.  Decided by ``data['dataset']``, as the reference
    decides by ``args.data_name``; a dict without that key holds [M, 2] shared pairs."""
    return (not heart) and "citation" in str(data.get("dataset", "")).lower()


def _negatives_layout(data, heart: bool) -> str:
    """``split_metrics``' layout for the negatives of ``data``: "rows" (per positive) or "shared"."""
    return "rows" if (heart or _target_only(data, heart)) else "shared"


@torch.no_grad()
def score_splits(model, score_func, data, batch_size: int = 32768, heart: bool = False, logits: bool = False) -> dict:
    """Scores of the five splits ``test()`` / ``test_citation2()`` score (testing.py:50-74, :124-161), on the device:
    ``{"train_pos_val", "valid_pos", "test_pos": [P], "valid_neg", "test_neg": [M] shared or [P, K] per positive}``.
    One encoder pass per graph; ``test_pos`` and ``test_neg`` on the test-time graph (``test_set=True``: encoder,
    typing adjacency and PPR matrix).  Negatives: [M, 2] shared ones; with ``heart`` [P, K, 2] per positive; for
    ogbl-citation2 without ``heart`` (``data['dataset']`` names it, as the reference's dispatch does) [P, K] target ids,
    paired with the source of their positive (``target_negatives``).

    Deliberately NOT the reference where it contradicts itself: ``test_heart_negatives`` encodes with
    ``model.propagate()`` -- the TRAINING graph -- even for the test negatives (testing.py:105, under a "TODO"), while it
    types and weighs them on the test graph and scores the test positives entirely on the test graph.  The two differ
    when ``use_val_in_test`` and ``heart`` are both on; here the test negatives see the same graph as the positives they
    are ranked against.  The reference's scores are ``score_negatives(..., h=model.propagate(test_set=False),
    test_set=True)``."""
    model.eval()
    score_func.eval()
    kw = dict(logits=logits)
    h = model.propagate(test_set=False)
    h_test = model.propagate(test_set=True)
    out = {"train_pos_val": score_edges(model, score_func, data["train_pos_val"], batch_size, h=h, **kw),
           "valid_pos": score_edges(model, score_func, data["valid_pos"], batch_size, h=h, **kw),
           "test_pos": score_edges(model, score_func, data["test_pos"], batch_size, h=h_test, test_set=True, **kw)}
    neg_valid, neg_test = data["valid_neg"], data["test_neg"]
    if _target_only(data, heart):
        neg_valid = target_negatives(data["valid_pos"], neg_valid)
        neg_test = target_negatives(data["test_pos"], neg_test)
    if _negatives_layout(data, heart) == "rows":
        out["valid_neg"] = score_negatives(model, score_func, neg_valid, batch_size, h=h, **kw)
        out["test_neg"] = score_negatives(model, score_func, neg_test, batch_size, h=h_test, test_set=True, **kw)
    else:
        out["valid_neg"] = score_edges(model, score_func, neg_valid, batch_size, h=h, **kw)
        out["test_neg"] = score_edges(model, score_func, neg_test, batch_size, h=h_test, test_set=True, **kw)
    return out


@torch.no_grad()
def evaluate_model(model, score_func, data, batch_size: int = 32768, k_list=(100,), heart: bool = False) -> dict:
    """The reference's ``test()`` / ``test_citation2()`` (testing.py:50-74, :124-161): the scores of ``score_splits``,
    still on the device, handed to ``split_metrics``.  ``heart``: ``valid_neg`` / ``test_neg`` are [P, K, 2] per-positive
    negatives (the citation2 metrics); ogbl-citation2 without ``heart``: [P, K] target ids, the same metrics; otherwise
    [M, 2] shared ones.

    Two deliberate differences to the reference, both pinned by tests/test_gpu_pipeline.py: HeaRT test negatives are
    encoded on the test-time graph (see ``score_splits``), and the train column of ogbl-citation2 is computed from the
    ``train_pos_val`` scores -- ``test_citation2`` scores them and then reports the VALIDATION positives in their place
    (``pos_train_pred = pos_valid_pred.view(-1)``, testing.py:70), so its train column repeats its valid column."""
    s = score_splits(model, score_func, data, batch_size, heart=heart)
    return split_metrics(s["train_pos_val"], s["valid_pos"], s["valid_neg"], s["test_pos"], s["test_neg"], k_list=k_list,
                         layout=_negatives_layout(data, heart))


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
    rows of the bin.  Returns one dict per bin: ``bin`` (lo, hi), ``count`` and the metrics -- NaN for an empty bin.

    Any per-positive value works, e.g. the hop distance of the endpoints:
    ``metrics_by_bin(pos, neg, pair_distance(model, pos_edges), bins=distance.DIST_BINS)``."""
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
