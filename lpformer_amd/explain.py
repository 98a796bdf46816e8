"""Why a pair got its score: per-pair attribution of the attention.

LPFormer's attention adapts per pair between common neighbours, one-hop nodes and >1-hop PPR nodes.  The reference
hands its weights out as ``[2, nnz]`` = (pair position, alpha) (src/modules/layers.py:73-75) -- no node ids, no types,
one batch per call.  Here the same softmax (PyG segment softmax over the pair's three types jointly, layers.py:220) is
reduced on the device to what explains a pair:

    explain(model, edges, top=8)    top nodes with their weights, types and PPR values, attention mass per type,
                                    entropy, counts; optionally the whole pair-major list and the logits
    explain_from_scores(...)        the reduction alone, from the exported selection layout and one score per entry
    pairs_of(sources, rec)          the pairs of a ``recommend`` result, to explain them
    attention_profile(expl, ...)    which type the model attends to, by bin of a pair heuristic (the paper's analysis)

Tensors on a GPU go through ``lpf_pair_explain_f32`` (csrc/explain.hip); tensors on the CPU through the torch
restatement in the same function, the pattern of ``evaluate.rank_counts``.  Both accumulate their sums in float64 and
round once; exp, the division and log are float32.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch

from .evaluate import CN_BINS
from .ops import f32_rows, raw_stream
from .sources import as_pairs, node_ids

MAX_TOP = 32
TYPE_NAMES = ("padding", "cn", "1-hop", ">1-hop")     # values of ``types``


class Reduction(NamedTuple):
    """What ``explain_from_scores`` returns (the per-pair part of an ``Explanation``)."""
    nodes: torch.Tensor      # int64 [P, top]: node ids, largest weight first; -1 padding
    weights: torch.Tensor    # float32 [P, top]: alpha; 0 padding
    types: torch.Tensor      # int8 [P, top]: 1 CN, 2 one-hop, 3 >1-hop; 0 padding
    ppr_a: torch.Tensor      # float32 [P, top]: the PPR values the positional encoding saw; 0 padding
    ppr_b: torch.Tensor
    mass: torch.Tensor       # float32 [P, 3]: sum of alpha per type
    entropy: torch.Tensor    # float32 [P]: -sum alpha ln alpha (nats)
    all: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]]   # (ptr, node, type, weight) or None


class Explanation(NamedTuple):
    nodes: torch.Tensor
    weights: torch.Tensor
    types: torch.Tensor
    ppr_a: torch.Tensor
    ppr_b: torch.Tensor
    counts: torch.Tensor     # int32 [P, 3]: selected nodes per type
    mass: torch.Tensor
    entropy: torch.Tensor
    scores: Optional[torch.Tensor]   # the ``score_pairs`` logits [P] when a score head was given
    all: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]]


def _check_top(top) -> int:
    if isinstance(top, bool) or int(top) != top or not 1 <= int(top) <= MAX_TOP:
        raise ValueError(f"top must be an integer in [1, {MAX_TOP}], got {top!r}")
    return int(top)


def _reduce_torch(tp, node, pa, pb, score, top: int, want_all: bool) -> Reduction:
    """The reduction in plain torch (any device; the CPU path of ``explain_from_scores``)."""
    dev = score.device
    bs = tp.shape[1] - 1
    cnt = tp[:, 1:] - tp[:, :-1]                                        # [3, bs]
    tot = [int(v) for v in tp[:, bs].tolist()]
    n_ent = sum(tot)
    ar = torch.arange(bs, device=dev)
    pair = torch.cat([torch.repeat_interleave(ar, cnt[t]) for t in range(3)])
    typ = torch.cat([torch.full((tot[t],), t + 1, dtype=torch.int8, device=dev) for t in range(3)])
    node, pa, pb, score = node[:n_ent].to(torch.int64), pa[:n_ent], pb[:n_ent], score[:n_ent]
    all_ptr = torch.zeros(bs + 1, dtype=torch.int64, device=dev)
    torch.cumsum(cnt.sum(dim=0), dim=0, out=all_ptr[1:])
    # PyG segment softmax (layers.py:220): shift by the pair's maximum, denominator + 1e-16
    m = torch.full((bs,), float("-inf"), dtype=torch.float32, device=dev)
    m = m.scatter_reduce(0, pair, score, "amax", include_self=True)
    e = torch.exp(score - m[pair])
    den = torch.zeros(bs, dtype=torch.float64, device=dev).index_add_(0, pair, e.double()).float() + 1e-16
    alpha = e / den[pair]
    mass = torch.zeros(bs * 3, dtype=torch.float64, device=dev)
    mass.index_add_(0, pair * 3 + (typ.long() - 1), alpha.double())
    term = torch.where(alpha == 0, torch.zeros_like(alpha), alpha * torch.log(alpha))
    ent = 0.0 - torch.zeros(bs, dtype=torch.float64, device=dev).index_add_(0, pair, term.double())
    # order inside a pair: alpha descending (NaN last), then node ascending -- three stable sorts, last key first
    order = torch.sort(node, stable=True).indices
    a_key = torch.where(torch.isnan(alpha), torch.full_like(alpha, -1.0), alpha)
    order = order[torch.sort(a_key[order], descending=True, stable=True).indices]
    order = order[torch.sort(pair[order], stable=True).indices]
    p_srt = pair[order]
    rank = torch.arange(n_ent, device=dev) - all_ptr[p_srt]
    keep = rank < top
    src, row, col = order[keep], p_srt[keep], rank[keep]
    nodes = torch.full((bs, top), -1, dtype=torch.int64, device=dev)
    weights = torch.zeros(bs, top, dtype=torch.float32, device=dev)
    types = torch.zeros(bs, top, dtype=torch.int8, device=dev)
    ppr_a = torch.zeros(bs, top, dtype=torch.float32, device=dev)
    ppr_b = torch.zeros(bs, top, dtype=torch.float32, device=dev)
    nodes[row, col], weights[row, col], types[row, col] = node[src], alpha[src], typ[src]
    ppr_a[row, col], ppr_b[row, col] = pa[src], pb[src]
    full = None
    if want_all:
        perm = torch.sort(pair, stable=True).indices     # type-major -> pair-major, the type order kept inside a pair
        full = (all_ptr, node[perm], typ[perm], alpha[perm])
    return Reduction(nodes, weights, types, ppr_a, ppr_b, mass.float().view(bs, 3), ent.float(), full)


def _reduce_device(tp, node, pa, pb, score, top: int, want_all: bool, max_entries: int) -> Reduction:
    """``lpf_pair_explain_f32`` on the current stream of the tensors' device; nothing is read back unless the pair-major
    list is wanted (its length sizes the returned views)."""
    from . import _lib
    dev = score.device
    bs = tp.shape[1] - 1
    f32 = dict(dtype=torch.float32, device=dev)
    nodes = torch.empty(bs, top, dtype=torch.int64, device=dev)
    weights, ppr_a, ppr_b = (torch.empty(bs, top, **f32) for _ in range(3))
    types = torch.empty(bs, top, dtype=torch.int8, device=dev)
    mass, ent = torch.empty(bs, 3, **f32), torch.empty(bs, **f32)
    all_ptr = all_node = all_type = all_w = None
    if want_all:
        all_ptr = torch.empty(bs + 1, dtype=torch.int64, device=dev)
        all_node = torch.empty(max_entries, dtype=torch.int64, device=dev)
        all_type = torch.empty(max_entries, dtype=torch.int8, device=dev)
        all_w = torch.empty(max_entries, **f32)
    heavy = torch.empty(bs + 1, dtype=torch.int32, device=dev)
    if node.dtype != torch.int32:
        node = node.to(torch.int32)
    p = _lib.ptr
    with torch.cuda.device(dev):
        _lib.check(_lib.hip().lpf_pair_explain_f32(
            bs, p(tp), p(node), p(pa), p(pb), p(score), max_entries, top, p(mass), p(ent), p(nodes), p(weights),
            p(types), p(ppr_a), p(ppr_b), p(all_ptr), p(all_node), p(all_type), p(all_w), p(heavy), raw_stream(dev)),
            "lpf_pair_explain_f32")
    full = None
    if want_all:
        n_ent = min(int(all_ptr[bs].item()), max_entries)
        full = (all_ptr, all_node[:n_ent], all_type[:n_ent], all_w[:n_ent])
    return Reduction(nodes, weights, types, ppr_a, ppr_b, mass, ent, full)


@torch.no_grad()
def explain_from_scores(type_ptr, node, pa, pb, score, top: int, want_all: bool = False) -> Reduction:
    """The reduction alone.  Input is the layout ``lpf_select_export`` leaves and ``lpf_pair_scores_f32`` reads:
    ``type_ptr`` int64 [3, P + 1] (or flat), segment pointers relative per type; ``node``, ``pa``, ``pb``, ``score``
    one value per entry -- all CN entries sorted by (pair, node), then all one-hop, then all >1-hop.

    Per pair, over its up to three segments jointly: the PyG segment softmax (shift by the maximum, denominator + 1e-16),
    ``mass`` per type, ``entropy`` = -sum alpha ln alpha in nats (alpha = 0 adds 0; an empty pair has mass 0 and entropy
    0), and the ``top`` entries by alpha descending -- ties to the smaller node id, a NaN alpha last, padding -1 / 0.
    ``want_all``: also ``all`` = (ptr int64 [P + 1], node int64, type int8, weight), pair-major, a pair's entries in CN,
    one-hop, >1-hop order and sorted by node inside each.  Tensors on a GPU go through ``lpf_pair_explain_f32``."""
    top = _check_top(top)
    score = torch.as_tensor(score)
    dev = score.device
    tp = torch.as_tensor(type_ptr).to(dev, torch.int64)
    if tp.dim() == 1:
        if tp.numel() % 3 or tp.numel() < 3:
            raise ValueError("type_ptr must hold 3 * (P + 1) segment pointers")
        tp = tp.view(3, -1)
    if tp.dim() != 2 or tp.shape[0] != 3 or tp.shape[1] < 1:
        raise ValueError("type_ptr must be [3, P + 1]")
    tp = tp.contiguous()
    node = torch.as_tensor(node).to(dev).reshape(-1)
    node = node_ids(node, "node")
    pa, pb, score = (torch.as_tensor(t).to(dev, torch.float32).reshape(-1).contiguous() for t in (pa, pb, score))
    n_have = min(node.numel(), pa.numel(), pb.numel(), score.numel())
    if n_have >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 entries")
    if not score.is_cuda:
        if bool((tp[:, 0] != 0).any()) or bool((tp[:, 1:] < tp[:, :-1]).any()) or int(tp[:, -1].sum()) > n_have:
            raise ValueError("type_ptr must start at 0, ascend and stay within the entry arrays")
        return _reduce_torch(tp, node, pa, pb, score, top, want_all)
    node = node.to(torch.int32).contiguous()
    return _reduce_device(tp, node, pa, pb, score, top, want_all, n_have)


@torch.no_grad()
def explain(model, edges, top: int = 8, *, test_set: bool = False, adj_mask=None, score_func=None,
            weights: str = "top", batch_size: int = 32768, h: Optional[torch.Tensor] = None) -> Explanation:
    """Explain the attention of every pair of ``edges`` ([P, 2] or [2, P]).

    Runs the selection in the reference layout and ``lpf_pair_scores_f32`` -- the front part of
    ``calc_pairwise(..., return_weights=True)`` -- then one ``lpf_pair_explain_f32`` launch per chunk of ``batch_size``
    pairs; results are concatenated on the device.  ``nodes`` / ``weights`` / ``types`` / ``ppr_a`` / ``ppr_b`` [P, top]
    as in ``explain_from_scores``; ``counts`` int32 [P, 3] the selected nodes per type; ``scores`` the
    ``score_pairs(..., logits=True)`` logits when ``score_func`` is given; ``weights="all"`` also returns the pair-major
    list ``all`` = (ptr, node, type, weight): ``return_weights`` with the node ids it lacks.  ``h``: the encoder output
    (``model.propagate(test_set=...)``), computed once when not given.

    Evaluation mode only; multi-head and two-layer models raise ``NotImplementedError`` like ``return_weights``."""
    from . import _lib
    top = _check_top(top)
    if weights not in ("top", "all"):
        raise ValueError("weights must be 'top' or 'all'")
    if int(batch_size) < 1:
        raise ValueError("batch_size must be positive")
    batch = as_pairs(edges, exc=TypeError)
    n = int(model.num_nodes)
    if batch.numel() and (int(batch.min()) < 0 or int(batch.max()) >= n):
        raise IndexError(f"explain: edges hold node ids outside [0, {n})")
    model._check_supported()       # eval mode, one layer, one head
    dev = model.device
    if dev.type != "cuda":
        raise _lib.LpfError("explain: the model must live on an MI355X; lpformer_amd has no CPU fallback")
    want_all = weights == "all"
    total = batch.shape[1]
    with torch.cuda.device(dev):
        batch = batch.to(dev, torch.int64).contiguous()
        if h is None and total:
            h = model.propagate(test_set=test_set)
        parts, counts, scores, lists = [], [], [], []
        base = 0
        for lo in range(0, total, int(batch_size)):
            b = model._prep_batch(batch[:, lo:lo + int(batch_size)])
            bs = b.shape[1]
            s, score, _, _ = model._pair_scores(b, f32_rows(h), test_set, adj_mask)
            tp = s["type_ptr"][:3 * (bs + 1)].view(3, bs + 1)
            cap = min(s["cap"], s["sel_node"].numel(), s["sel_pa"].numel(), s["sel_pb"].numel(), score.numel())
            red = _reduce_device(tp, s["sel_node"], s["sel_pa"], s["sel_pb"], score, top, want_all, cap)
            parts.append(red)
            counts.append((tp[:, 1:] - tp[:, :-1]).t().to(torch.int32))
            if want_all:
                ptr, nd, ty, w = red.all
                lists.append((ptr[1:] + base, nd, ty, w))
                base += int(nd.numel())
            if score_func is not None:
                for _attempt in range(4):
                    lg = model.score_pairs(b, h, score_func, test_set=test_set, adj_mask=adj_mask, logits=True)
                    if model.check_selection():
                        break
                else:
                    raise _lib.LpfError("explain: the selection workspace could not be sized")
                scores.append(lg)
        if not parts:
            z32 = dict(dtype=torch.float32, device=dev)
            full = None
            if want_all:
                full = (torch.zeros(1, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int64, device=dev),
                        torch.empty(0, dtype=torch.int8, device=dev), torch.empty(0, **z32))
            return Explanation(torch.empty(0, top, dtype=torch.int64, device=dev), torch.empty(0, top, **z32),
                               torch.empty(0, top, dtype=torch.int8, device=dev), torch.empty(0, top, **z32),
                               torch.empty(0, top, **z32), torch.empty(0, 3, dtype=torch.int32, device=dev),
                               torch.empty(0, 3, **z32), torch.empty(0, **z32),
                               torch.empty(0, **z32) if score_func is not None else None, full)
        cat = lambda name: torch.cat([getattr(r, name) for r in parts])   # noqa: E731
        full = None
        if want_all:
            full = (torch.cat([torch.zeros(1, dtype=torch.int64, device=dev)] + [l[0] for l in lists]),
                    torch.cat([l[1] for l in lists]), torch.cat([l[2] for l in lists]),
                    torch.cat([l[3] for l in lists]))
        return Explanation(cat("nodes"), cat("weights"), cat("types"), cat("ppr_a"), cat("ppr_b"), torch.cat(counts),
                           cat("mass"), cat("entropy"), torch.cat(scores) if score_func is not None else None, full)


def pairs_of(sources, rec):
    """The pairs of a ``recommend`` call: ``sources`` [S] as given to it, ``rec`` its ``Recommendations``.  Returns
    ``(edges int64 [2, sum(counts)], row, col)``: pair j is (sources[row[j]], rec.ids[row[j], col[j]]), rows in order and
    best first inside a row -- ``explain(model, pairs_of(sources, rec)[0])`` explains the recommendations."""
    ids = torch.as_tensor(rec.ids)
    dev = ids.device
    src = torch.as_tensor(sources).to(dev, torch.int64).reshape(-1)
    cnt = torch.as_tensor(rec.counts).to(dev, torch.int64).reshape(-1)
    if ids.dim() != 2 or ids.shape[0] != src.numel() or cnt.numel() != src.numel():
        raise ValueError("rec.ids must be [S, K] and rec.counts [S], one row per source")
    keep = torch.arange(ids.shape[1], device=dev)[None, :] < cnt[:, None]
    row, col = torch.nonzero(keep, as_tuple=True)
    return torch.stack([src[row], ids[row, col].to(torch.int64)]), row, col


def attention_profile(expl, values=None, bins=None) -> list:
    """Which type the model attends to, by bin of a per-pair value (a pair heuristic such as the CN count): one dict per
    half-open bin [lo, hi) -- the bins of ``evaluate.metrics_by_bin``, ``CN_BINS`` by default; with ``values=None`` one
    row over all pairs (``bin`` None).  Fields: ``bin``, ``count``, ``mass_cn`` / ``mass_1hop`` / ``mass_non1hop`` (mean
    attention mass per type), ``entropy`` (mean), ``top1`` (mean largest weight) and ``empty`` (share of the pairs
    without a selected node); NaN means for an empty bin.  Pure torch, on the device of the explanation."""
    mass, ent, top1 = expl.mass.to(torch.float64), expl.entropy.to(torch.float64), expl.weights[:, 0].to(torch.float64)
    empty = (expl.nodes[:, 0] < 0).to(torch.float64)
    P = ent.numel()
    if values is None:
        if bins is not None:
            raise ValueError("bins need the values they cut")
        sel = [(None, torch.ones(P, dtype=torch.bool, device=ent.device))]
    else:
        v = torch.as_tensor(values).reshape(-1).to(ent.device)
        if v.numel() != P:
            raise ValueError(f"values has {v.numel()} entries, the explanation {P} pairs")
        sel = [((lo, hi), (v >= lo) & (v < hi)) for lo, hi in (CN_BINS if bins is None else bins)]
    out = []
    nan = float("nan")
    for b, m in sel:
        c = int(m.sum())
        row = {"bin": b, "count": c}
        if c == 0:
            row.update(mass_cn=nan, mass_1hop=nan, mass_non1hop=nan, entropy=nan, top1=nan, empty=nan)
        else:
            mm = mass[m].mean(dim=0).tolist()
            row.update(mass_cn=mm[0], mass_1hop=mm[1], mass_non1hop=mm[2], entropy=float(ent[m].mean()),
                       top1=float(top1[m].mean()), empty=float(empty[m].mean()))
        out.append(row)
    return out
