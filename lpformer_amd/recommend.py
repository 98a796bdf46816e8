"""Top-K link recommendation: for each source node u, the K candidates v the model scores highest.

The reference only ranks a positive against negatives it is handed (src/train/testing.py:14-121); answering "which K
new links of u are most likely?" meant building the candidate pairs by hand, scoring them and writing a segmented
top-K.  Here the three steps are one call:

1. candidates on the device (``lpf_rec_candidate_count`` / ``lpf_rec_candidate_fill``, csrc/recommend.hip): u's PPR row
   or every node, minus the exclusion row (by default the model's own typing adjacency) and u itself; or the nodes
   most similar to u (``similar.similar_nodes``, csrc/similar.hip), alone or joined with the PPR row's;
2. scoring through ``evaluate.score_edges`` (logits) -- no scoring path of its own;
3. ranking by ``lpf_segment_topk_f32``: by logit, ties to the earlier candidate (the smaller id for the generated
   modes), -0.0 == +0.0, NaN below -inf.

Sources are processed in chunks of whole sources whose candidate total stays within ``max_pairs``.  The candidates
and the ranking of a source depend on that source and its candidates' logits alone, never on the chunking.  The
logits themselves come from ``score_edges``, whose value for a pair can move by a few ulps with the batch the pair
lands in (at most 9e-7 on the test fixtures), so the scores -- and, on such a near-tie, the order -- can too.
"""
from __future__ import annotations

from typing import List, NamedTuple, Tuple

import numpy as np
import torch

from . import _lib, graph
from ._lib import check, ptr
from .ops import raw_stream
from .sources import model_graphs, node_ids

MAX_K = _lib.CONST["LPF_TOPK_MAX_K"]
MAX_SIMILAR = _lib.CONST["LPF_SIMILAR_MAX_M"]
CANDIDATE_MODES = ("ppr", "all", "2hop", "similar", "ppr+similar")


class Recommendations(NamedTuple):
    ids: torch.Tensor           # int64 [S, k]: candidate ids, best first; -1 past counts
    scores: torch.Tensor        # float32 [S, k]: probabilities (logits with logits=True); -inf past counts
    counts: torch.Tensor        # int64 [S]: min(k, n_candidates)
    n_candidates: torch.Tensor  # int64 [S]: |C(u)|


def plan_chunks(counts, max_pairs: int) -> List[Tuple[int, int]]:
    """Split sources 0..S-1 with ``counts[s]`` candidates each into consecutive ranges [lo, hi) whose candidate total is
    at most ``max_pairs``; a source with more than ``max_pairs`` candidates gets a range of its own (a segment is never
    split).  Every source lies in exactly one range; no range is empty.  Pure host logic."""
    if int(max_pairs) < 1:
        raise ValueError("max_pairs must be positive")
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    if (c < 0).any():
        raise ValueError("counts must be non-negative")
    chunks, lo, acc = [], 0, 0
    for s, v in enumerate(c.tolist()):
        if s > lo and acc + v > max_pairs:
            chunks.append((lo, s))
            lo, acc = s, 0
        acc += v
    if c.size:
        chunks.append((lo, int(c.size)))
    return chunks


def _check_similar(n_similar, similar_table, similar_metric):
    """Argument checks of the ``"similar"`` modes' keywords that need no device."""
    from . import similar
    if isinstance(n_similar, bool) or not isinstance(n_similar, (int, np.integer)) or \
            not 1 <= int(n_similar) <= MAX_SIMILAR:
        raise ValueError(f"n_similar must be an integer in [1, {MAX_SIMILAR}]; got {n_similar!r}")
    if similar_metric not in similar.METRICS:
        raise ValueError(f"similar_metric must be one of {similar.METRICS}; got {similar_metric!r}")
    if not isinstance(similar_table, str) or similar_table not in similar.TABLES:
        raise ValueError(f"similar_table must be one of {similar.TABLES}; got {similar_table!r}")


def _check_args(sources, k, candidates):
    """Argument checks that need no device.  Returns (sources as a 1-D int64 tensor, explicit candidates or None)."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= MAX_K:
        raise ValueError(f"k must be an integer in [1, {MAX_K}]; got {k!r}")
    src = node_ids(sources, "sources")
    if src.dim() != 1:
        raise ValueError("sources must be a 1-D tensor [S]")
    explicit = None
    if isinstance(candidates, str):
        if candidates not in CANDIDATE_MODES:
            raise ValueError(f"candidates must be one of {CANDIDATE_MODES} or an int tensor [S, M]; got {candidates!r}")
    else:
        explicit = node_ids(candidates, "explicit candidates")
        if explicit.dim() != 2 or explicit.shape[0] != src.shape[0]:
            raise ValueError("explicit candidates must be [S, M] with one row per source")
    return src, explicit


def _exclusion(model, exclude, adj, dev):
    if exclude is None:
        return None
    if isinstance(exclude, str):
        if exclude != "adj":
            raise ValueError("exclude must be 'adj', None, a graph.CSR or a graph.DeviceCSR")
        return adj
    if isinstance(exclude, graph.DeviceCSR):
        if exclude.rowptr.device != dev:
            raise ValueError("the exclusion DeviceCSR must live on the model's device")
        g = exclude
    elif isinstance(exclude, graph.CSR):
        g = graph.CSR(exclude.rowptr, exclude.col, None, exclude.n).to_device(dev)
    else:
        raise TypeError("exclude must be 'adj', None, a graph.CSR or a graph.DeviceCSR")
    if g.n != model.num_nodes:
        raise ValueError(f"the exclusion graph has {g.n} nodes, the model {model.num_nodes}")
    return g


def _range_check(src: torch.Tensor, n: int, what: str):
    if src.numel() and (int(src.min()) < 0 or int(src.max()) >= n):
        bad = src[(src < 0) | (src >= n)][0]
        raise IndexError(f"{what}: node id {int(bad)} outside [0, {n})")


def generate_candidates(n: int, sources: torch.Tensor, include, min_ppr: float, exclude, exclude_self: bool,
                        split_threshold: int = -1):
    """The candidate counts of device int64 ``sources`` ([S] int64) and a function ``fill(lo, hi, total)`` that returns the
    [2, P] int64 pairs of sources lo..hi-1 (ascending v per source).  ``include``: a DeviceCSR with fp32 values (the
    PPR rows) or None (every node); ``exclude``: a DeviceCSR or None."""
    dev = sources.device
    S = sources.numel()
    hip = _lib.hip()
    inc = (ptr(include.rowptr), ptr(include.col), ptr(include.val)) if include is not None else (None, None, None)
    exc = (ptr(exclude.rowptr), ptr(exclude.col)) if exclude is not None else (None, None)
    counts = torch.zeros(S, dtype=torch.int64, device=dev)
    scratch = torch.empty(S + 1, dtype=torch.int32, device=dev)
    st = raw_stream(dev)
    if S:
        check(hip.lpf_rec_candidate_count(S, n, ptr(sources), *inc, float(min_ppr), *exc, int(bool(exclude_self)),
                                          int(split_threshold), ptr(scratch), ptr(counts), st),
              "lpf_rec_candidate_count")

    def fill(lo: int, hi: int, total: int) -> torch.Tensor:
        pairs = torch.empty((2, total), dtype=torch.int64, device=dev)
        if total:
            seg = counts[lo:hi]
            offset = torch.cumsum(seg, 0) - seg
            check(hip.lpf_rec_candidate_fill(hi - lo, n, sources.data_ptr() + lo * 8, *inc, float(min_ppr), *exc,
                                             int(bool(exclude_self)), int(split_threshold), ptr(scratch), ptr(offset),
                                             total, ptr(pairs), raw_stream(dev)), "lpf_rec_candidate_fill")
        return pairs
    return counts, fill


def twohop_candidates(adj, sources: torch.Tensor, exclude_adj: bool, exclude_self: bool, split_threshold: int = -1):
    """``generate_candidates`` for ``candidates="2hop"``: every v with a common neighbour with u on ``adj`` (one row of
    A A, ``lpf_twohop_count`` / ``lpf_twohop_fill``), minus N(u) with ``exclude_adj``, minus u with ``exclude_self``."""
    from .hard_negatives import TwoHop
    th = TwoHop(adj, sources, (), (1 if exclude_adj else 0) | (2 if exclude_self else 0), split_threshold)

    def fill(lo: int, hi: int, total: int) -> torch.Tensor:
        seg, col, _, _, _ = th.fill(lo, hi, total)
        return torch.stack([sources[lo:hi].repeat_interleave(th.counts[lo:hi], output_size=total),
                            col.to(torch.int64)])
    return th.counts, fill


def similar_candidates(src: torch.Tensor, sim):
    """``generate_candidates`` for ``candidates="similar"``: the ids of ``sim`` (a ``similar.Similar`` of the sources
    ``src``) with the padding dropped, in similarity order."""
    m = sim.ids.shape[1]
    slot = torch.arange(m, device=src.device)

    def fill(lo: int, hi: int, total: int) -> torch.Tensor:
        # entry (s, j) goes to output slot offset[s] + j: the live entries of a row are its first counts[s]
        cnt = sim.counts[lo:hi]
        offset = torch.cumsum(cnt, 0) - cnt
        live = slot[None, :] < cnt[:, None]
        pos = torch.where(live, offset[:, None] + slot[None, :], total)     # (padding lands in a slot past the end)
        pairs = torch.empty((2, total + 1), dtype=torch.int64, device=src.device)
        pairs[0].scatter_(0, pos.reshape(-1), src[lo:hi, None].expand(-1, m).reshape(-1))
        pairs[1].scatter_(0, pos.reshape(-1), sim.ids[lo:hi].reshape(-1))
        return pairs[:, :total]
    return sim.counts, fill


def union_candidates(n: int, src: torch.Tensor, ppr, min_ppr: float, exclude, exclude_self: bool, sim,
                     split_threshold: int = -1):
    """``generate_candidates`` for ``candidates="ppr+similar"``: per source the distinct ids of its ``"ppr"`` candidates
    and of ``sim`` (a ``similar.Similar`` made with the same exclusion), ascending.  A similar id is also a PPR
    candidate exactly when its PPR value passes the ``"ppr"`` test (the exclusion is the same on both sides), so the
    union's size is known from one ``lpf_csr_lookup_f32`` over the [S, m] ids, before anything is built; ``fill`` sorts
    the keys (row - lo) * n + v of the PPR candidates and of the similar-only ids.  Returns (int64 [2, S]: the union's
    counts and the PPR candidates', for the call's one read-back; ``make_fill(PPR counts on the host) -> fill``)."""
    dev = src.device
    S, m = sim.ids.shape
    n_ppr, fill_ppr = generate_candidates(n, src, ppr, min_ppr, exclude, exclude_self, split_threshold)
    live = sim.ids >= 0
    val = torch.zeros(S * m, dtype=torch.float32, device=dev)
    if S:
        rows = src[:, None].expand(-1, m).reshape(-1).contiguous()
        cols = sim.ids.clamp_min(0).reshape(-1).contiguous()
        check(_lib.hip().lpf_csr_lookup_f32(S * m, n, ptr(rows), ptr(cols), ptr(ppr.rowptr), ptr(ppr.col),
                                            ptr(ppr.val), ptr(val), raw_stream(dev)), "lpf_csr_lookup_f32")
    val = val.reshape(S, m)
    only = live & ~((val > 0) & (val >= float(np.float32(min_ppr))))   # similar ids the PPR candidates do not hold

    def make_fill(ppr_host):
        def fill(lo: int, hi: int, total: int) -> torch.Tensor:
            tp = int(ppr_host[lo:hi].sum())
            pp = fill_ppr(lo, hi, tp)
            row = torch.arange(hi - lo, device=dev)
            key_p = row.repeat_interleave(n_ppr[lo:hi], output_size=tp) * n + pp[1]
            key_s = torch.where(only[lo:hi], row[:, None] * n + sim.ids[lo:hi], (hi - lo) * n)   # (others: to the end)
            key = torch.sort(torch.cat([key_p, key_s.reshape(-1)])).values[:total]
            return torch.stack([src[lo:hi][torch.div(key, n, rounding_mode="floor")], key % n])
        return fill
    return torch.stack([n_ppr + only.sum(1), n_ppr]), make_fill


def segment_topk(seg_ptr: torch.Tensor, score: torch.Tensor, cand: torch.Tensor, k: int):
    """(ids int64 [S, k], scores float32 [S, k], counts int64 [S]) of the segments ``seg_ptr`` (int64 [S + 1]) of
    ``score`` (float32) / ``cand`` (int64): the top min(k, len) of each segment by score, ties to the earlier position,
    -0.0 == +0.0, NaN below -inf; padding -1 / -inf (``lpf_segment_topk_f32``)."""
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f"k must be in [1, {MAX_K}]")
    dev = score.device
    S = seg_ptr.numel() - 1
    ids = torch.empty((S, k), dtype=torch.int64, device=dev)
    out = torch.empty((S, k), dtype=torch.float32, device=dev)
    counts = torch.empty(S, dtype=torch.int64, device=dev)
    if S > 0:
        seg_ptr = seg_ptr.to(dev, torch.int64).contiguous()
        score = score.to(torch.float32).contiguous()
        cand = cand.to(dev, torch.int64).contiguous()
        scratch = torch.empty(S + 1, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            check(_lib.hip().lpf_segment_topk_f32(S, ptr(seg_ptr), ptr(score), ptr(cand), int(k), ptr(scratch),
                                                  ptr(ids), ptr(out), ptr(counts), raw_stream(dev)),
                  "lpf_segment_topk_f32")
    return ids, out, counts


@torch.no_grad()
def recommend(model, score_func, sources, k: int = 100, *, candidates="ppr", min_ppr: float = 0.0, exclude="adj",
              exclude_self: bool = True, test_set: bool = False, h=None, batch_size: int = 32768,
              max_pairs: int = 1 << 24, logits: bool = False, split_threshold: int = -1, n_similar: int = 128,
              similar_table: str = "embedding", similar_metric: str = "cosine") -> Recommendations:
    """The ``k`` highest-scoring candidates v of every source u in ``sources`` (int [S], host or device; duplicates are
    independent rows).

    ``candidates``: ``"2hop"`` -- every v that shares a neighbour with u on the split's typing adjacency (``exclude``
    must then be ``"adj"`` or None; ``split_threshold`` is the two-hop kernel's); ``"ppr"`` -- the entries of u's row of the split's PPR matrix (``data["ppr"]``, ``data["ppr_test"]``
    with ``test_set``) whose fp32 value is > 0 and >= ``min_ppr``; ``"all"`` -- every node; or an int tensor [S, M] of
    explicit candidates, taken as given (no exclusion, duplicates kept); ``"similar"`` -- the ``n_similar`` (at most
    ``LPF_SIMILAR_MAX_M``) eligible nodes most similar to u by ``similar_metric`` (``"cosine"`` or ``"dot"``) over
    ``similar_table`` (``"embedding"``: the ``h`` this call scores with; ``"x"``: the raw features), from
    ``similar.similar_nodes`` -- these stand in SIMILARITY order, most similar first, so a logit tie goes to the more
    similar node, not to the smaller id; ``"ppr+similar"`` -- the distinct ids of the ``"ppr"`` and the ``"similar"``
    candidates, ascending (the PPR candidates' counts ride in the same read-back as the union's).  ``exclude``:
    ``"adj"`` (the model's typing adjacency of the split), None, a ``graph.CSR`` or a ``graph.DeviceCSR``;
    ``exclude_self`` drops v = u.

    Candidates are scored by ``evaluate.score_edges(..., logits=True)`` (``h`` propagated once when not given), ranked by
    logit with ties to the earlier candidate (the smaller id for the generated modes).  ``scores`` are
    ``torch.sigmoid`` of the logits, or the logits themselves with ``logits=True``.  Sources go in chunks of whole
    sources of at most ``max_pairs`` candidates (one source may exceed it alone).  The counts are read back once to
    size the chunks.  ``split_threshold``: PPR-row length above which a source's candidates are built by a whole
    workgroup (negative: the library default)."""
    from . import evaluate
    src, explicit = _check_args(sources, k, candidates)
    k = int(k)
    similar_mode = explicit is None and candidates in ("similar", "ppr+similar")
    if similar_mode:
        _check_similar(n_similar, similar_table, similar_metric)
    if int(max_pairs) < 1 or int(batch_size) < 1:
        raise ValueError("max_pairs and batch_size must be positive")
    if model.training:
        raise NotImplementedError("recommend needs model.eval(), as score_pairs does")
    dev, adj, ppr = model_graphs(model, test_set, "recommend")
    n = int(model.num_nodes)
    _range_check(src, n, "recommend: sources")
    S = src.numel()
    with torch.cuda.device(dev):
        src = src.to(dev, torch.int64).contiguous()
        if explicit is not None:
            cand = explicit.to(dev, torch.int64).contiguous()
            _range_check(cand, n, "recommend: candidates")
            M = cand.shape[1]
            n_cand = torch.full((S,), M, dtype=torch.int64, device=dev)
            counts_host = np.full(S, M, dtype=np.int64)

            def fill(lo, hi, total):
                return torch.stack([src[lo:hi].repeat_interleave(M), cand[lo:hi].reshape(-1)])
        else:
            if similar_mode:
                from .similar import similar_nodes
                if h is None:
                    h = model.propagate(test_set=test_set)
                sim = similar_nodes(model, src, int(n_similar), table=similar_table, metric=similar_metric,
                                    exclude=exclude, exclude_self=exclude_self, test_set=test_set, h=h)
                if candidates == "similar":
                    n_cand, fill = similar_candidates(src, sim)
                else:
                    both, make_fill = union_candidates(n, src, ppr, min_ppr, _exclusion(model, exclude, adj, dev),
                                                       exclude_self, sim, split_threshold)
                    n_cand = both[0]
            elif candidates == "2hop":
                if exclude not in ("adj", None):
                    raise ValueError("candidates='2hop' takes exclude='adj' or None: the two-hop row kernel drops the "
                                     "row of the adjacency it walks")
                n_cand, fill = twohop_candidates(adj, src, exclude == "adj", exclude_self, split_threshold)
            else:
                n_cand, fill = generate_candidates(n, src, ppr if candidates == "ppr" else None, min_ppr,
                                                   _exclusion(model, exclude, adj, dev), exclude_self, split_threshold)
            if candidates == "ppr+similar":          # (the PPR candidates' counts ride in the same read-back)
                counts_host, ppr_host = both.cpu().numpy()
                fill = make_fill(ppr_host)
            else:
                counts_host = n_cand.cpu().numpy()   # the one read-back: it sizes the chunks and their outputs
        if h is None:
            h = model.propagate(test_set=test_set)
        ids = torch.full((S, k), -1, dtype=torch.int64, device=dev)
        out = torch.full((S, k), float("-inf"), dtype=torch.float32, device=dev)
        counts = torch.zeros(S, dtype=torch.int64, device=dev)
        starts = np.concatenate([[0], np.cumsum(counts_host)])
        for lo, hi in plan_chunks(counts_host, int(max_pairs)):
            total = int(starts[hi] - starts[lo])
            if total == 0:
                continue
            pairs = fill(lo, hi, total)
            lg = evaluate.score_edges(model, score_func, pairs, batch_size, h=h, test_set=test_set, logits=True)
            seg_ptr = torch.from_numpy(starts[lo:hi + 1] - starts[lo]).to(dev)
            ids[lo:hi], out[lo:hi], counts[lo:hi] = segment_topk(seg_ptr, lg, pairs[1], k)
        if not logits:
            out = torch.where(ids >= 0, torch.sigmoid(out), out)
    return Recommendations(ids, out, counts, n_cand)
