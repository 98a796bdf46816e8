"""Pairwise heuristics of candidate pairs on the device: common neighbours (CN), Adamic-Adar (AA), Resource Allocation
(RA) over the typing adjacency, plus the pair's PPR values and the cosine similarity of its node features.

The reference bins its test positives by CN to report ranking quality per bin (src/train/eval.py:21-77, behind the
``--bymetric`` / ``--percentile`` arguments of src/run.py:195-196); its ``compute_edge_cn`` builds dense
``adj[edge].to_dense()`` rows per batch, [BS, N] each.  Here CN / AA / RA come from one HIP entry point
(``lpf_pair_heuristics_f32``, csrc/pair_heuristics.hip) that intersects the sorted CSR rows, and the binning is
``evaluate.metrics_by_bin``.

Nothing here changes what scoring reads: a model's graphs are fetched through the same resident device copies the
selection uses, and the per-node weight tables (1 / ln deg, 1 / deg) are cached next to the graph object they belong to.
"""
from __future__ import annotations

import torch

from . import _lib, graph, ops, sources
from ._lib import check, ptr

KINDS = ("cn", "aa", "ra", "ppr", "feat")

# per-object state (sources.per_object): the weight tables of a graph, the device copy of a host feature tensor
_TABLES: dict = {}
_FEATURES: dict = {}


def weight_tables(g: graph.DeviceCSR):
    """(w_aa, w_ra) float32[n] of a device CSR: 1 / ln deg (0 where deg <= 1: the usual inf -> 0 of Adamic-Adar) and
    1 / deg (0 for an isolated node), each computed in fp64 and rounded to fp32 once.  Cached per graph object."""
    def make():
        deg = (g.rowptr[1:] - g.rowptr[:-1]).to(torch.float64)
        w_aa = torch.where(deg > 1, 1.0 / torch.log(deg.clamp_min(2.0)), torch.zeros_like(deg))
        w_ra = torch.where(deg > 0, 1.0 / deg.clamp_min(1.0), torch.zeros_like(deg))
        return w_aa.to(torch.float32).contiguous(), w_ra.to(torch.float32).contiguous()
    return sources.per_object(_TABLES, g, make)


def device_features(x: torch.Tensor, dev) -> torch.Tensor:
    """fp32 node features on ``dev``: ``x`` itself when it lives there, else a device copy cached per tensor object
    and version (a host-resident data["x"] is not uploaded again on every call)."""
    if x.device == dev and x.dtype == torch.float32:
        return x.detach()
    hit = sources.per_object(_FEATURES, x, lambda: [None, None])      # (keyed by the data dict's own tensor object)
    if hit[0] != x._version or hit[1] is None or hit[1].device != dev:
        hit[0], hit[1] = x._version, x.detach().to(dev, dtype=torch.float32)
    return hit[1]


def _check_kinds(kinds):
    if isinstance(kinds, str):
        kinds = (kinds,)
    kinds = tuple(kinds)
    bad = [k for k in kinds if k not in KINDS]
    if bad or not kinds:
        raise ValueError(f"kinds must be a non-empty subset of {KINDS}; got {kinds!r}")
    return kinds


@torch.no_grad()
def pair_heuristics(source, edges, *, test_set: bool = False, kinds=("cn", "aa", "ra"), chunk: int = 1 << 20,
                    split_threshold: int = -1) -> dict:
    """Pairwise heuristics of ``edges`` ([P, 2] or [2, P], host or device) as device tensors of shape [P]:

    * ``"cn"`` -> ``cn`` int32: |N(a) & N(b)| on the typing adjacency (``compute_edge_cn``, src/train/eval.py:21-41);
    * ``"aa"`` / ``"ra"`` -> ``aa`` / ``ra`` float32: Adamic-Adar (sum of 1 / ln deg) and Resource Allocation (sum of
      1 / deg) over the common neighbours;
    * ``"ppr"`` -> ``ppr_ab`` = PPR[a, b] and ``ppr_ba`` = PPR[b, a] (0 where nothing is stored) -- model sources only;
    * ``"feat"`` -> ``feat``: cosine similarity of the rows of ``data["x"]`` -- model sources only.

    ``source``: a ``LinkTransformer`` (the typing adjacency and PPR matrix of the split ``test_set`` selects, the same
    objects its selection reads), a ``graph.CSR`` or a ``graph.DeviceCSR`` (binary pattern: values are ignored).
    ``chunk``: pairs per launch.  ``split_threshold``: walked-row length above which a pair gets a whole workgroup
    (negative: the library default ``LPF_HEUR_SPLIT_DEFAULT``).  Nothing is read back to the host."""
    kinds = _check_kinds(kinds)
    chunk = sources.clamp_chunk(chunk)
    batch = sources.as_pairs(edges)
    dev, adj, ppr, x = sources.resolve(source, test_set, batch, who="pair_heuristics")
    if ("ppr" in kinds and ppr is None) or ("feat" in kinds and x is None):
        raise ValueError("'ppr' and 'feat' need a LinkTransformer source (its PPR matrix and node features)")
    batch = batch.to(dev, dtype=torch.int64).contiguous()
    P = batch.shape[1]
    out = {}
    with torch.cuda.device(dev):
        st = ops.raw_stream(dev)
        want = [k for k in ("cn", "aa", "ra") if k in kinds]
        if want:
            cn = torch.empty(P, dtype=torch.int32, device=dev) if "cn" in want else None
            aa = torch.empty(P, dtype=torch.float32, device=dev) if "aa" in want else None
            ra = torch.empty(P, dtype=torch.float32, device=dev) if "ra" in want else None
            w_aa, w_ra = weight_tables(adj) if ("aa" in want or "ra" in want) else (None, None)
            if P:
                scratch = torch.empty(min(P, chunk) + 1, dtype=torch.int32, device=dev)
                for lo, m in sources.chunks(P, chunk):
                    def at(t):
                        return None if t is None else t.data_ptr() + lo * t.element_size()
                    check(_lib.hip().lpf_pair_heuristics_f32(
                        m, adj.n, batch.data_ptr() + lo * 8, P, ptr(adj.rowptr), ptr(adj.col), ptr(w_aa), ptr(w_ra),
                        int(split_threshold), ptr(scratch), at(cn), at(aa), at(ra), st), "lpf_pair_heuristics_f32")
            out.update({k: v for k, v in (("cn", cn), ("aa", aa), ("ra", ra)) if v is not None})
        if "ppr" in kinds:
            for name, rows, cols in (("ppr_ab", batch[0], batch[1]), ("ppr_ba", batch[1], batch[0])):
                v = torch.empty(P, dtype=torch.float32, device=dev)
                if P:
                    check(_lib.hip().lpf_csr_lookup_f32(P, ppr.n, ptr(rows), ptr(cols), ptr(ppr.rowptr), ptr(ppr.col),
                                                        ptr(ppr.val), ptr(v), st), "lpf_csr_lookup_f32")
                out[name] = v
        if "feat" in kinds:
            out["feat"] = feature_cosine(device_features(x, dev), batch, chunk)
    return out


def feature_cosine(xd: torch.Tensor, batch: torch.Tensor, chunk: int = 1 << 20) -> torch.Tensor:
    """The ``"feat"`` values of device pairs ``batch`` ([2, P] int64): cosine similarity of the rows of ``xd`` (fp32, on
    the same device), ``chunk`` pairs at a time."""
    n, P = xd.shape[0], batch.shape[1]
    feat = torch.empty(P, dtype=torch.float32, device=batch.device)
    for lo in range(0, P, chunk):     # ids outside [0, n) give 0, as for cn / aa / ra (and nothing is read back)
        a, b = batch[0, lo:lo + chunk], batch[1, lo:lo + chunk]
        ok = (a >= 0) & (a < n) & (b >= 0) & (b < n)
        cos = torch.nn.functional.cosine_similarity(xd[a.clamp(0, n - 1)], xd[b.clamp(0, n - 1)], dim=1)
        feat[lo:lo + a.numel()] = torch.where(ok, cos, torch.zeros_like(cos))
    return feat
