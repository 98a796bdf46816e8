"""Data-dict builder and synthetic graph generators.

The reference's readers (src/util/read_datasets.py:20-254) need the OGB / HeaRT files, which are not available
offline; this module builds the SAME dictionary schema (keys ``x, adj_t, full_adj_t, adj_mask, full_adj_mask, ppr,
ppr_test, num_nodes`` + split tensors) from an edge list, with graph entries already in CSR form so nothing is
converted on the scoring path, and generates synthetic graphs shaped like the named datasets.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import graph
from .ppr import calc_ppr, calc_ppr_gpu


def to_undirected(edge_index, num_nodes: int) -> np.ndarray:
    """PyG ``to_undirected`` for an unweighted edge list (what the reference applies to the validation edges,
    src/util/read_datasets.py:98-99): both directions of every edge, then COALESCED -- duplicate and reciprocal input
    pairs end up once per direction -- sorted by (row, col)."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    row, col = np.concatenate([ei[0], ei[1]]), np.concatenate([ei[1], ei[0]])
    key = np.unique(row * np.int64(num_nodes) + col)
    return np.stack([key // num_nodes, key % num_nodes]).astype(np.int64)


def build_data(edge_index, x, num_nodes: int, *, edge_weight=None, eps: float = 5e-5, alpha: float = 0.15,
               ppr: Optional[graph.CSR] = None, val_edge_index=None, ppr_test: Optional[graph.CSR] = None,
               ppr_threads: int = 0, ppr_device=None) -> dict:
    """Reference-schema data dict (read_data_ogb, src/util/read_datasets.py:20-148) on CSR containers.

    edge_index: [2, E] directed list holding both directions of every undirected edge; edge_weight optional.
    val_edge_index: optional extra (validation) edges used when ``test_set=True`` (``--use-val-in-test``).
    ppr_device: None = host OpenMP producer; a device ("cuda:0") = the GPU producer (bit-identical result)."""
    ei = np.asarray(edge_index, dtype=np.int64)
    n = int(num_nodes)
    data = {"num_nodes": n, "x": torch.as_tensor(x, dtype=torch.float32)}
    w = None if edge_weight is None else np.asarray(edge_weight, np.float32)
    data["adj_t"] = graph.csr_from_coo(ei[0], ei[1], np.ones(ei.shape[1], np.float32) if w is None else w, n)
    data["adj_mask"] = graph.mask_csr(ei, n, symmetric=True)
    def producer(edges):
        if ppr_device is not None:
            return calc_ppr_gpu(edges, n, alpha, eps, device=ppr_device)
        return calc_ppr(edges, n, alpha, eps, ppr_threads)

    data["ppr"] = ppr if ppr is not None else producer(ei)
    if val_edge_index is not None:
        vei = to_undirected(val_edge_index, n)           # mirrored AND coalesced (read_datasets.py:98-99)
        full = np.concatenate([ei, vei], axis=1)
        fw = np.concatenate([np.ones(ei.shape[1], np.float32) if w is None else w, np.ones(vei.shape[1], np.float32)])
        data["full_adj_t"] = graph.csr_from_coo(full[0], full[1], fw, n)
        data["full_adj_mask"] = graph.mask_csr(full, n, symmetric=False)
        data["ppr_test"] = ppr_test if ppr_test is not None else producer(full)
    else:
        data["full_adj_t"], data["full_adj_mask"], data["ppr_test"] = data["adj_t"], data["adj_mask"], data["ppr"]
    return data


def link_split(edge_index, x, num_nodes: int, *, val_frac: float = 0.05, test_frac: float = 0.10,
               negatives: str = "shared", num_neg: Optional[int] = None, seed: int = 0, use_val_in_test: bool = False,
               **build_data_kw) -> dict:
    """A trainable, evaluable data dict from a user's own graph: ``build_data``'s graph entries plus the split tensors
    ``train_pos, train_pos_val, valid_pos, valid_neg, test_pos, test_neg`` of ``readers.py`` (int64 CPU tensors), ready
    for ``fit`` and ``evaluate.evaluate_model``.

    1. the undirected edges of ``edge_index`` ([2, E] or [E, 2], either or both directions) are canonicalised: self-loops
       dropped, one row (min, max) per pair, ascending;
    2. they are permuted by ``torch.randperm`` under ``seed`` and cut into valid (``int(val_frac * E)`` rows), test
       (``int(test_frac * E)``) and train (the rest), in that order;
    3. ``build_data`` runs on the training edges in both directions (``build_data_kw``: eps, alpha, ppr_device, ...);
       with ``use_val_in_test`` the valid edges join the test-time graph (``val_edge_index``);
    4. ``train_pos_val``: a ``randperm`` subset of ``train_pos`` of ``valid_pos``' size, as the readers make it;
    5. ``valid_neg`` / ``test_neg`` come from ``lpformer_amd.negatives`` under ``seed`` and avoid ALL edges (train,
       valid and test).  ``negatives="shared"``: [M, 2] each, M = ``num_neg`` or the split's number of positives, one
       call over both splits' slots (valid first), so no unordered pair occurs twice within or across the two.
       ``negatives="rows"``: [P, num_neg, 2] (default 500, HeaRT's), the sources the first column of the split's
       positives, the test rows on the slots after the valid ones: the two sets are drawn from different streams (a
       source both splits hold may still meet a target twice).  A graph too dense to supply them raises ``ValueError``.

    The same arguments give the same dict, with or without a GPU (the sampler is a pure function of its seed)."""
    from . import negatives as N
    if negatives not in ("shared", "rows"):
        raise ValueError(f"negatives must be 'shared' or 'rows'; got {negatives!r}")
    for key in ("edge_weight", "val_edge_index"):       # (the split decides the order and the roles of the edges)
        if key in build_data_kw:
            raise TypeError(f"link_split builds {key} itself; it takes an unweighted edge list")
    if not (0.0 <= float(val_frac) and 0.0 <= float(test_frac) and float(val_frac) + float(test_frac) < 1.0):
        raise ValueError("val_frac and test_frac must be >= 0 and sum to less than 1")
    n = int(num_nodes)
    ei = np.asarray(torch.as_tensor(edge_index).cpu().numpy() if isinstance(edge_index, torch.Tensor) else edge_index,
                    dtype=np.int64)
    if ei.ndim != 2 or 2 not in ei.shape:
        raise ValueError("edge_index must be [2, E] or [E, 2]")
    if ei.shape[0] != 2:
        ei = ei.T
    if ei.size and (ei.min() < 0 or ei.max() >= n):
        raise IndexError(f"edge_index holds node ids outside [0, {n})")
    lo, hi = np.minimum(ei[0], ei[1]), np.maximum(ei[0], ei[1])
    key = np.unique((lo * np.int64(n) + hi)[lo != hi])
    canon = torch.from_numpy(np.stack([key // n, key % n], axis=1))             # [E, 2], ascending
    E = canon.shape[0]
    g = torch.Generator().manual_seed(int(seed))
    canon = canon[torch.randperm(E, generator=g)]
    n_val, n_test = int(float(val_frac) * E), int(float(test_frac) * E)
    valid_pos, test_pos, train_pos = canon[:n_val], canon[n_val:n_val + n_test], canon[n_val + n_test:]
    tr = train_pos.t().numpy()
    both = np.concatenate([tr, tr[::-1]], axis=1)
    both = both[:, np.argsort(both[0] * np.int64(n) + both[1], kind="stable")]
    val_ei = valid_pos.t().numpy() if (use_val_in_test and n_val) else None
    data = build_data(both, x, n, val_edge_index=val_ei, **build_data_kw)
    data["edge_index"] = torch.from_numpy(np.ascontiguousarray(both))
    data["train_pos"], data["valid_pos"], data["test_pos"] = train_pos, valid_pos, test_pos
    data["train_pos_val"] = train_pos[torch.randperm(train_pos.shape[0], generator=g)[:n_val]]
    known = graph.mask_csr(np.stack([key // n, key % n]), n, symmetric=True)    # every edge of every split
    if negatives == "shared":
        m_val, m_test = (n_val, n_test) if num_neg is None else (int(num_neg), int(num_neg))
        neg = N.negative_pairs(known, m_val + m_test, seed=int(seed)).cpu().t().contiguous()
        data["valid_neg"], data["test_neg"] = neg[:m_val], neg[m_val:]
    else:
        k = 500 if num_neg is None else int(num_neg)
        data["valid_neg"] = N.negative_rows(known, valid_pos[:, 0], k, seed=int(seed), as_pairs=True).cpu()
        data["test_neg"] = N.negative_rows(known, test_pos[:, 0], k, seed=int(seed), as_pairs=True,
                                           row_base=n_val).cpu()
    return data


def chung_lu_graph(n: int, n_edges: int, gamma: float = 2.5, seed: int = 0, max_weight: int = 0):
    """Power-law (Chung-Lu) simple undirected graph: expected degree of node i ~ (i + i0)^(-1/(gamma-1)).
    Returns (edge_index [2, 2E] both directions sorted, edge_weight or None)."""
    rng = np.random.default_rng(seed)
    expo = 1.0 / (gamma - 1.0)
    wts = (np.arange(n, dtype=np.float64) + 10.0) ** (-expo)
    p = wts / wts.sum()
    cdf = np.cumsum(p)
    m = int(n_edges * 1.15) + 16
    a = np.searchsorted(cdf, rng.random(m)).clip(0, n - 1)
    b = np.searchsorted(cdf, rng.random(m)).clip(0, n - 1)
    perm = rng.permutation(n)  # decouple node id from degree rank
    a, b = perm[a], perm[b]
    keep = a != b
    lo, hi = np.minimum(a, b)[keep], np.maximum(a, b)[keep]
    key = np.unique(lo.astype(np.int64) * n + hi)
    if key.size > n_edges:
        key = np.sort(rng.choice(key, size=n_edges, replace=False))
    lo, hi = key // n, key % n
    src, dst = np.concatenate([lo, hi]), np.concatenate([hi, lo])
    weight = None
    if max_weight > 0:  # Zipf-like integer co-author counts (ogbl-collab carries summed multi-edge weights)
        wv = np.minimum(rng.zipf(2.0, size=lo.size), max_weight).astype(np.float32)
        weight = np.concatenate([wv, wv])
    order = np.argsort(src * n + dst, kind="stable")
    ei = np.stack([src[order], dst[order]]).astype(np.int64)
    return ei, (None if weight is None else weight[order])


def sample_pairs(edge_index, n: int, bs: int, seed: int = 0, frac_edges: float = 0.5) -> np.ndarray:
    """Candidate batch [2, bs]: a fraction of existing edges (positives) and uniform random pairs (negatives)."""
    rng = np.random.default_rng(seed)
    k = int(bs * frac_edges)
    pos = np.asarray(edge_index)[:, rng.integers(0, edge_index.shape[1], size=k)]
    neg = rng.integers(0, n, size=(2, bs - k))
    b = np.concatenate([pos, neg], axis=1)
    return np.ascontiguousarray(b[:, rng.permutation(bs)].astype(np.int64))


# name -> (N, F_in, undirected edges, D, L, residual, thresholds, eps, batch, gamma, max edge weight)
CONFIGS = {
    # SURVEY.md section 8 per-config table; dataset statistics are public OGB numbers, hyper-parameters from
    # scripts/replicate_existing.sh / replicate_heart.sh of the reference.
    "collab": dict(n=235_868, f_in=128, edges=1_180_000, dim=128, gnn_layers=3, residual=False,
                   thresholds=(0.0, 1e-4, 1e-2), eps=5e-5, batch=32_768, gamma=2.5, max_weight=10),
    "ppa": dict(n=576_289, f_in=58, edges=21_200_000, dim=64, gnn_layers=3, residual=True,
                thresholds=(0.0, 1e-4, 1e-2), eps=5e-5, batch=32_768, gamma=2.8, max_weight=0),
    "citation2": dict(n=2_927_963, f_in=128, edges=30_400_000, dim=64, gnn_layers=3, residual=True,
                      thresholds=(0.0, 1e-3, 1e-2), eps=2.5e-3, batch=32_768, gamma=2.6, max_weight=0),
    "ddi": dict(n=4_267, f_in=256, edges=1_070_000, dim=256, gnn_layers=3, residual=False,
                thresholds=(0.0, 1e-2, 1.0), eps=5e-6, batch=8_192, gamma=8.0, max_weight=0),
    "cora": dict(n=2_708, f_in=1_433, edges=4_488, dim=256, gnn_layers=1, residual=False,
                 thresholds=(0.0, 1e-2, 1e-2), eps=1e-4, batch=16_384, gamma=3.0, max_weight=0,
                 layer_norm=False, relu=False),
    "tiny": dict(n=3_000, f_in=32, edges=12_000, dim=64, gnn_layers=2, residual=False,
                 thresholds=(0.0, 1e-3, 1e-2), eps=1e-3, batch=2_048, gamma=2.5, max_weight=4),
}


def train_args_for(cfg: dict) -> dict:
    th = cfg["thresholds"]
    return {"thresh_cn": th[0], "thresh_1hop": th[1], "thresh_non1hop": th[2], "dim": cfg["dim"], "trans_layers": 1,
            "num_heads": 1, "att_drop": 0.0, "dropout": 0.0, "gnn_drop": 0.0, "feat_drop": 0.0, "gcn_cache": True,
            "gnn_layers": cfg["gnn_layers"], "residual": cfg["residual"], "layer_norm": cfg.get("layer_norm", True),
            "relu": cfg.get("relu", True)}
