"""Per-node structure of the typing adjacency: degree, core number, connected component and triangle count of every
node, on the device.

Every other analysis entry point describes a PAIR; this one describes a NODE.  It answers where the endpoints of a
pair sit in the graph (dense core or fringe: ``core``; clustered neighbourhood or tree-like: ``clustering``), which
pairs have no structural signal at all (endpoints in different components: two gathers instead of a BFS per pair), and
what the dataset table of a link-prediction paper lists (``NodeStructure.summary``).  The reference has no such code;
the host baselines are ``networkx.core_number`` / ``networkx.triangles``.

Contract (shared by the kernels of csrc/node_structure.hip and the numpy restatement below).  The graph is the simple
undirected graph G of a binary CSR with sorted, unique int32 columns and a SYMMETRIC pattern -- the typing adjacency
the selection reads, the contract of ``hops.py``.  ``u ~ v`` iff ``u != v`` and v is in row u.  Values are ignored;
stored self-loops change nothing (every kernel skips ``col == row``); a non-symmetric pattern is outside the contract.

* ``degree``     int32 [n]   neighbours other than the node itself
* ``core``       int32 [n]   core number: the largest k such that the node lies in a subgraph of G with minimum degree
                             >= k; 0 for an isolated node
* ``component``  int32 [n]   the SMALLEST NODE ID of the node's connected component; an isolated node is its own
* ``triangles``  int64 [n]   the triangles of G through the node

The result is a pure function of the graph: it does not depend on the launch shape, on ``sweeps_per_read`` or on
timing; two runs are bitwise equal.  Integers only.  There is no incremental refresh under ``update_graph``: a fresh
call IS the refresh.

    ns = node_structure(model, test_set=True)
    evaluate.metrics_by_bin(pos_scores, neg_scores, pair_node_values(ns.core, pos_edges), bins=CORE_BINS)
    hopeless = ~same_component(ns, pos_edges)                # positives no path joins
    ns.summary()                                             # the dataset table
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import scipy.sparse as sp
import torch
from scipy.sparse.csgraph import connected_components

from . import _lib, graph, ops, sources
from ._lib import LpfError, check, ptr

KINDS = ("degree", "core", "component", "triangles")
# Half-open [lo, hi) bins in the style of evaluate.CN_BINS, for min / max of the endpoints' values
# (pair_node_values).  DEGREE_BINS: isolated, then roughly geometric -- leaves and chains (1-2), the bulk of a
# collab-like graph (3-9, mean degree about 10), above the mean (10-31), well connected (32-99), hubs.  CORE_BINS:
# isolated (core 0), tree-like fringe (1), thin (2-3), then geometric up to the dense core; a ddi-like graph
# (degeneracy in the hundreds) fills the last bins, a collab-like one the first five.
DEGREE_BINS = ((0, 1), (1, 3), (3, 10), (10, 32), (32, 100), (100, 1 << 31))
CORE_BINS = ((0, 1), (1, 2), (2, 4), (4, 8), (8, 16), (16, 64), (64, 1 << 31))
HV_FORMS = {"default": _lib.CONST["LPF_CORE_FORM_DEFAULT"], "bisect": _lib.CONST["LPF_CORE_FORM_BISECT"]}
_MAX = (1 << 31) - 2                  # n, nnz < 2^31 - 1: int32 columns, int32 list items


# ----------------------------------------------------------------------------------------------------------- result
@dataclass
class NodeStructure:
    """The per-node columns of ``node_structure`` on one device (a kind that was not asked for is None), the number of
    nodes ``n``, and ``sweeps``: how many launches each iterative kernel ran (``"core"``: lpf_core_sweep,
    ``"component"``: lpf_components_hook), no-op launches behind the converged one included -- for diagnosis only, the
    one field that depends on ``sweeps_per_read`` and on timing."""
    n: int
    degree: Optional[torch.Tensor] = None
    core: Optional[torch.Tensor] = None
    component: Optional[torch.Tensor] = None
    triangles: Optional[torch.Tensor] = None
    sweeps: dict = field(default_factory=dict)

    def _need(self, *kinds):
        missing = [k for k in kinds if getattr(self, k) is None]
        if missing:
            raise ValueError(f"this NodeStructure was computed without {missing}: ask node_structure for these kinds")

    @property
    def clustering(self) -> torch.Tensor:
        """float64 [n]: the local clustering coefficient 2 T / (d (d - 1)), 0 where d < 2 -- from the integers, one
        division."""
        self._need("degree", "triangles")
        d = self.degree.to(torch.int64)
        wedges = d * (d - 1)
        ratio = (2 * self.triangles).to(torch.float64) / wedges.clamp(min=1).to(torch.float64)
        return torch.where(d >= 2, ratio, torch.zeros_like(ratio))

    @property
    def component_size(self) -> torch.Tensor:
        """int64 [n]: the number of nodes in each node's component."""
        self._need("component")
        label = self.component.to(torch.int64)
        return torch.bincount(label, minlength=self.n)[label]

    def summary(self) -> dict:
        """The dataset table as a plain dict: ``nodes``, ``edges`` (undirected), ``max_degree``, ``mean_degree``,
        ``degeneracy`` (the largest core number), ``components``, ``largest_component_share`` (of the nodes),
        ``triangles`` (of the graph), ``transitivity`` (sum_v T(v) / wedges, wedges = sum_v d (d - 1) / 2: three
        times the triangles over the connected triples) and ``mean_clustering``.  Needs all four kinds."""
        self._need(*KINDS)
        n = self.n
        d = self.degree.to(torch.int64)
        label = self.component.to(torch.int64)
        tri = int(self.triangles.sum())
        wedges = int((d * (d - 1)).sum()) // 2
        sizes = torch.bincount(label, minlength=n) if n else torch.zeros(0, dtype=torch.int64)
        return {"nodes": n, "edges": int(d.sum()) // 2, "max_degree": int(d.max()) if n else 0,
                "mean_degree": float(d.sum()) / n if n else 0.0, "degeneracy": int(self.core.max()) if n else 0,
                "components": int((sizes > 0).sum()), "largest_component_share": float(sizes.max()) / n if n else 0.0,
                "triangles": tri // 3, "transitivity": tri / wedges if wedges else 0.0,
                "mean_clustering": float(self.clustering.mean()) if n else 0.0}


# ------------------------------------------------------------------------------------------------------- pair values
def pair_node_values(column: torch.Tensor, edges, reduce: str = "min") -> torch.Tensor:
    """The per-pair axis for ``evaluate.metrics_by_bin``, ``bootstrap_by_bin`` and ``attention_profile``: ``min``,
    ``max`` or ``sum`` of ``column[a]``, ``column[b]`` over the pairs of ``edges`` ([P, 2] or [2, P], moved to the
    column's device), [P] in the column's dtype (int64 for the sum of an integer column).  A pair with an id outside
    ``[0, n)`` gives -1."""
    if reduce not in ("min", "max", "sum"):
        raise ValueError(f"reduce must be 'min', 'max' or 'sum'; got {reduce!r}")
    if not isinstance(column, torch.Tensor) or column.dim() != 1:
        raise ValueError("column must be a 1-D tensor of per-node values")
    batch = sources.as_pairs(edges).to(column.device, dtype=torch.int64)
    n = column.shape[0]
    ok = ((batch >= 0) & (batch < n)).all(dim=0)
    safe = torch.where(ok.unsqueeze(0), batch, torch.zeros_like(batch))
    if n == 0:
        va = vb = torch.zeros(batch.shape[1], dtype=column.dtype, device=column.device)
    else:
        va, vb = column[safe[0]], column[safe[1]]
    if reduce == "sum" and not column.dtype.is_floating_point:
        va, vb = va.to(torch.int64), vb.to(torch.int64)
    out = torch.minimum(va, vb) if reduce == "min" else torch.maximum(va, vb) if reduce == "max" else va + vb
    return torch.where(ok, out, torch.full_like(out, -1))


def same_component(ns: NodeStructure, edges) -> torch.Tensor:
    """bool [P]: whether a path joins the endpoints of each pair (``pair_distance(...) >= 0`` at the cost of two
    gathers); False for a pair with an id outside ``[0, n)``."""
    ns._need("component")
    batch = sources.as_pairs(edges).to(ns.component.device, dtype=torch.int64)
    ok = ((batch >= 0) & (batch < ns.n)).all(dim=0)
    if ns.n == 0:
        return ok
    safe = torch.where(ok.unsqueeze(0), batch, torch.zeros_like(batch))
    return ok & (ns.component[safe[0]] == ns.component[safe[1]])


# ---------------------------------------------------------------------------------------------------------- options
def _check_kinds(kinds) -> tuple:
    if isinstance(kinds, str):
        kinds = (kinds,)
    kinds = tuple(kinds)
    bad = [k for k in kinds if k not in KINDS]
    if bad or not kinds:
        raise ValueError(f"kinds must be drawn from {KINDS}; got {kinds!r}")
    return kinds


def _check_count(value, what: str, none_ok: bool = False):
    if value is None and none_ok:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or int(value) < 1:
        raise ValueError(f"{what} must be a positive integer; got {value!r}")
    return int(value)


# ------------------------------------------------------------------------------------------------- host restatement
def _simple(adj: graph.CSR) -> sp.csr_matrix:
    """The 0/1 int64 scipy matrix of the pattern without its diagonal."""
    n = int(adj.n)
    col = np.asarray(adj.col).astype(np.int64)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(adj.rowptr, np.int64)))
    keep = row != col
    A = sp.csr_matrix((np.ones(int(keep.sum()), np.int64), (row[keep], col[keep])), shape=(n, n))
    A.sum_duplicates()
    A.sort_indices()
    A.data[:] = 1
    return A


def _peel(indptr, indices, deg) -> np.ndarray:
    """Core numbers by bucket peeling (Batagelj-Zaversnik, O(m)): nodes kept sorted by current degree in ``vert``, the
    node of least degree is removed and each neighbour of larger degree moves one bucket down."""
    n = deg.size
    if n == 0:
        return deg.astype(np.int32)
    core = deg.astype(np.int64).tolist()
    start = np.concatenate([[0], np.cumsum(np.bincount(deg, minlength=int(deg.max()) + 1))[:-1]]).tolist()
    vert = np.argsort(deg, kind="stable").tolist()
    pos = [0] * n
    for i, v in enumerate(vert):
        pos[v] = i
    indptr, indices = indptr.tolist(), indices.tolist()
    for i in range(n):
        v = vert[i]
        dv = core[v]
        for u in indices[indptr[v]:indptr[v + 1]]:
            du = core[u]
            if du > dv:
                pu, pw = pos[u], start[du]
                w = vert[pw]
                if u != w:
                    vert[pu], vert[pw] = w, u
                    pos[u], pos[w] = pw, pu
                start[du] += 1
                core[u] = du - 1
    return np.asarray(core, np.int32)


def _triangle_rows(A: sp.csr_matrix, budget: int = 1 << 25) -> np.ndarray:
    """Row sums of (A @ A) o A over 2, the product taken a block of rows at a time (about ``budget`` multiply-adds)."""
    n = A.shape[0]
    out = np.zeros(n, np.int64)
    deg = np.diff(A.indptr).astype(np.int64)
    cost = np.cumsum(A @ deg) if n else np.zeros(0, np.int64)
    lo = 0
    while lo < n:
        hi = int(np.searchsorted(cost, (cost[lo - 1] if lo else 0) + budget, side="right"))
        hi = min(max(hi, lo + 1), n)
        rows = A[lo:hi]
        out[lo:hi] = np.asarray((rows @ A).multiply(rows).sum(axis=1)).ravel() // 2
        lo = hi
    return out


def structure_reference(adj: graph.CSR, *, kinds=KINDS) -> NodeStructure:
    """``node_structure`` of a host CSR in numpy / scipy (CPU tensors out), each quantity by a DIFFERENT algorithm from
    the device's: core numbers by bucket peeling (Batagelj-Zaversnik), components by
    ``scipy.sparse.csgraph.connected_components`` relabelled to the smallest id, triangles as the row sums of
    ``(A @ A) o A`` over 2 with the diagonal removed first.  The restatement the kernels are tested against, and what
    ``node_structure`` runs when there is no GPU."""
    kinds = _check_kinds(kinds)
    n = int(adj.n)
    A = _simple(adj)
    deg = np.diff(A.indptr).astype(np.int32)
    out = NodeStructure(n)
    if "degree" in kinds:
        out.degree = torch.from_numpy(deg.copy())
    if "core" in kinds:
        out.core = torch.from_numpy(_peel(A.indptr, A.indices, deg))
    if "component" in kinds:
        if n:
            k, label = connected_components(A, directed=False)
            first = np.full(k, n, np.int64)
            np.minimum.at(first, label, np.arange(n))
            out.component = torch.from_numpy(first[label].astype(np.int32))
        else:
            out.component = torch.zeros(0, dtype=torch.int32)
    if "triangles" in kinds:
        out.triangles = torch.from_numpy(_triangle_rows(A))
    return out


# ------------------------------------------------------------------------------------------------------ device path
_ENTRY_ROWS: dict = {}                # per graph.Structure (sources.per_object): the row id of every stored entry


def entry_rows(g: graph.DeviceCSR) -> torch.Tensor:
    """int32 [nnz]: the row id of every stored entry of a device CSR, what the entry-parallel kernels read.  Cached per
    ``graph.Structure``."""
    def make():
        ids = torch.arange(g.n, dtype=torch.int32, device=g.rowptr.device)
        return torch.repeat_interleave(ids, g.rowptr[1:] - g.rowptr[:-1]).contiguous()
    return sources.per_object(_ENTRY_ROWS, g.structure, make)


def _iterate(launch, sweeps_per_read: int, max_sweeps: int, dev, what: str) -> int:
    """Queue ``sweeps_per_read`` launches (``launch(slot)``: the int32 word the launch counts its changes in), read their
    slots back ONCE, stop at a batch with a slot that stayed 0 -- that launch found the fixpoint, the ones behind it
    were no-ops.  Returns the launches made; ``LpfError`` after ``max_sweeps`` without a fixpoint."""
    done = 0
    changed = torch.empty(sweeps_per_read, dtype=torch.int32, device=dev)
    while done < max_sweeps:
        batch = min(sweeps_per_read, max_sweeps - done)
        changed.zero_()
        for i in range(batch):
            launch(changed[i:])
        done += batch
        if not bool((changed[:batch] != 0).all()):       # the one read-back of the batch
            return done
    raise LpfError(f"node_structure: {what} not converged after max_sweeps = {max_sweeps} launches")


@torch.no_grad()
def node_structure(source, *, test_set: bool = False, kinds=KINDS, sweeps_per_read: int = 8, max_sweeps=None,
                   hv_form: str = "default", split_threshold: int = -1) -> NodeStructure:
    """Degree, core number, component label and triangle count of every node of the typing adjacency, by the module
    docstring's contract: a ``NodeStructure`` of device tensors.  Only the ``kinds`` asked for are computed (``core``
    computes the degree it starts from, but returns it only when asked); the others are None.

    ``source``: a ``LinkTransformer`` (the typing adjacency of the split ``test_set`` selects), a ``graph.CSR`` or a
    ``graph.DeviceCSR`` (binary SYMMETRIC pattern).  A host ``graph.CSR`` with no GPU present goes through
    ``structure_reference`` and gives CPU tensors.

    The two iterative kinds queue ``sweeps_per_read`` launches, each with a counter of its own, and read the counters
    back once per batch: core numbers by in-place sweeps of the h-index iteration (lpf_core_sweep: as many changing
    sweeps as the longest chain of dependent drops -- about half the length of a path --, so a long path costs hundreds
    of launches), components by rounds of hook and jump (lpf_components_hook / _jump: a handful).  ``max_sweeps``: the
    launches either loop may make; default nnz + 1 (core: every changing sweep lowers the sum of the estimates, which
    starts at the sum of the degrees <= nnz) and n + 1 (components), bounds that cannot be hit; hitting a smaller one
    raises ``LpfError`` and returns nothing partial.  ``hv_form``: ``"default"`` or ``"bisect"``, how a row of more than
    LPF_CORE_LONG_ROW entries finds its h-index (for measurement: the result is the same); ``split_threshold``: walked
    columns above which a triangle entry gets a workgroup of its own (negative: LPF_HEUR_SPLIT_DEFAULT).  There is no
    incremental form under ``update_graph``: call again."""
    kinds = _check_kinds(kinds)
    spr = _check_count(sweeps_per_read, "sweeps_per_read")
    cap = _check_count(max_sweeps, "max_sweeps", none_ok=True)
    if hv_form not in HV_FORMS:
        raise ValueError(f"hv_form must be one of {tuple(HV_FORMS)}; got {hv_form!r}")
    dev, adj, _, _ = sources.resolve(source, test_set, torch.empty(0), who="node_structure", host_ok=True)
    if dev is None:
        return structure_reference(adj, kinds=kinds)
    n, nnz = int(adj.n), int(adj.nnz)
    if n > _MAX or nnz > _MAX:
        raise ValueError("node_structure: the graph must have fewer than 2^31 - 1 nodes and stored entries")
    out = NodeStructure(n)
    with torch.cuda.device(dev):
        if n == 0:
            for k in kinds:
                setattr(out, k, torch.zeros(0, dtype=torch.int64 if k == "triangles" else torch.int32, device=dev))
            return out
        hip = _lib.hip()
        st = ops.raw_stream(dev)
        rowptr, col = adj.rowptr, adj.col
        row = entry_rows(adj) if ("component" in kinds or "triangles" in kinds) else None
        degree = None
        if "degree" in kinds or "core" in kinds:
            degree = torch.empty(n, dtype=torch.int32, device=dev)
            check(hip.lpf_node_degree(n, nnz, ptr(rowptr), ptr(col), ptr(degree), st), "lpf_node_degree")
            if "degree" in kinds:
                out.degree = degree
        if "core" in kinds:
            est = degree.clone()
            lens = rowptr[1:] - rowptr[:-1]
            long_rows = torch.nonzero(lens > _lib.CONST["LPF_CORE_LONG_ROW"]).flatten().to(torch.int32)
            form = HV_FORMS[hv_form]

            def sweep(slot):
                check(hip.lpf_core_sweep(n, nnz, ptr(rowptr), ptr(col), ptr(long_rows) if long_rows.numel() else None,
                                         long_rows.numel(), form, ptr(est), ptr(slot), st), "lpf_core_sweep")
            out.sweeps["core"] = _iterate(sweep, spr, cap or nnz + 1, dev, "core numbers") if n else 0
            out.core = est
        if "component" in kinds:
            parent = torch.arange(n, dtype=torch.int32, device=dev)

            def hook_and_jump(slot):
                check(hip.lpf_components_hook(n, nnz, ptr(row), ptr(col), ptr(parent), ptr(slot), st),
                      "lpf_components_hook")
                check(hip.lpf_components_jump(n, ptr(parent), st), "lpf_components_jump")
            out.sweeps["component"] = _iterate(hook_and_jump, spr, cap or n + 1, dev, "components") if n else 0
            out.component = parent
        if "triangles" in kinds:
            tri = torch.empty(n, dtype=torch.int64, device=dev)
            scratch = torch.empty(nnz + 1, dtype=torch.int32, device=dev)
            check(hip.lpf_node_triangles(n, nnz, ptr(rowptr), ptr(row), ptr(col), int(split_threshold), ptr(scratch),
                                         ptr(tri), st), "lpf_node_triangles")
            out.triangles = tri
    return out
