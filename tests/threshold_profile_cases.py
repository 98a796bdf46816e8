"""Graphs, pairs and threshold grids shared by test_threshold_profile_host.py and test_gpu_threshold_profile.py.

Two graphs: a 300-node Chung-Lu graph with one hub (degree >= 80) and one isolated node, PPR from the host producer at
eps = 1e-3; and the graph of the lp_all_d64 fixture.  257 pairs each.  The grid of a graph holds 0, two ordinary values
and two thresholds taken from round-tripped values the oracle returned for these very pairs:
  * the pa of a ONE-HOP entry whose raw P[a, v] lies strictly below its round trip rt1 (and whose pb is no smaller): a
    kernel that compared raw values would drop the entry at this threshold;
  * the pa of a COMMON-NEIGHBOUR entry with the same property for its round trip rt2.  (A common-neighbour value whose
    rt2 DIFFERS from its rt1 does not exist in fp32: 2 x and 2 (x + 1) are exact, so fl(2 x + 2) = 2 fl(x + 1) and
    rt2(x) == rt1(x) bit for bit for every finite x -- ``round_trips_differ`` counts such values and the host test
    asserts that count, so a change of that fact would be noticed.)
"""
import functools

import numpy as np

from lpformer_amd import data as D
from lpformer_amd import graph
from lpformer_amd.ppr import calc_ppr
from oracle import lpformer_oracle as O
from tests.golden_util import Fixture

N_PAIRS = 257
ORDINARY = (1e-3, 1e-2)
HUB_SEED = 0


class Case:
    def __init__(self, name, adj, ppr, pairs, hub=None, iso=None):
        self.name, self.adj, self.ppr, self.pairs, self.hub, self.iso = name, adj, ppr, pairs, hub, iso
        self.n = adj.n
        self.special = special_thresholds(self)              # (one-hop boundary, common-neighbour boundary)
        self.grid = np.sort(np.asarray((0.0,) + ORDINARY + self.special, dtype=np.float32))

    def oracle(self, triple):
        """tag -> per-pair counts of select_nodes for the threshold triple."""
        sel = O.select_nodes(self.pairs, (self.adj.rowptr, self.adj.col.astype(np.int64)),
                             (self.ppr.rowptr, self.ppr.col.astype(np.int64), self.ppr.val), triple, n=self.n)
        return {tag: np.bincount(v[0][0], minlength=self.pairs.shape[1]) for tag, v in sel.items()}


def raw_ppr(ppr, rows, cols):
    """P[rows, cols] as stored (0 where nothing is)."""
    out = np.zeros(rows.size, np.float32)
    for k, (r, c) in enumerate(zip(rows.tolist(), cols.tolist())):
        lo, hi = ppr.rowptr[r], ppr.rowptr[r + 1]
        i = lo + np.searchsorted(ppr.col[lo:hi], c)
        if i < hi and ppr.col[i] == c:
            out[k] = ppr.val[i]
    return out


def special_thresholds(case):
    sel = O.select_nodes(case.pairs, (case.adj.rowptr, case.adj.col.astype(np.int64)),
                         (case.ppr.rowptr, case.ppr.col.astype(np.int64), case.ppr.val), (0.0, 0.0, 0.0), n=case.n)
    ix, pa, pb = sel["onehop"]
    raw = raw_ppr(case.ppr, case.pairs[0][ix[0]], ix[1])
    ok = (raw < pa) & (pb >= pa) & (pa > 0)
    assert ok.any(), f"{case.name}: no one-hop entry whose raw PPR value lies below its round trip"
    th_hop = float(pa[ok].min())
    ix, pa, pb = sel["cn"]
    raw = raw_ppr(case.ppr, case.pairs[0][ix[0]], ix[1])
    ok = (raw < pa) & (pb >= pa) & (pa != np.float32(th_hop))
    assert ok.any(), f"{case.name}: no common neighbour whose raw PPR value lies below its round trip"
    th_cn = float(pa[ok].max())
    assert len({0.0, th_hop, th_cn} | {float(np.float32(t)) for t in ORDINARY}) == 5
    return th_hop, th_cn


def round_trips_differ(case) -> int:
    """Stored PPR values of the case whose two round trips differ (none can: see the module docstring)."""
    v = case.ppr.val.astype(np.float32)
    one, two = np.float32(1), np.float32(2)
    return int(np.count_nonzero(((v + one) - one) != ((v * two + two) - two) / two))


def _pairs(ei, n, rng, extra):
    """257 pairs: existing edges, a == b, the extras, a duplicated pair, random pairs."""
    edges = ei[:, rng.choice(ei.shape[1], size=96, replace=False)]
    same = rng.integers(0, n, size=16)
    parts = [edges, np.stack([same, same])] + extra
    have = sum(p.shape[1] for p in parts)
    rnd = rng.integers(0, n, size=(2, N_PAIRS - have - 1))
    pairs = np.concatenate(parts + [rnd, edges[:, :1]], axis=1).astype(np.int64)    # the last pair repeats the first
    assert pairs.shape == (2, N_PAIRS)
    return np.ascontiguousarray(pairs)


@functools.lru_cache(maxsize=None)
def hub_case() -> Case:
    n = 300
    ei, _ = D.chung_lu_graph(n, 900, seed=HUB_SEED)
    deg = np.bincount(ei[0], minlength=n)
    hub = int(np.argmax(deg))
    cand = np.flatnonzero(deg > 0)
    iso = int(cand[cand != hub][-1])                         # its edges are removed below
    rng = np.random.default_rng(HUB_SEED + 1)
    others = np.setdiff1d(np.arange(n), [hub, iso])
    spokes = rng.choice(others, size=90, replace=False)
    ei = np.concatenate([ei, np.stack([np.full(90, hub), spokes]), np.stack([spokes, np.full(90, hub)])], axis=1)
    ei = ei[:, (ei[0] != iso) & (ei[1] != iso)]
    ei = np.unique(ei, axis=1)                               # coalesced, sorted by (row, col)
    adj = graph.mask_csr(ei, n, symmetric=True)
    deg = np.diff(adj.rowptr)
    assert deg[hub] >= 80 and deg[iso] == 0
    ppr = calc_ppr(ei, n, eps=1e-3)
    leaf = int(np.flatnonzero(deg == 1)[0])
    extra = [np.array([[hub, hub, leaf, iso, iso, 5], [hub, leaf, hub, 7, iso, iso]])]
    return Case("hub300", adj, ppr, _pairs(ei, n, rng, extra), hub, iso)


@functools.lru_cache(maxsize=None)
def fixture_case() -> Case:
    fx = Fixture("lp_all_d64")
    ei = fx["edge_index"].astype(np.int64)
    adj = graph.mask_csr(ei, fx.n, symmetric=True)
    r, c, v = fx.ppr_coo
    ppr = graph.csr_from_coo(r, c, v, fx.n)
    rng = np.random.default_rng(11)
    batch = fx["batch"].astype(np.int64)[:, :64]
    return Case("lp_all_d64", adj, ppr, _pairs(ei, fx.n, rng, [batch]))


CASES = {"hub300": hub_case, "lp_all_d64": fixture_case}
