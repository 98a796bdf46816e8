"""node_structure without a GPU: the numpy / scipy restatement (structure_reference, what the entry point runs for a
host graph.CSR when no GPU is present) against networkx and the hand cases, the derived columns, the per-pair helpers,
argument validation and the C ABI registration.  Every comparison of the four columns is exact integer equality."""
import numpy as np
import pytest
import torch

import lpformer_amd
from lpformer_amd import _lib, graph, structure
from lpformer_amd.structure import (CORE_BINS, DEGREE_BINS, KINDS, NodeStructure, node_structure, pair_node_values,
                                    same_component, structure_reference)
from tests import node_structure_cases as NC

SYMBOLS = {"lpf_node_degree": 6, "lpf_core_sweep": 10, "lpf_components_hook": 7, "lpf_components_jump": 3,
           "lpf_node_triangles": 9}


def _ns(name) -> NodeStructure:
    ref = NC.reference(name)
    return NodeStructure(ref["degree"].size, **{k: torch.from_numpy(v.copy()) for k, v in ref.items()})


@pytest.mark.parametrize("name", NC.NAMES + ("Kloops",))
def test_restatement_matches_networkx(name):
    nx = pytest.importorskip("networkx")
    case = NC.graph_k_loops() if name == "Kloops" else NC.CASES[name]()
    A = case.A.copy()
    A.setdiag(0)
    A.eliminate_zeros()
    G = nx.from_scipy_sparse_array(A)
    ref = NC.reference(name)
    nodes = range(case.n)
    core, tri = nx.core_number(G), nx.triangles(G)
    np.testing.assert_array_equal(ref["degree"], [G.degree(v) for v in nodes])
    np.testing.assert_array_equal(ref["core"], [core[v] for v in nodes])
    np.testing.assert_array_equal(ref["triangles"], [tri[v] for v in nodes])
    want = np.empty(case.n, np.int32)
    for comp in nx.connected_components(G):
        want[list(comp)] = min(comp)
    np.testing.assert_array_equal(ref["component"], want)
    assert ref["degree"].dtype == np.int32 and ref["core"].dtype == np.int32
    assert ref["component"].dtype == np.int32 and ref["triangles"].dtype == np.int64


def test_the_graphs_are_what_the_cases_say():
    """The counts the graphs were chosen for, printed and pinned."""
    got = {}
    for name in NC.NAMES:
        ref = NC.reference(name)
        got[name] = (int(ref["core"].max()), int(np.unique(ref["component"]).size), int(ref["triangles"].sum()) // 3,
                     int(ref["degree"].max()))
        print(name, "max core, components, triangles, max degree:", got[name])
    assert got["S"][:3] == (2, 250, 3) and got["H"] == (3, 275, 165, 603) and got["C"] == (299, 1, 8_910_200, 300)
    assert got["P"] == (1, 1, 0, 2)
    k = NC.reference("K")
    assert got["K"][0] >= 129 and int((k["degree"] == 0).sum()) >= 40 and got["K"][2] > 300_000
    lens = np.diff(NC.graph_k().csr.rowptr)
    for cut in (32, 63, 64, 65):                       # rows on both sides of the wavefront width and the switches
        assert (lens <= cut).any() and (lens > cut).any()
    assert {63, 64, 65} <= set(lens.tolist()) | set((lens - 1).tolist())


def test_synchronous_sweep_counts_meet_the_bound():
    for name in ("P", "H"):
        sweeps = NC.sync_core_sweeps(NC.CASES[name]())
        print(name, "synchronous changing sweeps:", sweeps, "bound:", NC.SWEEP_BOUND[name])
        assert sweeps >= NC.SWEEP_BOUND[name]
    assert NC.SWEEP_BOUND == {"P": 1000, "H": 30}


@pytest.mark.parametrize("hand", NC.hand_cases(), ids=lambda h: h.what)
def test_restatement_matches_the_hand_cases(hand):
    ns = structure_reference(hand.csr)
    for k in KINDS:
        assert getattr(ns, k).tolist() == hand.want[k], k
    assert ns.n == hand.csr.n and ns.sweeps == {}


def test_stored_self_loops_change_nothing():
    plain, loops = NC.reference("K"), NC.reference("Kloops")
    assert NC.graph_k_loops().csr.nnz == NC.graph_k().csr.nnz + 100
    for k in KINDS:
        np.testing.assert_array_equal(plain[k], loops[k])


def test_only_the_kinds_asked_for():
    csr = NC.graph_k().csr
    for k in KINDS:
        ns = structure_reference(csr, kinds=(k,))
        for other in KINDS:
            assert (getattr(ns, other) is None) == (other != k)
        np.testing.assert_array_equal(getattr(ns, k).numpy(), NC.reference("K")[k])
    assert structure_reference(csr, kinds="core").degree is None


@pytest.mark.parametrize("name", ("K", "H"))
def test_derived_columns_against_numpy(name):
    ref, ns = NC.reference(name), _ns(name)
    d, t = ref["degree"].astype(np.int64), ref["triangles"]
    want = np.where(d >= 2, 2.0 * t / np.maximum(d * (d - 1), 1), 0.0)
    c = ns.clustering
    assert c.dtype == torch.float64 and np.array_equal(c.numpy(), want)
    assert (c >= 0).all() and (c <= 1).all()
    _, inv, cnt = np.unique(ref["component"], return_inverse=True, return_counts=True)
    size = ns.component_size
    assert size.dtype == torch.int64 and np.array_equal(size.numpy(), cnt[inv])
    s = ns.summary()
    wedges = int((d * (d - 1) // 2).sum())
    assert s == {"nodes": d.size, "edges": int(d.sum()) // 2, "max_degree": int(d.max()),
                 "mean_degree": float(d.sum()) / d.size, "degeneracy": int(ref["core"].max()),
                 "components": cnt.size, "largest_component_share": float(cnt.max()) / d.size,
                 "triangles": int(t.sum()) // 3, "transitivity": int(t.sum()) / wedges,
                 "mean_clustering": float(torch.from_numpy(want).mean())}
    assert all(type(v) in (int, float) for v in s.values())


def test_derived_columns_of_hand_cases_and_missing_kinds():
    tri = structure_reference(NC.hand_cases()[2].csr)
    assert tri.clustering.tolist() == [0.0, 1.0, 1.0 / 3.0, 0.0, 1.0]
    assert tri.component_size.tolist() == [4, 4, 4, 1, 4]
    s = tri.summary()
    assert (s["nodes"], s["edges"], s["components"], s["triangles"], s["degeneracy"]) == (5, 4, 2, 1, 2)
    assert s["transitivity"] == 3 / 5 and s["largest_component_share"] == 0.8       # wedges: 0 + 1 + 3 + 0 + 1
    empty = structure_reference(NC.hand_cases()[0].csr).summary()
    assert empty["edges"] == 0 and empty["components"] == 5 and empty["transitivity"] == 0.0
    assert empty["mean_clustering"] == 0.0 and empty["largest_component_share"] == 0.2
    part = structure_reference(NC.hand_cases()[2].csr, kinds=("degree", "core"))
    for use in (lambda: part.clustering, lambda: part.component_size, part.summary,
                lambda: same_component(part, torch.tensor([[0], [1]]))):
        with pytest.raises(ValueError):
            use()


def test_pair_node_values_and_same_component():
    case, ns = NC.graph_k(), _ns("K")
    a, b = case.pairs
    ok = (a >= 0) & (a < case.n) & (b >= 0) & (b < case.n)
    assert int((~ok).sum()) == 4
    sa, sb = np.where(ok, a, 0), np.where(ok, b, 0)
    core = NC.reference("K")["core"]
    for reduce, fn in (("min", np.minimum), ("max", np.maximum), ("sum", np.add)):
        want = np.where(ok, fn(core[sa].astype(np.int64), core[sb].astype(np.int64)), -1)
        for edges in (torch.from_numpy(case.pairs.copy()), torch.from_numpy(case.pairs.T.copy())):   # [2, P], [P, 2]
            got = pair_node_values(ns.core, edges, reduce)
            assert got.dtype == (torch.int64 if reduce == "sum" else torch.int32) and got.shape == (a.size,)
            np.testing.assert_array_equal(got.numpy(), want)
    np.testing.assert_array_equal(pair_node_values(ns.core, case.pairs.copy()).numpy(),
                                  np.where(ok, np.minimum(core[sa], core[sb]), -1))
    clus = pair_node_values(ns.clustering, torch.from_numpy(case.pairs.copy()), "max")
    assert clus.dtype == torch.float64 and (clus[torch.from_numpy(~ok)] == -1).all()
    comp = NC.reference("K")["component"]
    for edges in (torch.from_numpy(case.pairs.copy()), torch.from_numpy(case.pairs.T.copy())):
        same = same_component(ns, edges)
        assert same.dtype == torch.bool
        np.testing.assert_array_equal(same.numpy(), ok & (comp[sa] == comp[sb]))
    assert same.any() and not same.all()
    for bad in ("mean", None, 3):
        with pytest.raises(ValueError):
            pair_node_values(ns.core, case.pairs.copy(), bad)
    with pytest.raises(ValueError):
        pair_node_values(ns.core, torch.tensor([[0.5, 1.0], [2.0, 3.0]]))
    with pytest.raises(ValueError):
        pair_node_values(ns.core.view(2, -1), case.pairs.copy())
    assert pair_node_values(ns.core, torch.zeros(2, 0, dtype=torch.int64)).shape == (0,)


def test_bins_are_half_open_and_cover_every_value():
    for bins in (DEGREE_BINS, CORE_BINS):
        assert bins[0][0] == 0 and all(lo < hi for lo, hi in bins)
        assert all(bins[i][1] == bins[i + 1][0] for i in range(len(bins) - 1)) and bins[-1][1] >= (1 << 31)
    pos = torch.arange(8, dtype=torch.float32)
    neg = torch.zeros(16)
    rows = lpformer_amd.evaluate.metrics_by_bin(pos, neg, torch.tensor([0, 1, 2, 3, 7, 15, 63, 5000]), bins=CORE_BINS)
    assert len(rows) == len(CORE_BINS)


def test_argument_errors_come_before_any_device_use():
    csr = NC.graph_k().csr
    for bad in (("degree", "truss"), ("cores",), (), "triangle", (1,)):
        with pytest.raises(ValueError):
            node_structure(csr, kinds=bad)
        with pytest.raises(ValueError):
            structure_reference(csr, kinds=bad)
    for bad in (0, -1, True, 2.0, "8", None):
        with pytest.raises(ValueError):
            node_structure(csr, sweeps_per_read=bad)
    for bad in (0, -3, False, 1.5):
        with pytest.raises(ValueError):
            node_structure(csr, max_sweeps=bad)
    with pytest.raises(ValueError):
        node_structure(csr, hv_form="histogram")
    with pytest.raises(TypeError):
        node_structure("not a graph")
    with pytest.raises(TypeError):
        node_structure((csr, None))


def test_host_csr_without_a_gpu():
    """Through the public function where it takes the host path (no GPU present), else the restatement itself."""
    fn = structure_reference if torch.cuda.is_available() else node_structure
    case = NC.CASES["H"]()
    ns = fn(case.csr)
    for k in KINDS:
        t = getattr(ns, k)
        assert not t.is_cuda and t.dtype == (torch.int64 if k == "triangles" else torch.int32)
        np.testing.assert_array_equal(t.numpy(), NC.reference("H")[k])
    only = fn(case.csr, kinds=("component",))
    assert only.degree is None and only.core is None and only.triangles is None
    np.testing.assert_array_equal(only.component.numpy(), NC.reference("H")["component"])


def test_abi_registration_and_exports():
    assert _lib.ABI_VERSION == 16
    for name, n_args in SYMBOLS.items():
        assert len(_lib.HIP_PROTOTYPES[name]) == n_args and _lib.PROTOTYPES[name][0] is not None
    assert _lib.CONST["LPF_CORE_LONG_ROW"] == 64
    assert structure.HV_FORMS == {"default": _lib.CONST["LPF_CORE_FORM_DEFAULT"], "bisect": _lib.CONST["LPF_CORE_FORM_BISECT"]}
    hip = _lib.hip()                                                          # loads without a GPU
    for name in SYMBOLS:
        assert getattr(hip, name) is not None
    # bad arguments are refused before anything touches a device
    assert hip.lpf_node_degree(-1, 0, None, None, None, None) == -1
    assert hip.lpf_node_degree(5, 0, None, None, None, None) == -1
    assert hip.lpf_core_sweep(5, 0, None, None, None, 0, 0, None, None, None) == -1
    assert hip.lpf_components_hook(-1, 0, None, None, None, None, None) == -1
    assert hip.lpf_components_jump(3, None, None) == -1
    assert hip.lpf_node_triangles(3, 0, None, None, None, -1, None, None, None) == -1
    for name in ("node_structure", "NodeStructure", "structure_reference", "pair_node_values", "same_component",
                 "DEGREE_BINS", "CORE_BINS"):
        assert getattr(lpformer_amd, name) is getattr(structure, name) and name in lpformer_amd.__all__
    assert "node_structure" in lpformer_amd.__doc__
