"""node_structure (the kernels of csrc/node_structure.hip) on the MI355X against the numpy / scipy restatement and the
hand cases.  Every comparison is exact integer equality."""
import numpy as np
import pytest
import torch

from lpformer_amd import _lib, graph
from lpformer_amd.distance import pair_distance
from lpformer_amd.heuristics import pair_heuristics
from lpformer_amd.structure import KINDS, node_structure, pair_node_values, same_component, structure_reference
from tests import node_structure_cases as NC
from tests.golden_util import Fixture
from tests.test_gpu_pair_distance import _build

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = {"degree": torch.int32, "core": torch.int32, "component": torch.int32, "triangles": torch.int64}


def _case(name):
    return NC.graph_k_loops() if name == "Kloops" else NC.CASES[name]()


def _dev(name):
    case = _case(name)
    return case, case.csr.to_device(DEV)


def _check(ns, ref, kinds=KINDS):
    for k in KINDS:
        t = getattr(ns, k)
        if k not in kinds:
            assert t is None, k
            continue
        assert t.is_cuda and t.dtype == DTYPES[k] and t.shape == (ns.n,), k
        np.testing.assert_array_equal(t.cpu().numpy(), ref[k], err_msg=k)


@pytest.mark.parametrize("name", NC.NAMES + ("Kloops",))
def test_matches_the_restatement(name):
    _, g = _dev(name)
    ns = node_structure(g)
    print(name, "launches:", ns.sweeps)
    _check(ns, NC.reference(name))
    assert set(ns.sweeps) == {"core", "component"} and ns.n == g.n


@pytest.mark.parametrize("hand", NC.hand_cases(), ids=lambda h: h.what)
def test_matches_the_hand_cases(hand):
    ns = node_structure(hand.csr.to_device(DEV))
    for k in KINDS:
        assert getattr(ns, k).tolist() == hand.want[k], k
    for spr in (1, 64):
        again = node_structure(hand.csr.to_device(DEV), sweeps_per_read=spr, hv_form="bisect", split_threshold=0)
        for k in KINDS:
            assert getattr(again, k).tolist() == hand.want[k], k


def test_each_kind_alone_and_the_self_loop_variant():
    _, g = _dev("K")
    _, loops = _dev("Kloops")
    ref = NC.reference("K")
    for k in KINDS:
        _check(node_structure(g, kinds=(k,)), ref, (k,))
        _check(node_structure(loops, kinds=k), ref, (k,))
    _check(node_structure(g, kinds=("triangles", "degree")), ref, ("degree", "triangles"))
    both = node_structure(loops)
    _check(both, ref)
    want = structure_reference(_case("K").csr).clustering
    np.testing.assert_array_equal(both.clustering.cpu().numpy(), want.numpy())


@pytest.mark.parametrize("name", ("P", "H", "K"))
def test_sweeps_per_read_changes_no_tensor(name):
    """The launches recorded (no-op launches behind the converged one included) are at least the changing sweeps the
    synchronous iteration needs on the graph's free-hanging path (tests/node_structure_cases.SWEEP_BOUND)."""
    _, g = _dev(name)
    ref = NC.reference(name)
    for spr in (1, 3, 8, 64):
        ns = node_structure(g, kinds=("core", "component"), sweeps_per_read=spr)
        print(name, "sweeps_per_read", spr, "launches:", ns.sweeps)
        _check(ns, ref, ("core", "component"))
        assert ns.sweeps["core"] >= 1 and ns.sweeps["component"] >= 1
        if name in NC.SWEEP_BOUND:
            assert ns.sweeps["core"] >= NC.SWEEP_BOUND[name]


def test_max_sweeps_raises_and_leaves_nothing_behind():
    _, g = _dev("P")
    for spr in (1, 8):
        with pytest.raises(_lib.LpfError, match="not converged"):
            node_structure(g, kinds=("core",), max_sweeps=2, sweeps_per_read=spr)
    _check(node_structure(g), NC.reference("P"))
    _check(node_structure(g, max_sweeps=5000), NC.reference("P"))


@pytest.mark.parametrize("name", ("H", "C", "K"))
def test_two_runs_and_both_row_forms_give_the_same_bits(name):
    _, g = _dev(name)
    a, b = node_structure(g), node_structure(g)
    c = node_structure(g, hv_form="bisect", split_threshold=0)
    d = node_structure(g, split_threshold=1 << 20)
    for k in KINDS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
        assert torch.equal(getattr(a, k), getattr(c, k)) and torch.equal(getattr(a, k), getattr(d, k)), k
    _check(c, NC.reference(name))


def test_model_source_equals_its_adjacency():
    fx = Fixture("lp_all_d64_residual_valtest")
    model = _build(fx)
    seen = []
    for test_set, key in ((False, "edge_index"), (True, "full_edge_index")):
        csr = graph.mask_csr(fx[key].astype(np.int64), fx.n, symmetric=True)
        ns = node_structure(model, test_set=test_set)
        ref = structure_reference(csr)
        _check(ns, {k: getattr(ref, k).numpy() for k in KINDS})
        _check(node_structure(csr), {k: getattr(ref, k).numpy() for k in KINDS})      # a host CSR is uploaded
        seen.append(ns)
    assert not torch.equal(seen[0].degree, seen[1].degree)                            # the two splits' adjacencies differ


def test_node_permutation():
    case = _case("K")
    pcase, perm = NC.permuted(case)
    ref = NC.reference("K")
    ns = node_structure(pcase.csr.to_device(DEV))
    p = torch.from_numpy(perm).to(DEV)
    for k in ("degree", "core", "triangles"):
        np.testing.assert_array_equal(getattr(ns, k)[p].cpu().numpy(), ref[k], err_msg=k)
    # the partition is the permuted partition, each label the smallest NEW id of its part
    label = ns.component[p].cpu().numpy()
    want = np.full(case.n, case.n, np.int64)
    np.minimum.at(want, ref["component"], perm)
    np.testing.assert_array_equal(label, want[ref["component"]])


def test_same_component_against_pair_distance():
    case, g = _dev("H")
    e = torch.from_numpy(case.pairs.copy()).to(DEV)
    ns = node_structure(g, kinds=("component", "degree"))
    same = same_component(ns, e)
    assert same.is_cuda and same.dtype == torch.bool
    assert torch.equal(same, pair_distance(g, e) >= 0) and same.any() and not same.all()
    assert torch.equal(same, same_component(ns, e.t().contiguous()))
    v = pair_node_values(ns.degree, e, "max")
    assert v.is_cuda and torch.equal(v, torch.maximum(ns.degree[e[0]], ns.degree[e[1]]))


def test_triangles_against_pair_heuristics():
    case, g = _dev("K")
    coo = case.A.tocoo()
    e = torch.from_numpy(np.stack([coo.row, coo.col]).astype(np.int64)).to(DEV)
    cn = pair_heuristics(g, e, kinds=("cn",))["cn"].to(torch.int64)
    tri = node_structure(g, kinds=("triangles",)).triangles
    assert int(tri.sum()) * 2 == int(cn.sum()) and int(tri.sum()) > 0
    # per node as well: the triangles through u are half the common neighbours over its row
    per_node = torch.zeros(case.n, dtype=torch.int64, device=DEV).index_add_(0, e[0], cn)
    assert torch.equal(tri * 2, per_node)


def test_c_entries_reject_bad_arguments_without_a_launch():
    case, g = _dev("S")
    hip = _lib.hip()
    n, nnz = g.n, g.nnz
    deg = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    slot = torch.zeros(1, dtype=torch.int32, device=DEV)
    rp, col = g.rowptr.data_ptr(), g.col.data_ptr()
    assert hip.lpf_node_degree(-1, nnz, rp, col, deg.data_ptr(), 0) == -1
    assert hip.lpf_node_degree(n, -1, rp, col, deg.data_ptr(), 0) == -1
    assert hip.lpf_node_degree(n, nnz, None, col, deg.data_ptr(), 0) == -1
    assert hip.lpf_node_degree(n, nnz, rp, None, deg.data_ptr(), 0) == -1
    assert hip.lpf_node_degree(n, nnz, rp, col, None, 0) == -1
    assert hip.lpf_core_sweep(n, nnz, rp, col, None, 1, 0, deg.data_ptr(), slot.data_ptr(), 0) == -1   # list missing
    assert hip.lpf_core_sweep(n, nnz, rp, col, None, 0, 7, deg.data_ptr(), slot.data_ptr(), 0) == -1   # unknown form
    assert hip.lpf_core_sweep(n, nnz, rp, col, None, 0, 0, deg.data_ptr(), None, 0) == -1
    assert hip.lpf_components_hook(n, nnz, None, col, deg.data_ptr(), slot.data_ptr(), 0) == -1
    assert hip.lpf_components_jump(-1, deg.data_ptr(), 0) == -1
    assert hip.lpf_node_triangles(n, nnz, rp, col, col, -1, None, deg.data_ptr(), 0) == -1
    assert hip.lpf_node_degree(0, 0, rp, col, deg.data_ptr(), 0) == 0                  # n == 0: LPF_OK, no launch
    assert hip.lpf_components_jump(0, deg.data_ptr(), 0) == 0
    torch.cuda.synchronize()
    assert (deg == -7).all() and int(slot) == 0                                       # nothing ran
    assert hip.lpf_node_degree(n, nnz, rp, col, deg.data_ptr(), 0) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(deg.cpu().numpy(), NC.reference("S")["degree"])
    empty = node_structure(graph.CSR(np.zeros(1, np.int64), np.zeros(0, np.int32), None, 0).to_device(DEV))
    assert all(getattr(empty, k).shape == (0,) and getattr(empty, k).dtype == DTYPES[k] for k in KINDS)
