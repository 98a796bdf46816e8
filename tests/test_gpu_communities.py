"""communities (the kernels of csrc/community.hip) on the MI355X against the numpy restatement and the hand cases.
Every comparison is exact integer equality."""
import numpy as np
import pytest
import torch

from lpformer_amd import _lib, graph
from lpformer_amd.community import (communities, communities_reference, move_round_reference, partition_quality,
                                    quality_reference, same_community)
from lpformer_amd.structure import entry_rows, node_structure
from tests import communities_cases as CC
from tests import node_structure_cases as NC
from tests.golden_util import Fixture
from tests.test_gpu_pair_distance import _build

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# what the comparison is repeated with: the device-memory table on every listed row, another seed, levels cut short by
# max_rounds, one level only
VARIANTS = {"default": {}, "global_table": {"lds_slots": 64}, "seed1": {"seed": 1}, "two_rounds": {"max_rounds": 2},
            "one_level": {"max_levels": 1}}


def _dev(name):
    case = CC.CASES[name]()
    return case, case.csr.to_device(DEV)


def _same(c, ref):
    assert c.label.is_cuda and c.label.dtype == torch.int32 and c.label.shape == (ref.n,)
    np.testing.assert_array_equal(c.label.cpu().numpy(), ref.label.numpy())
    assert c.levels == ref.levels and len(c.hierarchy) == len(ref.hierarchy)
    for got, want in zip(c.hierarchy, ref.hierarchy):
        assert got.is_cuda and got.dtype == torch.int32
        np.testing.assert_array_equal(got.cpu().numpy(), want.numpy())
    assert (c.n, c.count, c.two_m, c.quality_num, c.modularity) == \
        (ref.n, ref.count, ref.two_m, ref.quality_num, ref.modularity)
    assert isinstance(c.quality_num, int) and isinstance(c.count, int)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", CC.NAMES)
def test_matches_the_restatement(name, variant):
    _, g = _dev(name)
    kw = VARIANTS[variant]
    ref_kw = {k: v for k, v in kw.items() if k != "lds_slots"}
    c = communities(g, **kw)
    print(name, variant, "communities", c.count, "levels", c.levels)
    _same(c, CC.reference(name, **ref_kw))


@pytest.mark.parametrize("hand", CC.hand_cases(), ids=lambda h: h.what)
def test_matches_the_hand_cases(hand):
    for kw in VARIANTS.values():
        c = communities(hand.csr.to_device(DEV), **kw)
        assert c.label.tolist() == hand.label and c.count == hand.count, kw
    _same(communities(hand.csr.to_device(DEV)), communities_reference(hand.csr))


@pytest.mark.parametrize("name", ("H", "K", "D"))
def test_two_runs_and_both_tables_give_the_same_bits(name):
    _, g = _dev(name)
    a, b, c = communities(g), communities(g), communities(g, lds_slots=64)
    d = communities(g, lds_slots=8192)
    for other in (b, c, d):
        assert torch.equal(a.label, other.label) and a.levels == other.levels
        assert all(torch.equal(x, y) for x, y in zip(a.hierarchy, other.hierarchy))


def test_model_source_equals_its_adjacency():
    fx = Fixture("lp_all_d64_residual_valtest")
    model = _build(fx)
    seen = []
    for test_set, key in ((False, "edge_index"), (True, "full_edge_index")):
        csr = graph.mask_csr(fx[key].astype(np.int64), fx.n, symmetric=True)
        c = communities(model, test_set=test_set)
        ref = communities_reference(csr)
        _same(c, ref)
        _same(communities(csr), ref)                                                  # a host CSR is uploaded
        assert partition_quality(model, c.label, test_set=test_set) == (ref.quality_num, ref.two_m)
        seen.append(c)
    assert seen[0].two_m != seen[1].two_m                                             # the two splits' adjacencies differ


@pytest.mark.parametrize("name", ("K", "Kloops", "H", "D"))
def test_partition_quality(name):
    case, g = _dev(name)
    c = communities(g)
    assert partition_quality(g, c.label) == (c.quality_num, c.two_m)
    for lv, h in zip(c.levels, c.hierarchy):
        assert partition_quality(g, h) == (lv["quality_num"], c.two_m)
    # any labelling: the components, as node_structure names them, against numpy
    comp = node_structure(g, kinds=("component",)).component
    A = case.A.copy()
    A.setdiag(0)
    A.eliminate_zeros()
    degree = np.diff(A.indptr).astype(np.int64)
    want = quality_reference(A.indptr, A.indices, None, None, degree, comp.cpu().numpy())
    assert partition_quality(g, comp) == (want, int(degree.sum()))
    assert partition_quality(g, comp.cpu().numpy().astype(np.int64) * 3 - 7) == (want, int(degree.sum()))   # labels are names
    assert partition_quality(case.csr, comp.cpu()) == (want, int(degree.sum()))


def test_same_community_against_a_numpy_gather():
    case, g = _dev("D")
    c = communities(g)
    label = c.label.cpu().numpy()
    a, b = case.pairs
    ok = (a >= 0) & (a < case.n) & (b >= 0) & (b < case.n)
    assert int((~ok).sum()) == 4
    want = ok & (label[np.where(ok, a, 0)] == label[np.where(ok, b, 0)])
    e = torch.from_numpy(case.pairs.copy()).to(DEV)
    for edges in (e, e.t().contiguous(), case.pairs.copy()):
        same = same_community(c, edges)
        assert same.is_cuda and same.dtype == torch.bool
        np.testing.assert_array_equal(same.cpu().numpy(), want)
    assert want.any() and not want.all()
    sizes = np.bincount(label, minlength=case.n)
    assert c.size.is_cuda and np.array_equal(c.size.cpu().numpy(), sizes[label])
    assert c.summary()["communities"] == c.count == 11


class _Launches:
    """A recorder (``_lib.recording``) that counts the C entry points fetched."""

    def __init__(self):
        self.names = []

    def launch(self, name, fn):
        self.names.append(name)
        return fn

    def keep(self, t):
        pass

    def wait(self, a, b):
        pass


def test_empty_graphs_launch_nothing():
    for n in (0, 7):
        g = graph.CSR(np.zeros(n + 1, np.int64), np.zeros(0, np.int32), None, n).to_device(DEV)
        with _lib.recording(_Launches()) as rec:
            c = communities(g)
            q = partition_quality(g, torch.zeros(n, dtype=torch.int64))
        assert rec.names == [] and q == (0, 0)
        assert c.label.is_cuda and c.label.dtype == torch.int32 and c.label.tolist() == list(range(n))
        assert (c.count, c.two_m, c.quality_num, c.modularity, c.levels, c.hierarchy) == (n, 0, 0, 0.0, [], [])
    # stored self-loops only: the degree is asked for, then nothing moves
    loops = graph.CSR(np.arange(5, dtype=np.int64), np.arange(4, dtype=np.int32), None, 4).to_device(DEV)
    with _lib.recording(_Launches()) as rec:
        c = communities(loops)
    assert rec.names == ["lpf_node_degree"] and c.label.tolist() == [0, 1, 2, 3] and c.two_m == 0


@pytest.mark.parametrize("lds_slots", (4096, 64))
def test_one_weighted_round_called_directly(lds_slots):
    """A level-1 shape made by hand on K's pattern (int64 weights, self weights in k, a non-trivial comm with
    singletons): lpf_community_move against the restatement's single-round function, so that the weighted path is
    pinned without relying on what level 0 happens to produce."""
    case = NC.graph_k()
    lv = CC.weighted_level(case)
    n, nnz = case.n, int(lv["indices"].size)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in lv.items() if k != "two_m"}
    lens = np.diff(lv["indptr"])
    long_rows = torch.from_numpy(np.nonzero(lens > 64)[0].astype(np.int32)).to(DEV)
    assert long_rows.numel() > 100 and (lens <= 64).sum() > 100
    hip = _lib.hip()
    nbytes = hip.lpf_community_workspace_bytes(long_rows.numel(), int(lens.max()), lds_slots)
    assert (nbytes > 0) == (lds_slots == 64)
    scratch = torch.zeros(max(nbytes, 1), dtype=torch.uint8, device=DEV)
    for seed, level, rnd in ((0, 1, 0), (9, 3, 17)):
        new = torch.full((n,), -7, dtype=torch.int32, device=DEV)
        moved = torch.zeros(1, dtype=torch.int32, device=DEV)
        rc = hip.lpf_community_move(n, nnz, t["indptr"].data_ptr(), t["indices"].data_ptr(), t["weight"].data_ptr(),
                                    t["k"].data_ptr(), t["comm"].data_ptr(), t["tot"].data_ptr(), t["cnt"].data_ptr(),
                                    lv["two_m"], seed, level, rnd, long_rows.data_ptr(), long_rows.numel(), lds_slots,
                                    scratch.data_ptr() if nbytes else None, nbytes, new.data_ptr(), moved.data_ptr(), 0)
        assert rc == 0
        torch.cuda.synchronize()
        want = move_round_reference(lv["indptr"], lv["indices"], lv["weight"], lv["k"], lv["comm"], lv["tot"],
                                    lv["cnt"], lv["two_m"], seed, level, rnd)
        np.testing.assert_array_equal(new.cpu().numpy(), want)
        n_moved = int((want != lv["comm"]).sum())
        assert int(moved) == n_moved and n_moved > 100
        assert int(scratch.count_nonzero()) == 0                                      # the tables are left all zero
    # the inside weight of that comm, weights and all
    inside = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    rows = entry_rows(case.csr.to_device(DEV))
    assert hip.lpf_community_quality(n, nnz, rows.data_ptr(), t["indices"].data_ptr(), t["weight"].data_ptr(),
                                     t["comm"].data_ptr(), inside.data_ptr(), 0) == 0
    r = np.repeat(np.arange(n), lens)
    same = (r != lv["indices"]) & (lv["comm"][r] == lv["comm"][lv["indices"]])
    assert int(inside) == int(lv["weight"][same].sum()) > 0


def test_c_entries_reject_bad_arguments_without_a_launch():
    case, g = _dev("R")
    hip = _lib.hip()
    n, nnz = g.n, g.nnz
    k = torch.ones(n, dtype=torch.int64, device=DEV)
    comm = torch.arange(n, dtype=torch.int32, device=DEV)
    cnt = torch.ones(n, dtype=torch.int32, device=DEV)
    new = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    moved = torch.zeros(1, dtype=torch.int32, device=DEV)

    def move(n=n, rowptr=g.rowptr.data_ptr(), two_m=100, long_rows=None, n_long=0, lds_slots=64, scratch=None,
             scratch_bytes=0, new_p=new.data_ptr(), moved_p=moved.data_ptr(), level=0, rnd=0):
        return hip.lpf_community_move(n, nnz, rowptr, g.col.data_ptr(), None, k.data_ptr(), comm.data_ptr(),
                                      k.data_ptr(), cnt.data_ptr(), two_m, 0, level, rnd, long_rows, n_long, lds_slots,
                                      scratch, scratch_bytes, new_p, moved_p, 0)
    assert move(n=-1) == -1 and move(rowptr=None) == -1 and move(new_p=None) == -1 and move(moved_p=None) == -1
    assert move(two_m=1 << 31) == -1 and move(two_m=-1) == -1 and move(level=-1) == -1 and move(rnd=-1) == -1
    assert move(n_long=1) == -1 and move(n_long=-1) == -1                             # list missing / negative
    for bad in (0, 63, 96, 16384, -64):
        assert move(lds_slots=bad) == -1
    assert move(scratch_bytes=64) == -1 and move(scratch_bytes=-1) == -1              # bytes without a pointer
    assert move(n=0) == 0                                                             # n == 0: LPF_OK, no launch
    torch.cuda.synchronize()
    assert (new == -7).all() and int(moved) == 0                                      # nothing ran
    inside = torch.full((1,), -3, dtype=torch.int64, device=DEV)
    assert hip.lpf_community_quality(n, nnz, None, g.col.data_ptr(), None, comm.data_ptr(), inside.data_ptr(), 0) == -1
    assert hip.lpf_community_quality(n, nnz, g.col.data_ptr(), g.col.data_ptr(), None, comm.data_ptr(), None, 0) == -1
    torch.cuda.synchronize()
    assert int(inside) == -3
