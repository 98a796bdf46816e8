"""pair_walks / pair_katz (lpf_pair_walks: the meet-in-the-middle spread-and-walk kernel) on the MI355X against scipy's
A @ A row products on the host.  All walk-count comparisons are exact int64 equality; the Katz values are compared bit
for bit."""
import numpy as np
import pytest
import torch

from lpformer_amd import _lib, graph
from lpformer_amd.distance import pair_distance
from lpformer_amd.heuristics import pair_heuristics
from lpformer_amd.katz import katz_from_walks, pair_katz, pair_walks
from tests import pair_katz_cases as KC
from tests.golden_util import Fixture
from tests.test_gpu_pair_distance import _build

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _t(pairs):
    return torch.from_numpy(np.array(pairs, dtype=np.int64))


def _dev(name):
    case = KC.case(name)
    return case, case.csr.to_device(DEV), _t(case.pairs).to(DEV)


def _ref(name, ignore_direct=False, max_len=4):
    w = KC.exact_ignore_direct(name) if ignore_direct else KC.exact(name)
    return torch.from_numpy(w[:, :max_len].copy())


def _run(g, e, **kw):
    out = pair_walks(g, e, **kw)
    assert out.is_cuda and out.dtype == torch.int64 and out.shape == (max(e.shape), kw.get("max_len", 3))
    return out


@pytest.mark.parametrize("ignore_direct", [False, True])
@pytest.mark.parametrize("max_len", KC.MAX_LENS)
@pytest.mark.parametrize("name", ["S", "H", "C"])
def test_matches_scipy(name, max_len, ignore_direct):
    _, g, e = _dev(name)
    got = _run(g, e, max_len=max_len, ignore_direct=ignore_direct)
    assert torch.equal(got.cpu(), _ref(name, ignore_direct, max_len))


@pytest.mark.parametrize("name", ["S", "H", "C"])
def test_invariances(name):
    """groups=1: every unit through one workgroup's state (stale epochs); chunk=37: many launches on one workspace."""
    _, g, e = _dev(name)
    for ig in (False, True):
        ref = _ref(name, ig).to(DEV)
        w4 = _run(g, e, max_len=4, ignore_direct=ig)
        assert torch.equal(w4, ref)
        assert torch.equal(w4, _run(g, e, max_len=4, ignore_direct=ig))                        # two runs
        assert torch.equal(w4[:, :3], _run(g, e, max_len=3, ignore_direct=ig))
        assert torch.equal(w4, _run(g, e, max_len=4, ignore_direct=ig, groups=1))
        assert torch.equal(w4, _run(g, e, max_len=4, ignore_direct=ig, groups=5, chunk=300))
        assert torch.equal(w4, _run(g, e.flip(0), max_len=4, ignore_direct=ig))                # (b, a)
        assert torch.equal(w4, _run(g, e.t().contiguous(), max_len=4, ignore_direct=ig))       # [P, 2]
        perm = torch.randperm(e.shape[1], generator=torch.Generator().manual_seed(3)).to(DEV)
        assert torch.equal(w4[perm], _run(g, e[:, perm], max_len=4, ignore_direct=ig, groups=7))


def test_many_launches_on_one_workspace():
    _, g, e = _dev("H")
    assert torch.equal(_run(g, e, max_len=4, chunk=37), _ref("H").to(DEV))
    assert torch.equal(_run(g, e, max_len=4, chunk=37, ignore_direct=True, groups=3), _ref("H", True).to(DEV))


@pytest.mark.parametrize("name", ["S", "H", "C"])
def test_katz_is_bitwise_the_host_arithmetic(name):
    case, g, e = _dev(name)
    for beta, L in ((0.005, 3), (0.05, 4), (0.3, 2)):
        got = pair_katz(g, e, beta=beta, max_len=L)
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == (e.shape[1],)
        want = katz_from_walks(_ref(name, False, L), beta)
        assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))
    assert torch.equal(pair_katz(g, e, ignore_direct=True).cpu().view(torch.int32),
                       katz_from_walks(_ref(name, True, 3), 0.005).view(torch.int32))
    assert torch.equal(pair_katz(case.csr, _t(case.pairs)).cpu(), katz_from_walks(_ref(name, False, 3), 0.005))


@pytest.mark.parametrize("name", ["S", "H", "C"])
def test_against_common_neighbours_and_distance(name):
    case, g, e = _dev(name)
    w = _run(g, e, max_len=4)
    cn = pair_heuristics(g, e, kinds=("cn",))["cn"]
    differ = e[0] != e[1]
    assert torch.equal(w[differ, 1], cn[differ].to(torch.int64)) and int(cn[differ].max()) > 0
    d = pair_distance(g, e, max_dist=4)
    ok = ((e >= 0) & (e < case.n)).all(dim=0)
    for k in (1, 2, 3, 4):
        at = (d == k) & ok
        assert int(at.sum()) > 0 or name == "C"                  # (C's batch need not hold every distance)
        assert (w[at, :k - 1] == 0).all() and (w[at, k - 1] >= 1).all()
    assert (w[(d == -1) & ok] == 0).all()                                     # farther than 4 hops, or no path


def test_model_source_equals_its_adjacency():
    fx = Fixture("lp_all_d64_residual_valtest")
    model = _build(fx)
    rng = np.random.default_rng(2)
    e = _t(np.concatenate([fx["batch"].astype(np.int64), rng.integers(0, fx.n, size=(2, 500))], axis=1))
    for test_set, key in ((False, "edge_index"), (True, "full_edge_index")):
        csr = graph.mask_csr(fx[key].astype(np.int64), fx.n, symmetric=True)
        got = pair_walks(model, e, test_set=test_set, max_len=4)
        assert torch.equal(got, pair_walks(csr, e.to(DEV), max_len=4)) and int(got[:, 2].max()) > 0
        A = KC.PC._adjacency(np.repeat(np.arange(fx.n), np.diff(csr.rowptr)), csr.col.astype(np.int64), fx.n)
        np.testing.assert_array_equal(got.cpu().numpy(), KC.scipy_walks(A, e.numpy()))


def test_empty_batches():
    _, g, _ = _dev("S")
    for empty in (torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0, 2, dtype=torch.int64, device=DEV)):
        w = pair_walks(g, empty, max_len=4)
        assert w.is_cuda and w.dtype == torch.int64 and w.shape == (0, 4)
        k = pair_katz(g, empty)
        assert k.is_cuda and k.dtype == torch.float32 and k.shape == (0,)


def test_c_entry_rejects_bad_options_without_a_launch():
    _, g, e = _dev("S")
    hip = _lib.hip()
    m = 8
    pairs = e[:, :m].contiguous()
    unit_ptr = torch.arange(m + 1, dtype=torch.int32, device=DEV)
    ws = torch.zeros(int(hip.lpf_pair_walks_workspace_bytes(g.n, 1)), dtype=torch.uint8, device=DEV)
    out = torch.full((m, 4), -7, dtype=torch.int64, device=DEV)

    def call(max_len, n_groups, workspace=ws):
        return hip.lpf_pair_walks(m, g.n, pairs.data_ptr(), m, g.rowptr.data_ptr(), g.col.data_ptr(), max_len, 0,
                                  unit_ptr.data_ptr(), workspace.data_ptr() if workspace is not None else None,
                                  n_groups, out.data_ptr(), 0)
    assert call(5, 1) == -1 and call(0, 1) == -1 and call(3, 0) == -1 and call(3, 65536) == -1
    assert call(3, 1, None) == -1
    torch.cuda.synchronize()
    assert (out == -7).all()                                                  # nothing ran
    assert call(4, 1) == 0                                                    # the same arguments, valid: one-pair units
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), _ref("S")[:m])
