"""pair_hop_counts (lpf_pair_hop_counts: the spread-and-expand kernel of pair_hops.hip) on the MI355X against scipy's
shortest paths on the host and the hand cases.  Every comparison is exact integer equality."""
import numpy as np
import pytest
import torch

from lpformer_amd import _lib, graph
from lpformer_amd.distance import pair_distance
from lpformer_amd.heuristics import pair_heuristics
from lpformer_amd.hops import ball_jaccard, elph_features, hop_counts_reference, pair_hop_counts
from tests import pair_hops_cases as HC
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


def _ref(name, k=2, ignore_direct=False):
    return torch.from_numpy(HC.exact(name, k, ignore_direct).copy())


def _run(g, e, **kw):
    out = pair_hop_counts(g, e, **kw)
    k = kw.get("hops", 2)
    assert out.is_cuda and out.dtype == torch.int32 and out.shape == (max(e.shape), k + 2, k + 2)
    return out


@pytest.mark.parametrize("ignore_direct", [False, True])
@pytest.mark.parametrize("k", HC.HOPS)
@pytest.mark.parametrize("name", HC.NAMES)
def test_matches_scipy(name, k, ignore_direct):
    _, g, e = _dev(name)
    got = _run(g, e, hops=k, ignore_direct=ignore_direct)
    assert torch.equal(got.cpu(), _ref(name, k, ignore_direct))


@pytest.mark.parametrize("hand", HC.hand_cases(), ids=lambda h: h.what)
def test_matches_the_hand_cases(hand):
    g, e = hand.csr.to_device(DEV), _t(hand.pairs).to(DEV)
    want = torch.from_numpy(hand.tables.copy())
    for kw in ({}, {"groups": 1}, {"chunk": 1}):
        assert torch.equal(_run(g, e, hops=hand.hops, ignore_direct=hand.ignore_direct, **kw).cpu(), want)
    assert torch.equal(_run(g, e.flip(0), hops=hand.hops, ignore_direct=hand.ignore_direct).cpu(),
                       want.transpose(1, 2))


@pytest.mark.parametrize("name", HC.NAMES)
def test_invariances(name):
    """groups=1: every unit and every pair through one workgroup's state (stale epochs in both arrays); chunk=37: many
    launches on one workspace."""
    _, g, e = _dev(name)
    for k, ig in ((2, False), (2, True), (1, True)):
        ref = _ref(name, k, ig).to(DEV)
        t = _run(g, e, hops=k, ignore_direct=ig)
        assert torch.equal(t, ref)
        assert torch.equal(t, _run(g, e, hops=k, ignore_direct=ig))                            # two runs
        assert torch.equal(t, _run(g, e, hops=k, ignore_direct=ig, groups=1))
        assert torch.equal(t, _run(g, e, hops=k, ignore_direct=ig, groups=5, chunk=300))
        assert torch.equal(t, _run(g, e, hops=k, ignore_direct=ig, chunk=37))
        assert torch.equal(t.transpose(1, 2), _run(g, e.flip(0), hops=k, ignore_direct=ig))    # (b, a)
        assert torch.equal(t, _run(g, e.t().contiguous(), hops=k, ignore_direct=ig))           # [P, 2]
        perm = torch.randperm(e.shape[1], generator=torch.Generator().manual_seed(3)).to(DEV)
        assert torch.equal(t[perm], _run(g, e[:, perm], hops=k, ignore_direct=ig, groups=7))


@pytest.mark.parametrize("name", HC.NAMES)
def test_against_pair_distance_and_common_neighbours(name):
    """T[0][j] has its single 1 at j = min(dist, k + 1), dist -1 mapped to k + 1 (ignore_direct off and on); T[1][1] is
    pair_heuristics' CN for a != b."""
    case, g, e = _dev(name)
    ok = ((e >= 0) & (e < case.n)).all(dim=0)
    rows = torch.arange(e.shape[1], device=DEV)
    for ig in (False, True):
        d = pair_distance(g, e, ignore_direct=ig).long()
        for k in HC.HOPS:
            t = _run(g, e, hops=k, ignore_direct=ig)
            at = torch.where((d < 0) | (d > k), torch.full_like(d, k + 1), d)
            want = torch.zeros((e.shape[1], k + 2), dtype=torch.int32, device=DEV)
            want[rows[ok], at[ok]] = 1
            assert torch.equal(t[:, 0, :], want) and torch.equal(t[:, :, 0], want)
    cn = pair_heuristics(g, e, kinds=("cn",))["cn"]
    differ = ok & (e[0] != e[1])
    for k in HC.HOPS:
        assert torch.equal(_run(g, e, hops=k)[differ, 1, 1].long(), cn[differ].long())
    assert int(cn[differ].max()) > 0


def test_model_source_equals_its_adjacency():
    fx = Fixture("lp_all_d64_residual_valtest")
    model = _build(fx)
    rng = np.random.default_rng(2)
    e = _t(np.concatenate([fx["batch"].astype(np.int64), rng.integers(0, fx.n, size=(2, 500))], axis=1))
    seen = []
    for test_set, key in ((False, "edge_index"), (True, "full_edge_index")):
        csr = graph.mask_csr(fx[key].astype(np.int64), fx.n, symmetric=True)
        for k in HC.HOPS:
            got = pair_hop_counts(model, e, test_set=test_set, hops=k)
            assert got.is_cuda and got.dtype == torch.int32
            assert torch.equal(got.cpu(), hop_counts_reference(csr, e, hops=k))
            assert int(got[:, 1, 1].max()) > 0 and (got.sum(dim=(1, 2)) == fx.n).all()
        seen.append(got)
        got = pair_hop_counts(model, e, test_set=test_set, ignore_direct=True)
        assert torch.equal(got.cpu(), hop_counts_reference(csr, e, ignore_direct=True))
    assert not torch.equal(seen[0], seen[1])                                  # the two splits' adjacencies differ


def test_features_on_the_device_and_host_csr_source():
    case, g, e = _dev("H")
    t = _run(g, e)
    assert torch.equal(_run(case.csr, _t(case.pairs)), t)                     # a host CSR is uploaded: device result
    f, j = elph_features(t), ball_jaccard(t)
    assert f.is_cuda and f.shape == (e.shape[1], 8) and j.is_cuda and j.dtype == torch.float32
    assert torch.equal(f.cpu(), elph_features(_ref("H"))) and torch.equal(j.cpu(), ball_jaccard(_ref("H")))


def test_empty_batches():
    _, g, _ = _dev("S")
    for empty in (torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0, 2, dtype=torch.int64, device=DEV)):
        for k in HC.HOPS:
            t = pair_hop_counts(g, empty, hops=k)
            assert t.is_cuda and t.dtype == torch.int32 and t.shape == (0, k + 2, k + 2)
        assert elph_features(pair_hop_counts(g, empty)).shape == (0, 8)
        assert ball_jaccard(pair_hop_counts(g, empty)).shape == (0,)


def test_c_entry_rejects_bad_options_without_a_launch():
    _, g, e = _dev("S")
    hip = _lib.hip()
    m = 8
    pairs = e[:, :m].contiguous()
    unit_ptr = torch.arange(m + 1, dtype=torch.int32, device=DEV)
    assert hip.lpf_pair_hop_counts_workspace_bytes(g.n, 3) == 16 + 3 * 8 * g.n
    assert hip.lpf_pair_hop_counts_workspace_bytes(g.n, 0) == 0 and hip.lpf_pair_hop_counts_workspace_bytes(0, 3) == 0
    ws = torch.zeros(int(hip.lpf_pair_hop_counts_workspace_bytes(g.n, 1)), dtype=torch.uint8, device=DEV)
    out = torch.full((m, 4, 4), -7, dtype=torch.int32, device=DEV)

    def call(hops, n_groups, workspace=ws, m=m):
        return hip.lpf_pair_hop_counts(m, g.n, pairs.data_ptr(), 8, g.rowptr.data_ptr(), g.col.data_ptr(), hops, 0,
                                       unit_ptr.data_ptr(), workspace.data_ptr() if workspace is not None else None,
                                       n_groups, out.data_ptr(), 0)
    assert call(0, 1) == -1 and call(3, 1) == -1 and call(2, 0) == -1 and call(2, 65536) == -1
    assert call(0, 1, m=0) == -1 and call(2, 0, m=0) == -1                    # options are checked first
    assert call(2, 1, None) == -1
    assert call(2, 1, m=0) == 0 and call(2, 1, None, m=0) == 0                # m == 0: LPF_OK, no launch
    torch.cuda.synchronize()
    assert (out == -7).all()                                                  # nothing ran
    assert call(2, 1) == 0                                                    # the same arguments, valid: one-pair units
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), _ref("S")[:m])
