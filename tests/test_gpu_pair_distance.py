"""pair_distance (lpf_pair_bfs: front kernel + bidirectional BFS search kernel) on the MI355X against scipy's unweighted
shortest_path on the host.  All comparisons are exact int32 equality."""
import numpy as np
import pytest
import torch

import lpformer_amd
from lpformer_amd import graph
from lpformer_amd.distance import distance_reference, pair_distance
from tests import pair_distance_cases as PC
from tests.golden_util import Fixture

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _build(fx):
    """Model on cuda:0 from a fixture, graph entries as torch sparse COO tensors (tests/test_gpu_heuristics.py)."""
    n = fx.n
    data = {"x": torch.from_numpy(fx["x"]).to(DEV), "num_nodes": n}

    def pack(ei_key, w_key, ppr_prefix):
        ei = fx[ei_key].astype(np.int64)
        adj_t = graph.csr_from_coo(ei[0], ei[1], fx[w_key], n)
        mask = graph.mask_csr(ei, n, symmetric=True)
        ppr = graph.csr_from_coo(fx[ppr_prefix + "row"], fx[ppr_prefix + "col"], fx[ppr_prefix + "val"], n)
        return adj_t.to_torch_sparse_coo().to(DEV), mask.to_torch_sparse_coo().to(DEV).int(), \
            ppr.to_torch_sparse_coo().to(DEV)

    data["adj_t"], data["adj_mask"], data["ppr"] = pack("edge_index", "edge_weight", "ppr_")
    if fx.test_set:
        data["full_adj_t"], data["full_adj_mask"], data["ppr_test"] = pack("full_edge_index", "full_edge_weight",
                                                                            "ppr_test_")
    else:
        data["full_adj_t"], data["full_adj_mask"], data["ppr_test"] = data["adj_t"], data["adj_mask"], data["ppr"]
    cfg = {k: fx.cfg[k] for k in ("thresh_cn", "thresh_1hop", "thresh_non1hop", "dim", "trans_layers", "num_heads",
                                  "att_drop", "dropout", "gnn_drop", "feat_drop", "gcn_cache", "gnn_layers",
                                  "residual", "layer_norm", "relu")}
    model = lpformer_amd.LinkTransformer(cfg, data, device=DEV).to(DEV)
    m_sd, _ = fx.state_dicts()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in m_sd.items()}, strict=True)
    return model.eval()


def _t(pairs):
    return torch.from_numpy(np.array(pairs, dtype=np.int64))


def _dev(name):
    case = PC.CASES[name]()
    return case, case.csr.to_device(DEV), _t(case.pairs).to(DEV)


def _run(g, e, **kw):
    out = pair_distance(g, e, **kw)
    assert out.is_cuda and out.dtype == torch.int32 and out.dim() == 1
    return out.cpu().numpy()


@pytest.mark.parametrize("groups", [1, 7, None])
@pytest.mark.parametrize("thr", [0, -1, 1 << 30])
@pytest.mark.parametrize("name", ["S", "H", "C"])
def test_matches_scipy(name, thr, groups):
    """groups=1: every listed pair through one workgroup's stamps (stale epochs); thr=0: every distance-2 candidate
    through the search kernel; thr=1<<30: every one through the front kernel."""
    case, g, e = _dev(name)
    ref = PC.exact(name)
    if name == "S":
        assert set(range(-1, 16)) <= set(ref.tolist()) and (ref == -1).sum() == 739
    elif name == "H":
        deg = np.diff(case.A.indptr)                # 64: the farthest drawn pair (the graph's largest distance is 69)
        assert deg[list(PC.HUBS)].min() > 256 and (ref == -1).sum() == 594 and ref.max() == 64
    else:
        assert ref.max() == 8 and np.diff(case.A.indptr).max() == PC.CLIQUE
    np.testing.assert_array_equal(_run(g, e, split_threshold=thr, groups=groups), ref)


@pytest.mark.parametrize("name", ["S", "H", "C"])
def test_symmetric_and_repeatable(name):
    _, g, e = _dev(name)
    for thr in (-1, 0):
        d1 = pair_distance(g, e, split_threshold=thr)
        assert torch.equal(d1, pair_distance(g, e, split_threshold=thr))
        assert torch.equal(d1, pair_distance(g, e.flip(0), split_threshold=thr))                 # d(a, b) == d(b, a)
        perm = torch.randperm(e.shape[1], generator=torch.Generator().manual_seed(3)).to(DEV)
        assert torch.equal(d1[perm], pair_distance(g, e[:, perm], split_threshold=thr, groups=5))   # batch position


@pytest.mark.parametrize("m", PC.MAX_DISTS)
@pytest.mark.parametrize("name", ["S", "H", "C"])
def test_max_dist_is_the_masked_exact_result(name, m):
    _, g, e = _dev(name)
    want = PC.masked(PC.exact(name), m)
    assert (want == -1).sum() > (PC.exact(name) == -1).sum()                                      # the cut-off bites
    for thr in (-1, 0):
        np.testing.assert_array_equal(_run(g, e, max_dist=m, split_threshold=thr), want)


def test_ignore_direct_against_per_edge_scipy():
    pairs, ref, plain = PC.ignore_direct_h()
    assert set(ref[:64].tolist()) == {-1, 2, 3, 4, 5, 6, 7} and (ref[:64] == -1).sum() == 11 and (plain[:64] == 1).all()
    _, g, _ = _dev("H")
    e = _t(pairs).to(DEV)
    for thr in (-1, 0, 1 << 30):
        got = _run(g, e, ignore_direct=True, split_threshold=thr)
        np.testing.assert_array_equal(got, ref)
        np.testing.assert_array_equal(got[64:], plain[64:])                                       # non-edges unchanged
        np.testing.assert_array_equal(_run(g, e.flip(0), ignore_direct=True, split_threshold=thr, groups=1), ref)
        np.testing.assert_array_equal(_run(g, e, ignore_direct=True, max_dist=3, split_threshold=thr),
                                      PC.masked(ref, 3))
    np.testing.assert_array_equal(_run(g, e), plain)
    # a == b stays 0 under ignore_direct
    same = torch.arange(0, 4000, 37, device=DEV).repeat(2, 1)
    assert not _run(g, same, ignore_direct=True).any()


def test_targeted_pairs_on_h():
    case, g, _ = _dev("H")
    iso = np.flatnonzero(np.diff(case.A.indptr) == 0)
    assert iso.size >= 2
    pairs = np.array([[0, 0, 1, 0, PC.PATH_LAST, PC.PATH_FIRST, PC.PATH_LAST, iso[0], iso[0], 5],
                      [1, 2, 2, PC.PATH_LAST, 0, PC.PATH_LAST, PC.PATH_FIRST, iso[1], 0, PC.PATH_LAST]])
    ref = PC.scipy_distance(case.A, pairs)
    # hub - hub; hub to the far end of the path (one-node frontiers against a 600-entry row); both ends of the path
    assert ref[3] == ref[4] >= 61 and ref[5] == ref[6] == 59 and ref[7] == -1 and ref[8] == -1 and ref[9] == 60
    assert (ref[:3] > 0).all()
    for thr in (-1, 0, 1 << 30):
        for groups in (1, None):
            np.testing.assert_array_equal(_run(g, _t(pairs), split_threshold=thr, groups=groups), ref)
    np.testing.assert_array_equal(_run(g, _t(pairs), max_dist=59), PC.masked(ref, 59))
    np.testing.assert_array_equal(_run(g, _t(pairs), max_dist=60), PC.masked(ref, 60))


@pytest.mark.parametrize("P", [1, 63, 64, 65, 257, 4096])
def test_batch_sizes(P):
    case, g, e = _dev("H")
    ref = PC.exact("H")
    # the tail of the batch: the last pairs, so that P = 1 is not the first pair of every other size
    np.testing.assert_array_equal(_run(g, e[:, -P:].contiguous()), ref[-P:])
    np.testing.assert_array_equal(_run(g, e[:, :P], split_threshold=0), ref[:P])      # a strided view of the batch


def test_layouts_chunks_host_edges_and_bad_ids():
    case, g, e = _dev("H")
    ref = PC.exact("H")
    np.testing.assert_array_equal(_run(g, e, chunk=1000), ref)
    np.testing.assert_array_equal(_run(g, e, chunk=1000, groups=3, split_threshold=0), ref)
    np.testing.assert_array_equal(_run(g, e.t().contiguous()), ref)                  # [P, 2] on the device
    np.testing.assert_array_equal(_run(g, _t(case.pairs)), ref)                      # [2, P] on the host
    np.testing.assert_array_equal(_run(g, _t(case.pairs.T).to(torch.int32)), ref)    # [P, 2] int32 on the host
    np.testing.assert_array_equal(_run(case.csr, e), ref)                            # a host CSR: uploaded once
    assert _run(g, torch.zeros(2, 0, dtype=torch.int64)).size == 0
    assert _run(g, torch.zeros(0, 2, dtype=torch.int64, device=DEV)).size == 0
    # ids outside [0, n) mixed into a batch
    mixed = case.pairs[:, :512].copy()
    mixed[0, ::7] = -1
    mixed[1, ::11] = case.n
    mixed[0, ::13] = case.n + 5
    mixed[:, 100] = -3                                                               # a == b reads 0 first
    want = ref[:512].copy()
    bad = (mixed < 0).any(axis=0) | (mixed >= case.n).any(axis=0)
    want[bad] = -1
    want[mixed[0] == mixed[1]] = 0
    assert bad.sum() > 100 and (~bad).sum() > 100
    for thr in (-1, 0):
        np.testing.assert_array_equal(_run(g, _t(mixed), split_threshold=thr), want)


def test_equals_the_numpy_restatement_on_s():
    case, g, e = _dev("S")
    for kw in ({}, {"max_dist": 3}, {"ignore_direct": True}, {"ignore_direct": True, "max_dist": 5}):
        want = distance_reference(case.csr, _t(case.pairs), **kw).numpy()
        np.testing.assert_array_equal(_run(g, e, **kw), want, err_msg=str(kw))
    r, c = case.A.nonzero()
    edges = _t(np.stack([r[::9], c[::9]]))
    want = distance_reference(case.csr, edges, ignore_direct=True).numpy()
    assert (want == -1).any() and (want >= 2).any() and not (want == 1).any()
    np.testing.assert_array_equal(_run(g, edges, ignore_direct=True), want)
    np.testing.assert_array_equal(_run(g, edges, ignore_direct=True, split_threshold=0, groups=1), want)


def test_model_source_uses_the_split_adjacency():
    fx = Fixture("lp_all_d64_residual_valtest")
    assert fx.test_set
    model = _build(fx)
    rng = np.random.default_rng(2)
    pairs = np.concatenate([fx["batch"].astype(np.int64), rng.integers(0, fx.n, size=(2, 2000))], axis=1)
    e = _t(pairs)
    d_tr = pair_distance(model, e, test_set=False)
    d_te = pair_distance(model, e, test_set=True)
    tr = graph.mask_csr(fx["edge_index"].astype(np.int64), fx.n, symmetric=True)
    te = graph.mask_csr(fx["full_edge_index"].astype(np.int64), fx.n, symmetric=True)
    assert torch.equal(d_tr, pair_distance(tr, e.to(DEV)))
    assert torch.equal(d_te, pair_distance(te, e.to(DEV)))
    assert not torch.equal(d_tr, d_te)                                               # the two splits differ
    for csr, d in ((tr, d_tr), (te, d_te)):
        A = PC._adjacency(*(np.repeat(np.arange(fx.n), np.diff(csr.rowptr)), csr.col.astype(np.int64)), fx.n)
        np.testing.assert_array_equal(d.cpu().numpy(), PC.scipy_distance(A, pairs))
    both = pair_distance(model, e, test_set=True, ignore_direct=True, max_dist=4)
    np.testing.assert_array_equal(both.cpu().numpy(),
                                  distance_reference(te, e, ignore_direct=True, max_dist=4).numpy())
