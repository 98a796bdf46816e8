"""threshold_profile on the MI355X (lpf_threshold_profile): exactly the numpy restatement in all five outputs, whatever
the split threshold and the chunking, and exactly what models built with the grid's thresholds select themselves."""
import numpy as np
import pytest
import torch

import lpformer_amd
from lpformer_amd import _lib, graph
from lpformer_amd import data as D
from lpformer_amd.threshold_profile import profile_reference, threshold_profile
from tests import threshold_profile_cases as TC
from tests.golden_util import Fixture
from tests.test_gpu_heuristics import _build

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FIELDS = ("thresholds", "total", "max_per_pair", "nonempty", "per_pair")


@pytest.fixture(scope="module", params=list(TC.CASES))
def case(request):
    return TC.CASES[request.param]()


@pytest.fixture(scope="module")
def want(case):
    return profile_reference(case.adj, case.ppr, case.pairs, case.grid, per_pair=True)


@pytest.fixture(scope="module")
def device_graphs(case):
    return case.adj.to_device(DEV), case.ppr.to_device(DEV)


def _same(got, ref, what=""):
    assert got.n_pairs == ref.n_pairs
    for f in FIELDS:
        g, r = getattr(got, f), getattr(ref, f)
        assert g.is_cuda and g.dtype == r.dtype and g.shape == r.shape, (what, f)
        assert torch.equal(g.cpu(), r), (what, f, g.cpu().tolist() if g.numel() < 40 else None, r.tolist()
                                         if r.numel() < 40 else None)


@pytest.mark.parametrize("split", [-1, 0, 16])
def test_equals_the_restatement_on_every_split_path(case, want, device_graphs, split):
    e = torch.from_numpy(case.pairs).to(DEV)
    got = threshold_profile(device_graphs, e, case.grid, per_pair=True, split_threshold=split)
    _same(got, want, f"{case.name} split {split}")
    again = threshold_profile(device_graphs, e, case.grid, per_pair=True, split_threshold=split)
    for f in FIELDS:
        assert torch.equal(getattr(got, f), getattr(again, f)), f           # two runs: bitwise equal
    slim = threshold_profile(device_graphs, e, case.grid, split_threshold=split)
    assert slim.per_pair is None and torch.equal(slim.total, got.total)
    assert torch.equal(slim.max_per_pair, got.max_per_pair) and torch.equal(slim.nonempty, got.nonempty)


def test_chunks_and_host_sources(case, want, device_graphs):
    e = torch.from_numpy(case.pairs)
    _same(threshold_profile(device_graphs, e, case.grid, per_pair=True, chunk=100), want, "chunk 100")
    _same(threshold_profile(device_graphs, e.t().contiguous(), case.grid, per_pair=True, chunk=64, split_threshold=16),
          want, "chunk 64, [P, 2]")
    _same(threshold_profile((case.adj, case.ppr), e, case.grid, per_pair=True), want, "host CSR source")   # uploaded


def test_mode_cn(case, device_graphs):
    ref = profile_reference(case.adj, case.ppr, case.pairs, case.grid, mode_cn=True, per_pair=True)
    for split in (-1, 0):
        got = threshold_profile(device_graphs, torch.from_numpy(case.pairs), case.grid, per_pair=True, mode_cn=True,
                                split_threshold=split)
        _same(got, ref, f"mode cn, split {split}")
    assert not got.total[1:].any()


def test_default_grid_and_all_32_thresholds(case, device_graphs):
    e = torch.from_numpy(case.pairs)
    _same(threshold_profile(device_graphs, e, per_pair=True), profile_reference(case.adj, case.ppr, e, per_pair=True))
    grid = np.concatenate([[0.0], np.geomspace(1e-6, 0.5, 31)])
    for split in (-1, 0):
        _same(threshold_profile(device_graphs, e, grid, per_pair=True, split_threshold=split),
              profile_reference(case.adj, case.ppr, e, grid, per_pair=True), f"T = 32, split {split}")


def test_empty_single_and_out_of_range(case, want, device_graphs):
    T = case.grid.size
    p0 = threshold_profile(device_graphs, torch.zeros(2, 0, dtype=torch.int64), case.grid, per_pair=True)
    assert p0.n_pairs == 0 and p0.per_pair.shape == (0, 3, T) and p0.total.is_cuda and not p0.total.any()
    assert not p0.max_per_pair.any() and not p0.nonempty.any()
    hub = int(np.argmax(np.diff(case.adj.rowptr)))
    for split in (-1, 0):
        one = np.array([[hub], [hub]])
        _same(threshold_profile(device_graphs, torch.from_numpy(one), case.grid, per_pair=True, split_threshold=split),
              profile_reference(case.adj, case.ppr, one, case.grid, per_pair=True), "P = 1")
        bad = np.array([[-1, case.n, 0, 3], [2, 1, case.n + 5, -7]])
        pairs = np.concatenate([case.pairs[:, :5], bad, case.pairs[:, 5:]], axis=1)
        got = threshold_profile(device_graphs, torch.from_numpy(pairs), case.grid, per_pair=True, split_threshold=split)
        assert not got.per_pair[5:9].any()
        keep = torch.tensor([i for i in range(pairs.shape[1]) if not 5 <= i < 9], device=DEV)
        assert torch.equal(got.per_pair[keep].cpu(), want.per_pair)
        for f in ("total", "max_per_pair", "nonempty"):
            assert torch.equal(getattr(got, f).cpu(), getattr(want, f)), f


def _model(fx, triple):
    ei = fx["edge_index"].astype(np.int64)
    r, c, v = fx.ppr_coo
    data = D.build_data(ei, fx["x"], fx.n, edge_weight=fx["edge_weight"], ppr=graph.csr_from_coo(r, c, v, fx.n))
    cfg = {k: fx.cfg[k] for k in ("dim", "trans_layers", "num_heads", "att_drop", "dropout", "gnn_drop", "feat_drop",
                                  "gcn_cache", "gnn_layers", "residual", "layer_norm", "relu")}
    cfg.update(thresh_cn=triple[0], thresh_1hop=triple[1], thresh_non1hop=triple[2])
    model = lpformer_amd.LinkTransformer(cfg, data, device=DEV).to(DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in fx.state_dicts()[0].items()}, strict=True)
    assert model.mask == "all"
    return model.eval()


def test_equals_what_models_with_these_thresholds_select():
    """The check that proves the kernel: for three threshold triples of the grid a LinkTransformer built with them
    selects, pair by pair and type by type, exactly the profile's counts."""
    case = TC.fixture_case()
    fx = Fixture("lp_all_d64")
    g = [float(t) for t in case.grid]
    hop_b, cn_b = (float(np.float32(t)) for t in case.special)
    triples = [(0.0, hop_b, g[3]), (g[2], g[2], g[2]), (cn_b, g[3], hop_b)]
    batch = torch.from_numpy(case.pairs)
    prof = None
    for triple in triples:
        model = _model(fx, triple)
        if prof is None:
            prof = threshold_profile(model, batch, case.grid, per_pair=True)      # (the model's own thresholds play no part)
            _same(prof, profile_reference(case.adj, case.ppr, case.pairs, case.grid, per_pair=True), "model source")
        sel = model.compute_node_mask(batch.to(DEV))
        lens = []
        for t in range(3):
            j = g.index(triple[t])
            cnt = torch.bincount(sel[t][0][0], minlength=case.pairs.shape[1])
            assert torch.equal(cnt.to(torch.int32), prof.per_pair[:, t, j]), (triple, t)
            lens.append(int(sel[t][0].shape[1]))
        assert prof.entries(*triple) == tuple(lens)
        assert sum(lens) > 0


def test_test_set_uses_the_full_adjacency_and_ppr_test():
    fx = Fixture("lp_all_d64_residual_valtest")
    model, _ = _build(fx)
    rng = np.random.default_rng(2)
    pairs = np.concatenate([fx["batch"].astype(np.int64)[:, :129], rng.integers(0, fx.n, size=(2, 128))], axis=1)
    grid = sorted({0.0, 1e-3, 1e-2, float(fx.cfg["thresh_cn"]), float(fx.cfg["thresh_1hop"]),
                   float(fx.cfg["thresh_non1hop"])})
    refs = {}
    for test_set, ek, pk in ((False, "edge_index", "ppr_"), (True, "full_edge_index", "ppr_test_")):
        adj = graph.mask_csr(fx[ek].astype(np.int64), fx.n, symmetric=True)
        ppr = graph.csr_from_coo(fx[pk + "row"], fx[pk + "col"], fx[pk + "val"], fx.n)
        refs[test_set] = profile_reference(adj, ppr, pairs, grid, per_pair=True)
        _same(threshold_profile(model, torch.from_numpy(pairs), grid, per_pair=True, test_set=test_set), refs[test_set],
              f"test_set {test_set}")
    assert not torch.equal(refs[False].per_pair, refs[True].per_pair)
    # ... and what the model itself selects on that split with its own thresholds
    th = [float(np.float32(fx.cfg[k])) for k in ("thresh_cn", "thresh_1hop", "thresh_non1hop")]
    sel = model.compute_node_mask(torch.from_numpy(pairs).to(DEV), test_set=True)
    gl = [float(np.float32(t)) for t in grid]
    for t in range(3):
        cnt = torch.bincount(sel[t][0][0], minlength=pairs.shape[1]).to(torch.int32).cpu()
        assert torch.equal(cnt, refs[True].per_pair[:, t, gl.index(th[t])]), t


def test_entry_point_rejects_bad_thresholds(device_graphs):
    import ctypes as C
    adj, ppr = device_graphs
    z = torch.zeros(2, 4, dtype=torch.int64, device=DEV)
    out = torch.zeros(3, 33, dtype=torch.int64, device=DEV)
    mx = torch.zeros(3, 33, dtype=torch.int32, device=DEV)
    scratch = torch.zeros(8, dtype=torch.int32, device=DEV)

    def call(values, T=None):
        arr = (C.c_float * max(len(values), 1))(*values)
        return _lib.hip().lpf_threshold_profile(
            4, adj.n, z.data_ptr(), 4, adj.rowptr.data_ptr(), adj.col.data_ptr(), ppr.rowptr.data_ptr(),
            ppr.col.data_ptr(), ppr.val.data_ptr(), len(values) if T is None else T, C.cast(arr, C.c_void_p), 0, -1,
            scratch.data_ptr(), None, out.data_ptr(), mx.data_ptr(), out.data_ptr(), None)

    assert call([0.0, 1e-3]) == 0
    for values in ([], [float(i) for i in range(33)], [-1e-3, 0.0], [0.0, float("nan")], [0.0, float("inf")],
                   [1e-3, 1e-3], [1e-2, 1e-3]):
        assert call(values) == -1, values                          # LPF_ERR_INVALID
    torch.cuda.synchronize()


def test_abi_version():
    assert _lib.hip().lpf_abi_version() == 16 == _lib.ABI_VERSION
