"""CPU checks of similar_nodes: the numpy restatement against a plain Python loop on the exact integer cases, the
argument checks that must raise before any device use, and the exports and bindings."""
import numpy as np
import pytest
import torch

import lpformer_amd
from lpformer_amd import _lib, graph, similar
from lpformer_amd.recommend import CANDIDATE_MODES, MAX_SIMILAR, _check_args
from tests import similar_cases as SC

SPECS = SC.exact_specs()


def test_specs_cover_every_listed_value():
    assert 45 <= len(SPECS) <= 70
    for key, values in (("n", SC.N_VALUES), ("S", SC.S_VALUES), ("D", SC.D_VALUES), ("m", SC.M_VALUES),
                        ("exclusion", SC.EXCLUSIONS), ("metric", ("dot", "cosine")), ("exclude_self", (True, False)),
                        ("kind", ("increasing", "decreasing", "special"))):
        assert set(values) <= {s.get(key) for s in SPECS}, key
    assert any(s["m"] > s["n"] for s in SPECS)


@pytest.mark.parametrize("spec", SPECS, ids=lambda s: SC.make_case(**s)["id"])
def test_reference_against_python_loop(spec):
    case = SC.make_case(**spec)
    got = similar.similar_reference(case["Q"], case["T"], case["m"], q_scale=case["q_scale"], t_scale=case["t_scale"],
                                    src_ids=case["src_ids"], exclude=case["exclude"],
                                    exclude_self=case["exclude_self"])
    want = SC.loop_reference(case)
    np.testing.assert_array_equal(got[2], want[2])
    np.testing.assert_array_equal(got[0], want[0])
    assert SC.same_bits(got[1], want[1])
    assert got[0].dtype == np.int64 and got[1].dtype == np.float32 and got[2].dtype == np.int64


def test_reference_hand_case():
    T = np.array([[1.0], [3.0], [3.0], [-0.0], [0.0], [np.nan], [-np.inf]], np.float32)
    Q = np.array([[1.0]], np.float32)
    ids, sc, cnt = similar.similar_reference(Q, T, 8)
    # ties to the smaller id; -0.0 ties +0.0; NaN below -inf; padding never among the results
    np.testing.assert_array_equal(ids[0], [1, 2, 0, 3, 4, 6, 5, -1])
    assert cnt[0] == 7 and np.isnan(sc[0, 6]) and np.isneginf(sc[0, 5]) and np.isneginf(sc[0, 7])
    assert SC.same_bits(sc[0, 3:5], [0.0, 0.0])
    ids, _, cnt = similar.similar_reference(Q, T, 3, src_ids=[1], exclude=(np.array([0, 0, 1, 1, 1, 1, 1, 1]),
                                                                        np.array([2])))
    np.testing.assert_array_equal(ids[0], [0, 3, 4])          # 1 is the source, 2 its excluded neighbour
    ids, _, cnt = similar.similar_reference(Q, T, 3, src_ids=[1], exclude_self=False)
    np.testing.assert_array_equal(ids[0], [1, 2, 0])
    assert similar.similar_reference(Q, T, 3, src_ids=[7])[2][0] == 0


def test_cpu_tensors_without_a_model_use_the_reference():
    rng = np.random.default_rng(4)
    T = torch.from_numpy(rng.standard_normal((40, 6)).astype(np.float32))
    T[7] = 0                                                   # a zero row: cosine 0, not NaN
    nodes = torch.tensor([3, 7, 3, 41])
    exc = graph.CSR(*SC.random_csr(40, rng), None, 40)
    got = lpformer_amd.similar_nodes(None, nodes, 5, table=T, exclude=exc)
    assert isinstance(got, lpformer_amd.Similar) and got.ids.shape == (4, 5)
    with np.errstate(divide="ignore"):
        inv = 1.0 / np.linalg.norm(T.numpy(), axis=1)
    inv[7] = 0
    want = similar.similar_reference(T.numpy()[[3, 7, 3, 39]], T.numpy(), 5, q_scale=inv[[3, 7, 3, 39]].astype(np.float32),
                                     t_scale=inv.astype(np.float32), src_ids=nodes.numpy(),
                                     exclude=(exc.rowptr, exc.col))
    np.testing.assert_array_equal(got.ids.numpy(), want[0])
    np.testing.assert_allclose(got.scores.numpy(), want[1], rtol=1e-6)
    assert got.counts.tolist() == [5, 5, 5, 0] and bool((got.scores[1] == 0).all())
    free = lpformer_amd.similar_nodes(None, queries=T[:2] * 2, m=3, table=T, metric="dot", exclude=None)
    np.testing.assert_array_equal(free.ids.numpy(), similar.similar_reference(2 * T.numpy()[:2], T.numpy(), 3)[0])


def test_argument_checks_raise_before_any_device_use():
    T = torch.zeros(10, 4)
    nodes = torch.tensor([0, 1, 2])
    for bad_m in (0, -1, similar.MAX_M + 1, 2.5, True):
        with pytest.raises(ValueError):
            lpformer_amd.similar_nodes(None, nodes, bad_m, table=T, exclude=None)
    with pytest.raises(ValueError):                            # neither nodes nor queries
        lpformer_amd.similar_nodes(None, table=T, exclude=None)
    with pytest.raises(ValueError):                            # both, with different S
        lpformer_amd.similar_nodes(None, nodes, queries=torch.zeros(2, 4), table=T, exclude=None)
    with pytest.raises(TypeError):                             # float ids
        lpformer_amd.similar_nodes(None, torch.tensor([0.0, 1.0]), table=T, exclude=None)
    with pytest.raises(TypeError):
        lpformer_amd.similar_nodes(None, queries=torch.zeros(2, 4, dtype=torch.int64), table=T, exclude=None)
    with pytest.raises(ValueError):
        lpformer_amd.similar_nodes(None, nodes, table=T, metric="euclid", exclude=None)
    with pytest.raises(ValueError):
        lpformer_amd.similar_nodes(None, nodes, table="ppr", exclude=None)
    with pytest.raises(TypeError):
        lpformer_amd.similar_nodes(None, nodes, table=torch.zeros(10, 4, dtype=torch.int64), exclude=None)
    with pytest.raises(ValueError):                            # a named table or 'adj' needs a model
        lpformer_amd.similar_nodes(None, nodes, table="embedding", exclude=None)
    with pytest.raises(ValueError):
        lpformer_amd.similar_nodes(None, nodes, table=T, exclude="adj")
    with pytest.raises(ValueError):
        lpformer_amd.similar_nodes(None, nodes, table=T, exclude="ppr")
    with pytest.raises(ValueError):
        lpformer_amd.similar_nodes(None, queries=torch.zeros(2, 5), table=T, exclude=None)
    # (a model argument of None proves that nothing touched a model or a device before the check)
    with pytest.raises(ValueError):
        lpformer_amd.similar_nodes(None, nodes, 0, table="embedding")


def test_recommend_modes_and_keywords_raise_before_any_device_use():
    src = torch.tensor([0, 1, 2])
    assert CANDIDATE_MODES == ("ppr", "all", "2hop", "similar", "ppr+similar")
    assert MAX_SIMILAR == similar.MAX_M == 256
    for mode in ("similar", "ppr+similar"):
        _check_args(src, 10, mode)
        for bad in (0, similar.MAX_M + 1, 1.5, True):
            with pytest.raises(ValueError):
                lpformer_amd.recommend(None, None, src, candidates=mode, n_similar=bad)
        with pytest.raises(ValueError):
            lpformer_amd.recommend(None, None, src, candidates=mode, similar_metric="l2")
        with pytest.raises(ValueError):
            lpformer_amd.recommend(None, None, src, candidates=mode, similar_table="h")
        with pytest.raises(ValueError):
            lpformer_amd.recommend(None, None, src, candidates=mode, similar_table=torch.zeros(3, 4))
    with pytest.raises(ValueError):
        lpformer_amd.recommend(None, None, src, candidates="similar+ppr")


def test_exports_constant_and_bindings():
    for name in ("similar_nodes", "similar_reference", "Similar"):
        assert name in lpformer_amd.__all__ and hasattr(lpformer_amd, name)
    assert "similar_nodes" in lpformer_amd.__doc__
    assert _lib.CONST["LPF_SIMILAR_MAX_M"] == 256 and _lib.CONST["LPF_ABI_VERSION"] == 16
    lib = _lib.hip()
    for name in ("lpf_similar_workspace_bytes", "lpf_similar_topm_f32"):
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (_lib.PROTOTYPES[name][0], _lib.PROTOTYPES[name][1])
    assert lib.lpf_similar_workspace_bytes.restype is __import__("ctypes").c_int64
    assert len(_lib.PROTOTYPES["lpf_similar_topm_f32"][1]) == 20
    # sizes: S * ranges * m keys of 8 bytes; bad arguments are a negative error code
    assert lib.lpf_similar_workspace_bytes(5, 7, 3) == 5 * 3 * 7 * 8
    assert lib.lpf_similar_workspace_bytes(0, 7, -1) == 0
    assert lib.lpf_similar_workspace_bytes(33, 256, -1) >= 33 * 256 * 8
    for bad in ((5, 0, 1), (5, 257, 1), (5, 7, 0), (-1, 7, 1)):
        assert lib.lpf_similar_workspace_bytes(*bad) < 0
