"""random_walks (lpf_random_walks in csrc/random_walk.hip) on the MI355X against the numpy restatement: every
comparison of walks and forced counts is exact integer equality.  node2vec_embeddings: qualitative inequalities."""
import numpy as np
import pytest
import torch

from lpformer_amd import _lib, graph
from lpformer_amd.random_walks import (FORMS, Walks, node2vec_embeddings, random_walks, walk_pairs, walk_thresholds,
                                       walks_reference)
from tests import pair_distance_cases as DC
from tests import random_walks_cases as RC
from tests.golden_util import Fixture
from tests.test_gpu_pair_distance import _build

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(name):
    case = RC.case(name)
    return case, case.csr.to_device(DEV), torch.from_numpy(RC.starts(name).copy()).to(DEV)


def _run(g, starts, p, q, **kw):
    kw.setdefault("length", RC.LENGTH)
    kw.setdefault("seed", RC.SEED)
    out = random_walks(g, starts, p=p, q=q, **kw)
    assert isinstance(out, Walks) and out.walks.is_cuda and out.forced.is_cuda
    assert out.walks.dtype == torch.int32 and out.forced.dtype == torch.int32
    assert out.walks.shape == (out.forced.shape[0], kw["length"] + 1)
    return out


@pytest.mark.parametrize("name", RC.NAMES)
@pytest.mark.parametrize("pq", RC.PQ)
def test_matches_the_restatement(name, pq):
    """Every node twice, starts outside the graph and repeated starts, at max_tries 64 and 2, both forms."""
    _, g, starts = _dev(name)
    for T in (64, 2):
        walks, forced = RC.reference(name, *pq, T)
        for form in ("lane", "group8"):
            out = _run(g, starts, *pq, walks_per_node=2, max_tries=T, form=form)
            np.testing.assert_array_equal(out.walks.cpu().numpy(), walks, err_msg=f"{form} T={T}")
            np.testing.assert_array_equal(out.forced.cpu().numpy(), forced, err_msg=f"{form} T={T}")
        print(name, pq, "max_tries", T, "forced steps", int(forced.sum()))
        if T == 2 and pq != (1.0, 1.0):
            assert forced.sum() > 0
        if pq == (1.0, 1.0):
            assert not forced.any()


@pytest.mark.parametrize("name", ("H", "C"))
def test_both_forms_and_two_runs_give_the_same_bits(name):
    _, g, starts = _dev(name)
    a = _run(g, starts, 0.25, 4.0, form="default")
    for form in FORMS:
        b = _run(g, starts, 0.25, 4.0, form=form)
        assert torch.equal(a.walks, b.walks) and torch.equal(a.forced, b.forced), form
    host = _run(RC.case(name).csr, starts.cpu(), 0.25, 4.0)                # a host CSR is uploaded
    assert torch.equal(a.walks, host.walks) and torch.equal(a.forced, host.forced)


def test_one_call_equals_chunked_calls_with_walk_base():
    _, g, starts = _dev("H")
    whole = _run(g, starts, 4.0, 0.25, walks_per_node=2)
    both = starts.repeat(2)
    cuts = (0, 63, 64, 1000, 4097, both.numel())
    parts = [_run(g, both[lo:hi], 4.0, 0.25, walk_base=lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
    assert torch.equal(whole.walks, torch.cat([p.walks for p in parts]))
    assert torch.equal(whole.forced, torch.cat([p.forced for p in parts]))
    # the kernel's buffer is step-major: the returned view has the walk as its fast-changing index
    assert whole.walks.stride() == (1, whole.walks.shape[0])
    every = _run(g, None, 1.0, 1.0, length=3)
    assert every.walks.shape == (g.n, 4) and torch.equal(every.walks[:, 0].long(), torch.arange(g.n, device=DEV))
    assert _run(g, torch.zeros(0, dtype=torch.int64), 1.0, 1.0).walks.shape == (0, RC.LENGTH + 1)


def test_second_step_frequencies_are_node2vec():
    g = RC.bias_graph().to_device(DEV)
    starts = torch.zeros(RC.BIAS_WALKS, dtype=torch.int64, device=DEV)
    for pq, want in RC.BIAS_WANT.items():
        out = _run(g, starts, *pq, length=2, seed=0)
        z = RC.bias_z(out.walks.cpu().numpy(), want)
        print(pq, "|z| per target", z.round(2))
        assert (z < 4.0).all()


def test_model_source_equals_its_adjacency():
    fx = Fixture("lp_all_d64_residual_valtest")
    model = _build(fx)
    seen = []
    for test_set, key in ((False, "edge_index"), (True, "full_edge_index")):
        csr = graph.mask_csr(fx[key].astype(np.int64), fx.n, symmetric=True)
        out = _run(model, None, 0.25, 4.0, walks_per_node=2, test_set=test_set)
        ref = walks_reference(csr, None, length=RC.LENGTH, walks_per_node=2, p=0.25, q=4.0, seed=RC.SEED)
        np.testing.assert_array_equal(out.walks.cpu().numpy(), ref.walks.numpy())
        np.testing.assert_array_equal(out.forced.cpu().numpy(), ref.forced.numpy())
        seen.append(out.walks)
    assert not torch.equal(seen[0], seen[1])                               # the two splits' adjacencies differ


def test_c_entry_rejects_bad_arguments_without_a_launch():
    _, g, starts = _dev("S")
    hip = _lib.hip()
    n, nnz, W, L = g.n, g.nnz, 512, 4
    starts = starts[:W].contiguous()
    walks = torch.full((L + 1, W), -7, dtype=torch.int32, device=DEV)
    forced = torch.full((W,), -7, dtype=torch.int32, device=DEV)
    rp, col, sp, wp, fp = g.rowptr.data_ptr(), g.col.data_ptr(), starts.data_ptr(), walks.data_ptr(), forced.data_ptr()
    thr = walk_thresholds(0.25, 4.0)

    def call(n=n, nnz=nnz, rp=rp, col=col, W=W, sp=sp, base=0, L=L, thr=thr, second=1, T=64, form=0, wp=wp, ldw=W,
             fp=fp):
        return hip.lpf_random_walks(n, nnz, rp, col, W, sp, base, L, 3, thr[0], thr[1], thr[2], second, T, form, wp,
                                    ldw, fp, 0)
    for bad in (dict(n=-1), dict(nnz=-1), dict(W=-1), dict(n=1 << 31), dict(rp=None), dict(col=None), dict(sp=None),
                dict(wp=None), dict(L=0), dict(L=_lib.CONST["LPF_WALK_MAX_LENGTH"] + 1), dict(T=0),
                dict(T=_lib.CONST["LPF_WALK_MAX_TRIES"] + 1), dict(form=2), dict(form=-1), dict(second=2),
                dict(ldw=W - 1), dict(thr=((1 << 63) + 1, 1, 1))):
        assert call(**bad) == -1, bad
    assert call(W=0) == 0 and call(W=0, sp=None, wp=None) == 0 and call(n=0, nnz=0) == 0   # LPF_OK, no launch
    torch.cuda.synchronize()
    assert (walks == -7).all() and (forced == -7).all()                    # nothing ran
    assert call(fp=None) == 0                                              # forced is optional
    torch.cuda.synchronize()
    ref = walks_reference(RC.case("S").csr, starts.cpu(), length=L, p=0.25, q=4.0, seed=3)
    np.testing.assert_array_equal(walks.t().cpu().numpy(), ref.walks.numpy())
    assert (forced == -7).all()
    empty = random_walks(graph.CSR(np.zeros(1, np.int64), np.zeros(0, np.int32), None, 0).to_device(DEV),
                         torch.tensor([0, 5]), length=3, seed=1)
    assert empty.walks.tolist() == [[-1] * 4] * 2 and empty.forced.tolist() == [0, 0]


def test_node2vec_embeddings_separate_two_cliques():
    case, g, _ = _dev("C")
    emb, losses = node2vec_embeddings(g, 16, walk_length=10, context=5, walks_per_node=4, epochs=2, batch_walks=64,
                                      lr=0.05)
    assert emb.is_cuda and emb.shape == (case.n, 16) and emb.dtype == torch.float32 and torch.isfinite(emb).all()
    assert len(losses) == 2 and all(np.isfinite(losses))
    k = DC.CLIQUE
    e = torch.nn.functional.normalize(emb[:2 * k].double(), dim=1)
    cos = e @ e.t()
    within = (cos[:k, :k].sum() + cos[k:, k:].sum() - 2 * k) / (2 * k * (k - 1))
    across = cos[:k, k:].mean()
    print("losses", losses, "mean cosine within", float(within), "across", float(across))
    assert losses[-1] < losses[0]
    assert float(within) > float(across)
    pairs = walk_pairs(random_walks(g, None, length=10, seed=0).walks, 5)
    assert pairs.is_cuda and pairs.dtype == torch.int64 and pairs.shape == (2, case.n * 7 * 4)
