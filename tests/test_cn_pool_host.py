"""The host side of common-neighbour pooling (lpformer_amd/ncn.py): the restatements against the dense fp64 form
((A[a] o A[b]) diag(w)) @ T, the chunk order, symmetry, autograd through the CPU path, NCNPredictor on the CPU and the
argument errors.  No GPU."""
import numpy as np
import pytest
import torch

from lpformer_amd import ncn
from tests import cn_pool_cases as CC


@pytest.mark.parametrize("name", CC.NAMES)
def test_case_facts(name):
    c, k = CC.case(name), CC.counts(name)
    a, b = c.pairs
    facts = {"S": (4096 + 4, 6, 3, 3), "H": (4096 + 6 + 4, 126 + 6, 53, 2), "C": (837 + 4, 259, 298, None)}
    if name in facts:
        P, positive, largest, same = facts[name]
        assert (c.pairs.shape[1], int((k > 0).sum()), int(k.max())) == (P, positive, largest)
        assert same is None or int((a == b).sum()) == same
    if name == "C":
        assert int((k == 298).sum()) == 257
    if name == "H":
        assert k[4096:4102].tolist() == [53, 32, 19, 53, 32, 19]
        deg = np.diff(c.csr.rowptr)
        assert [int(min(deg[x], deg[y])) for x, y in CC.HUB_PAIRS] == [302, 260, 260]
    if name == "fan":
        m = len(CC.fan_facts())
        want = [f[2] for f in CC.fan_facts()]
        assert k[:m].tolist() == want and k[m:2 * m].tolist() == want and want[:-1] == list(CC.FAN_KS)
    assert c.n_bad == 4 and not k[-4:].any()


@pytest.mark.parametrize("name", CC.NAMES)
def test_entries_reference_equals_the_dense_rows(name):
    ent, M = CC.entries(name), CC.dense_rows(name)
    assert ent.seg.dtype == torch.int64 and ent.node.dtype == torch.int32
    assert np.array_equal(ent.seg.numpy(), M.indptr.astype(np.int64))
    assert np.array_equal(ent.node.numpy(), M.indices.astype(np.int32))


@pytest.mark.parametrize("name", CC.NAMES)
@pytest.mark.parametrize("kind", CC.WEIGHT_KINDS)
def test_pool_reference_equals_the_dense_form(name, kind):
    dim = 36
    ref, mag = CC.reference(name, dim, kind)
    dense = CC.dense_pool(name, CC.table(name, dim), CC.weights(name, kind))
    assert ref.dtype == torch.float64 and ref.shape == dense.shape
    # two fp64 orders of at most 600 terms
    assert ((ref - dense).abs() <= 600 * 2.0 ** -52 * mag + 1e-300).all()
    assert not ref[CC.counts(name) == 0].any()


@pytest.mark.parametrize("name", CC.NAMES)
def test_pool_reference_is_exact_on_integers(name):
    ref = CC.int_reference(name)
    assert torch.equal(ref, CC.dense_pool(name, CC.int_table(name), CC.int_weights(name)))


def test_chunk_size_moves_only_last_bits():
    c, t, w = CC.case("C"), CC.table("C", 36), CC.weights("C", "aa")
    ref, mag = CC.reference("C", 36, "aa")
    for chunk in (1, 7, 128, 1 << 20):
        other = ncn.cn_pool_reference(c.csr, c.pairs, t, w, chunk=chunk)
        assert ((other - ref).abs() <= 600 * 2.0 ** -52 * mag).all(), chunk
    assert not torch.equal(ncn.cn_pool_reference(c.csr, c.pairs, t, w, chunk=1 << 20), ref)   # the order is real


@pytest.mark.parametrize("name", ("H", "fan"))
def test_swapped_pairs_give_the_same_bits(name):
    c = CC.case(name)
    t = CC.table(name, 36)
    swapped = c.pairs.flip(0)
    for w in (None, CC.weights(name, "tensor")):
        assert torch.equal(ncn.cn_pool_reference(c.csr, c.pairs, t, w), ncn.cn_pool_reference(c.csr, swapped, t, w))
        assert torch.equal(ncn.cn_pool(c.csr, c.pairs, t, weights="none" if w is None else w),
                           ncn.cn_pool(c.csr, swapped, t, weights="none" if w is None else w))
    a, b = ncn.cn_entries_reference(c.csr, c.pairs), ncn.cn_entries_reference(c.csr, swapped)
    assert torch.equal(a.seg, b.seg) and torch.equal(a.node, b.node)


def test_cpu_path_follows_the_contract_and_passes_gradcheck():
    c = CC.case("fan")
    t32 = CC.table("fan", 4)
    pool, cn = ncn.cn_pool(c.csr, c.pairs.t(), t32, weights="ra", return_count=True)       # [P, 2] in
    assert pool.dtype == torch.float32 and pool.shape == (c.pairs.shape[1], 4)
    assert torch.equal(cn.to(torch.int64), CC.counts("fan")) and cn.dtype == torch.int32
    ref = ncn.cn_pool_reference(c.csr, c.pairs, t32, CC.weights("fan", "ra"))
    mag = ncn.cn_pool_reference(c.csr, c.pairs, t32.abs(), CC.weights("fan", "ra"))
    assert ((pool.double() - ref).abs() <= CC.forward_bound("fan", mag)).all()
    ent = ncn.cn_entries(c.csr, c.pairs)
    assert torch.equal(ent.node, CC.entries("fan").node) and torch.equal(ent.seg, CC.entries("fan").seg)
    m = 2 * len(CC.fan_facts())
    pairs = c.pairs[:, :m]
    gen = torch.Generator().manual_seed(1)
    t = torch.randn((c.n, 4), dtype=torch.float64, generator=gen, requires_grad=True)
    w = CC.weights("fan", "tensor")
    # the whole table along random directions, then element by element on 48 rows: 40 common neighbours of the named
    # pairs (of up to 192 a pair, so every chunk of the sum is touched) and 8 other nodes
    assert torch.autograd.gradcheck(lambda x: ncn.cn_pool(c.csr, pairs, x, weights=w), (t,), eps=1e-6, atol=1e-6,
                                    fast_mode=True)
    assert torch.autograd.gradcheck(lambda x: ncn.cn_pool(c.csr, pairs, x), (t,), eps=1e-6, atol=1e-6, fast_mode=True)
    held = ncn.cn_entries_reference(c.csr, pairs).node.to(torch.int64).unique()
    rows = torch.cat([held[torch.randperm(held.numel(), generator=gen)[:40]], torch.arange(8)]).unique()
    base = t.detach()
    sub = base[rows].clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x: ncn.cn_pool(c.csr, pairs, base.index_copy(0, rows, x), weights=w), (sub,),
                                    eps=1e-6, atol=1e-6)


def test_predictor_on_the_cpu_separates_the_cliques():
    c = CC.case("C")
    pairs, labels = CC.clique_pairs()
    torch.manual_seed(0)
    h = torch.nn.Parameter(0.1 * torch.randn(c.n, 16))
    model = ncn.NCNPredictor(16, hidden=32, layers=2, beta=1.0)
    logits = model(c.csr, h, pairs)
    assert logits.shape == (pairs.shape[1],) and logits.dtype == torch.float32
    assert model(c.csr, h, pairs.t()).shape == logits.shape                                # [P, 2] in
    loss0 = torch.nn.functional.binary_cross_entropy_with_logits(logits, labels)
    loss0.backward()
    for name, p in list(model.named_parameters()) + [("h", h)]:
        assert p.grad is not None and bool(p.grad.abs().sum() > 0), name
    assert model.beta.grad.dim() == 0
    opt = torch.optim.Adam(list(model.parameters()) + [h], lr=0.01)
    loss = loss0
    for _ in range(30):
        opt.zero_grad()
        loss = torch.nn.functional.binary_cross_entropy_with_logits(model(c.csr, h, pairs), labels)
        loss.backward()
        opt.step()
    final = ncn.ncn_scores(c.csr, model, h.detach(), pairs, chunk=50)
    assert torch.allclose(final, model(c.csr, h, pairs).detach(), atol=1e-6)
    assert float(loss.detach()) < float(loss0.detach())
    assert float(final[labels == 1].mean()) > float(final[labels == 0].mean())


def test_argument_errors():
    c = CC.case("fan")
    t = CC.table("fan", 4)
    with pytest.raises(ValueError):
        ncn.cn_pool(c.csr, c.pairs.to(torch.float32), t)                                   # a float edge dtype
    with pytest.raises(ValueError):
        ncn.cn_entries(c.csr, c.pairs.to(torch.float64))
    with pytest.raises(ValueError):
        ncn.cn_pool(c.csr, c.pairs, torch.zeros(c.n, 6))                                   # D = 6
    with pytest.raises(ValueError):
        ncn.cn_pool(c.csr, c.pairs, torch.zeros(c.n, 516))                                 # D = 516
    with pytest.raises(ValueError):
        ncn.cn_pool(c.csr, c.pairs, t, weights=torch.ones(c.n + 1))                        # weights of the wrong length
    with pytest.raises(ValueError):
        ncn.cn_pool(c.csr, c.pairs, t, weights="jaccard")
    with pytest.raises(ValueError):
        ncn.cn_pool(c.csr, c.pairs, t[:-1])                                                # not a row per node
    with pytest.raises(ValueError):
        ncn.cn_pool(c.csr, c.pairs, torch.empty((c.n, 4), device="meta"))                  # a table on another device
    with pytest.raises(ValueError):
        ncn.cn_pool(c.csr, c.pairs, t, chunk=0)
    with pytest.raises(ValueError):
        ncn.NCNPredictor(16, weights="jaccard")
