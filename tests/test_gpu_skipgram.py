"""The skip-gram kernels (csrc/skipgram.hip) on the MI355X, each entry on its own against ``skipgram_reference`` with
the bounds of tests/skipgram_cases.py (built from the reference's own magnitudes), exact integer sums for the gradient
kernel, repeatable bits, ``node2vec_embeddings(trainer="device")`` and the C entries' argument checks.  Every test
prints its worst ratio error / bound-with-C-equal-1: the constants in skipgram_cases.py are set from those."""
import numpy as np
import pytest
import torch

from lpformer_amd import _lib, skipgram
from lpformer_amd.random_walks import node2vec_embeddings, random_walks
from tests import pair_distance_cases as DC
from tests import random_walks_cases as RC
from tests import skipgram_cases as SC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U23 = SC.U23


def _buffer(view):
    """A step-major view on the device with the host view's row stride (the padding holds an id far outside)."""
    base = torch.full((view.shape[0], view.stride(0)), 1 << 30, dtype=torch.int32, device=DEV)
    base[:, :view.shape[1]] = view.to(DEV)
    return base[:, :view.shape[1]]


def _dev(name):
    c = SC.case(name)
    return c, c.table.to(DEV), _buffer(c.pos), _buffer(c.neg)


def _coef(c, table, pos, neg):
    """lpf_skipgram_coef_f32 alone: (coef float32 [M], ids int32 [2 M], loss 0-d float64)."""
    L, ctx = c.spec.length, c.spec.context
    nwin = L + 2 - ctx
    M = (pos.shape[1] + neg.shape[1]) * nwin * (ctx - 1)
    coef = torch.full((M,), 7.0, dtype=torch.float32, device=DEV)
    ids = torch.full((2 * M,), -7, dtype=torch.int32, device=DEV)
    partial = torch.empty(-(-(pos.shape[1] + neg.shape[1]) * nwin // skipgram.BLOCK_WINDOWS), dtype=torch.float64,
                          device=DEV)
    loss = torch.zeros((), dtype=torch.float64, device=DEV)
    rc = _lib.hip().lpf_skipgram_coef_f32(c.n, c.spec.dim, table.data_ptr(), table.stride(0), L, ctx, pos.data_ptr(),
                                          pos.shape[1], pos.stride(0), neg.data_ptr(), neg.shape[1], neg.stride(0),
                                          coef.data_ptr(), ids.data_ptr(), ids[M:].data_ptr(), partial.data_ptr(),
                                          partial.numel(), loss.data_ptr(), 0)
    assert rc == 0
    torch.cuda.synchronize()
    return coef, ids, loss


def _grad(n, dim, table, coef, occ_other, occ_pair, seg, groups=0):
    """lpf_skipgram_grad_rows_f32 alone: grad float32 [U, dim]."""
    U, n_occ = seg.numel() - 1, occ_other.numel()
    grad = torch.full((U, dim), float("nan"), dtype=torch.float32, device=DEV)
    scratch = torch.full((-(-n_occ // SC.CHUNK), dim), float("nan"), dtype=torch.float32, device=DEV)
    rc = _lib.hip().lpf_skipgram_grad_rows_f32(n, dim, table.data_ptr(), table.stride(0), coef.numel(),
                                               coef.data_ptr(), n_occ, occ_other.data_ptr(), occ_pair.data_ptr(), U,
                                               seg.data_ptr(), grad.data_ptr(), dim, scratch.data_ptr(),
                                               scratch.shape[0], groups, 0)
    assert rc == 0
    torch.cuda.synchronize()
    return grad


def _ref_keys(ref):
    return torch.cat([ref.centre, ref.other]).to(torch.int32).to(DEV)


@pytest.mark.parametrize("name", SC.NAMES)
def test_coefficients_ids_and_loss(name):
    c, table, pos, neg = _dev(name)
    ref = SC.reference(name)
    coef, ids, loss = _coef(c, table, pos, neg)
    M = ref.coef.numel()
    assert torch.equal(ids.cpu().to(torch.int64), torch.cat([ref.centre, ref.other]))
    bad = ref.centre < 0
    assert bool(bad.any()) == c.spec.bad and (coef.cpu()[bad] == 0).all()
    b_l, b_g = SC.coef_bound(c, c.table, ref, c1=1.0)
    err = (coef.cpu().to(torch.float64) - ref.coef).abs()
    ratio = float((err[~bad] / b_g[~bad]).max())
    # the loss moves by at most scale |dl| per pair (|dloss/dl| <= scale), in fp64 beyond that
    loss_bound = float((SC.pair_scale(c, M) * b_l).sum())
    loss_ratio = abs(float(loss.cpu() - ref.loss)) / loss_bound
    print(name, "coefficient: worst |dg| / (u (scale L1 / 4 + |g|)) =", round(ratio, 3), " loss:", round(loss_ratio, 4))
    assert ratio <= SC.C1 and loss_ratio <= SC.C1
    assert loss.dtype == torch.float64 and loss.dim() == 0


@pytest.mark.parametrize("name", SC.NAMES)
def test_gradient_rows(name):
    """(a) the entry on its own: the reference's coefficients rounded to fp32 and its ids in; (b) behind the coef
    entry: the device's coefficients in, held to the bound that carries the coefficients' bound through the sum."""
    c, table, pos, neg = _dev(name)
    ref = SC.reference(name)
    rows, seg, occ_other, occ_pair = skipgram.occurrence_list(_ref_keys(ref))
    lead = 1 if c.spec.bad else 0                                          # the segment of row -1 comes first
    assert torch.equal(rows[lead:].cpu().to(torch.int64), ref.rows) and (lead == 0 or int(rows[0]) == -1)
    own = SC.grad_bound(c.table, ref, None, own_only=True)
    grad = _grad(c.n, c.spec.dim, table, ref.coef.to(torch.float32).to(DEV), occ_other, occ_pair, seg)
    if lead:
        assert not grad[0].any()
    err = (grad[lead:].cpu().to(torch.float64) - ref.grad).abs()
    ratio = float((err / (U23 * own)).max())
    coef, ids, _ = _coef(c, table, pos, neg)
    chained = _grad(c.n, c.spec.dim, table, coef, *skipgram.occurrence_list(ids)[2:4], seg)
    _, b_g = SC.coef_bound(c, c.table, ref)
    err2 = (chained[lead:].cpu().to(torch.float64) - ref.grad).abs()
    worst2 = float((err2 / SC.grad_bound(c.table, ref, b_g)).max())
    print(name, "gradient: worst |d grad| / (u sum |g| |E|) =", round(ratio, 3), " behind the coef entry, error / bound:",
          round(worst2, 3), " longest segment", int((seg[1:] - seg[:-1]).max()))
    assert ratio <= SC.C2 and worst2 <= 1.0


@pytest.mark.parametrize("name", ("C_d128", "S_d36_ctx2", "S_d4_onewindow", "iso_d512"))
def test_sparse_adam_rows(name):
    """The reference's second-step gradient rows rounded to fp32 in, so the inputs are identical; the fp64 formulas
    on those fp32 inputs are the expectation."""
    c = SC.case(name)
    table, state, ref = SC.second(name)
    grad = ref.grad.to(torch.float32)
    want = SC.adam_expected(table, state, ref.rows, grad, c3=1.0)
    t, m, v = table.to(DEV), state.exp_avg.to(DEV), state.exp_avg_sq.to(DEV)
    rows, g = ref.rows.to(torch.int32).to(DEV), grad.to(DEV)
    b1, b2, step = 0.9, 0.999, state.step + 1
    rc = _lib.hip().lpf_sparse_adam_rows_f32(c.n, c.spec.dim, t.data_ptr(), t.stride(0), m.data_ptr(), v.data_ptr(),
                                             m.stride(0), rows.numel(), rows.data_ptr(), g.data_ptr(), g.stride(0),
                                             SC.LR, b1, b2, 1e-8, step, 1.0 - b1 ** step, 1.0 - b2 ** step, 0)
    assert rc == 0 and step == 2
    torch.cuda.synchronize()
    ratios = {}
    for key, got in (("m", m), ("v", v), ("p", t)):
        err = (got.cpu().to(torch.float64)[ref.rows] - want[key]).abs()
        ratios[key] = float((err / want["b_" + key]).max())
    print(name, "Adam: worst error / (u magnitude):", {k: round(r, 3) for k, r in ratios.items()})
    assert max(ratios.values()) <= SC.C3
    untouched = torch.ones(c.n, dtype=torch.bool)
    untouched[ref.rows] = False
    for got, before in ((t, table), (m, state.exp_avg), (v, state.exp_avg_sq)):
        assert torch.equal(got.cpu()[untouched], before[untouched])


def test_gradient_sums_are_exact_on_integers_at_every_chunk_edge():
    p = {k: v.to(DEV) for k, v in SC.integer_lists().items()}
    n, dim = p["table"].shape
    first = _grad(n, dim, p["table"], p["coef"], p["occ_other"], p["occ_pair"], p["seg"])
    assert torch.equal(first.cpu().to(torch.float64), p["want"].cpu())
    for groups in (1, 3, 1000):
        again = _grad(n, dim, p["table"], p["coef"], p["occ_other"], p["occ_pair"], p["seg"], groups)
        assert torch.equal(first, again), groups
    # the star: the hub's row (thousands of occurrences) with an integer table and integer coefficients
    c, ref = SC.case("star_d128"), SC.reference("star_d128")
    rng = np.random.default_rng(9)
    table = torch.from_numpy(rng.integers(-3, 4, (c.n, c.spec.dim)).astype(np.float32))
    coef = torch.from_numpy(rng.integers(-4, 5, ref.coef.numel()).astype(np.float32))
    row, other, pair = SC.occurrences(ref)
    want = torch.zeros((ref.rows.numel(), c.spec.dim), dtype=torch.float64)
    want.index_add_(0, torch.searchsorted(ref.rows, row), coef.double()[pair, None] * table.double()[other])
    assert float(want.abs().max()) < 2 ** 24 and int((row == 0).sum()) > 8 * SC.CHUNK
    rows, seg, occ_other, occ_pair = skipgram.occurrence_list(_ref_keys(ref))
    got = _grad(c.n, c.spec.dim, table.to(DEV), coef.to(DEV), occ_other, occ_pair, seg)
    assert torch.equal(got.cpu().to(torch.float64), want)
    assert int(rows[0]) == 0 and torch.equal(got[0].cpu().to(torch.float64), want[0])


def test_two_runs_and_any_launch_shape_give_the_same_bits():
    for name in ("star_d128", "C_d512_long"):
        c, table, pos, neg = _dev(name)
        out = []
        for _ in range(2):
            t, st = table.clone(), skipgram.skipgram_state(table)
            losses = [skipgram.skipgram_step(t, st, pos, neg, c.spec.context, lr=SC.LR) for _ in range(2)]
            out.append((t, st.exp_avg, st.exp_avg_sq, torch.stack(losses)))
            assert st.step == 2
        for a, b in zip(*out):
            assert torch.equal(a, b), name
        ref = SC.reference(name)
        rows, seg, occ_other, occ_pair = skipgram.occurrence_list(_ref_keys(ref))
        coef = ref.coef.to(torch.float32).to(DEV)
        first = _grad(c.n, c.spec.dim, table, coef, occ_other, occ_pair, seg)
        for groups in (1, 7, 4096):
            assert torch.equal(first, _grad(c.n, c.spec.dim, table, coef, occ_other, occ_pair, seg, groups)), groups
    g = RC.case("C").csr.to_device(DEV)
    kw = dict(walk_length=10, context=5, walks_per_node=1, batch_walks=64, lr=0.05, trainer="device", seed=3)
    (e1, l1), (e2, l2) = node2vec_embeddings(g, 16, **kw), node2vec_embeddings(g, 16, **kw)
    assert torch.equal(e1, e2) and l1 == l2


@pytest.mark.parametrize("name", ("C_d128", "bad_d36"))
def test_a_whole_step(name):
    """skipgram_step: the loss, the first moment (0.1 grad at step 1, so the gradient bound applies) and which rows
    move.  The updated table is NOT held to a bound through the kernel's own gradients: at step 1 the update is
    lr g / (|g| + eps / sqrt(1 - beta2)), whose slope near g = 0 is lr / 3e-7."""
    c, table, pos, neg = _dev(name)
    ref = SC.reference(name)
    before = table.clone()
    state = skipgram.skipgram_state(table)
    loss = skipgram.skipgram_step(table, state, pos, neg, c.spec.context, lr=SC.LR)
    assert loss.is_cuda and loss.dtype == torch.float64 and loss.dim() == 0 and state.step == 1
    b_l, b_g = SC.coef_bound(c, c.table, ref)
    assert abs(float(loss.cpu() - ref.loss)) <= float((SC.pair_scale(c, ref.coef.numel()) * b_l).sum())
    bound = 0.1 * SC.grad_bound(c.table, ref, b_g) + SC.C3 * U23 * 0.1 * ref.grad.abs()
    assert ((state.exp_avg.cpu().to(torch.float64)[ref.rows] - ref.exp_avg[ref.rows]).abs() <= bound).all()
    touched = torch.zeros(c.n, dtype=torch.bool)
    touched[ref.rows] = True
    moved = (table != before).any(dim=1).cpu()
    assert not moved[~touched].any() and not state.exp_avg.cpu()[~touched].any()
    assert torch.isfinite(table).all() and int(moved.sum()) > 0.9 * int(touched.sum())
    # a second step from here runs and counts
    skipgram.skipgram_step(table, state, pos, neg, c.spec.context, lr=SC.LR)
    assert state.step == 2 and torch.isfinite(table).all()
    with pytest.raises(ValueError):
        skipgram.skipgram_step(table, state, pos.t(), neg, c.spec.context)          # the view, not the buffer
    with pytest.raises(ValueError):
        skipgram.skipgram_step(table[:, :3], state, pos, neg, c.spec.context)


def test_node2vec_embeddings_on_the_device_separate_two_cliques():
    case = RC.case("C")
    g = case.csr.to_device(DEV)
    emb, losses = node2vec_embeddings(g, 16, walk_length=10, context=5, walks_per_node=4, epochs=2, batch_walks=64,
                                      lr=0.05, trainer="device")
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


def test_one_device_step_equals_one_torch_step():
    """One optimiser step of either trainer from the same seed: the same table, walks and negatives.  The tables are
    compared on the rows whose every gradient element exceeds 1e-3 in magnitude (printed: how many of the touched rows
    that keeps; at least half), where the update's slope is at most lr 3.2e-7 / 1e-6, with the gradient-row bound on
    both sides carried through that slope, plus the update's own fp32 arithmetic."""
    case = RC.case("C")
    g = case.csr.to_device(DEV)
    dim, L, ctx, B, lr, seed = 4, 10, 5, 4, 0.05, 2
    kw = dict(walk_length=L, context=ctx, walks_per_node=1, batch_walks=B, seed=seed, max_steps=1)
    dev_t, dev_l = node2vec_embeddings(g, dim, lr=lr, trainer="device", **kw)
    tor_t, tor_l = node2vec_embeddings(g, dim, lr=lr, trainer="torch", **kw)
    start_t, _ = node2vec_embeddings(g, dim, lr=0.0, trainer="device", **kw)          # lr 0: the initial table
    # the step's inputs, drawn as node2vec_embeddings draws them
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    table = torch.randn((case.n, dim), generator=gen, device=DEV, dtype=torch.float32)
    assert torch.equal(table, start_t)
    start = torch.randperm(case.n, generator=gen, device=DEV)[:B]
    walks = random_walks(g, start, length=L, seed=seed, walk_base=0).walks
    noise = torch.randint(case.n, (B, L), generator=gen, device=DEV)
    neg = torch.cat([start[:, None], noise], dim=1).to(torch.int32).t().contiguous()
    ref = skipgram.skipgram_reference(table, skipgram.skipgram_state(table.cpu()), walks.t(), neg, ctx, lr=lr)
    assert abs(dev_l[0] - float(ref.loss)) < 1e-5 and abs(tor_l[0] - float(ref.loss)) < 1e-5
    keep = (ref.grad.abs() > 1e-3).all(dim=1)
    print("rows compared:", int(keep.sum()), "of", ref.rows.numel(), "touched")
    assert 2 * int(keep.sum()) >= ref.rows.numel()
    class _C:                                                               # what coef_bound reads of a case
        spec = SC.Spec("C", dim, L, ctx, B, 0)
        pos = walks.t()
    b_g = SC.coef_bound(_C, table.cpu(), ref)[1]
    slope = lr * 3.2e-7 / 1e-6
    rows = ref.rows[keep]
    a, b = dev_t.cpu().to(torch.float64)[rows], tor_t.cpu().to(torch.float64)[rows]
    upd = (ref.table - table.cpu().to(torch.float64))[rows].abs()
    bound = 2 * slope * SC.grad_bound(table.cpu(), ref, b_g)[keep] + 2 * SC.C3 * U23 * (a.abs() + upd)
    worst = float(((a - b).abs() / bound).max())
    print("device against torch, worst |difference| / bound:", worst)
    assert worst <= 1.0
    for t in (dev_t, tor_t):                                                # both are near the reference's step
        assert ((t.cpu().to(torch.float64)[rows] - ref.table[rows]).abs() <= bound).all()
    untouched = torch.ones(case.n, dtype=torch.bool)
    untouched[ref.rows] = False
    assert torch.equal(dev_t.cpu()[untouched], table.cpu()[untouched])


def test_c_entries_reject_bad_arguments_without_a_launch():
    c, table, pos, neg = _dev("S_d36_ctx2")
    hip = _lib.hip()
    n, dim, L, ctx = c.n, c.spec.dim, c.spec.length, c.spec.context
    Wp, Wn, ldp = pos.shape[1], neg.shape[1], pos.stride(0)
    M = (Wp + Wn) * (L + 2 - ctx) * (ctx - 1)
    coef = torch.full((M,), -7.0, dtype=torch.float32, device=DEV)
    ids = torch.full((2 * M,), -7, dtype=torch.int32, device=DEV)
    partial = torch.full((M,), -7.0, dtype=torch.float64, device=DEV)
    loss = torch.full((), -7.0, dtype=torch.float64, device=DEV)
    tp, pp, np_, cp, ip, xp, sp, lp = (t.data_ptr() for t in (table, pos, neg, coef, ids, ids[M:], partial, loss))

    def coef_call(n=n, dim=dim, tp=tp, ldt=dim, L=L, ctx=ctx, pp=pp, Wp=Wp, ldp=ldp, np_=np_, Wn=Wn, ldn=ldp, cp=cp,
                  ip=ip, xp=xp, sp=sp, plen=M, lp=lp):
        return hip.lpf_skipgram_coef_f32(n, dim, tp, ldt, L, ctx, pp, Wp, ldp, np_, Wn, ldn, cp, ip, xp, sp, plen, lp, 0)
    for bad in (dict(n=-1), dict(n=1 << 31), dict(dim=34), dict(dim=0), dict(dim=516), dict(tp=None), dict(tp=tp + 4),
                dict(ldt=dim - 4), dict(ldt=dim + 2), dict(L=0), dict(ctx=1), dict(ctx=L + 2), dict(pp=None),
                dict(np_=None), dict(Wp=-1), dict(Wn=-1), dict(ldp=Wp - 1), dict(ldn=Wn - 1), dict(cp=None),
                dict(ip=None), dict(xp=None), dict(sp=None), dict(lp=None), dict(plen=1), dict(plen=-1)):
        assert coef_call(**bad) == -1, bad
    assert coef_call(Wp=0, Wn=0) == 0 and coef_call(Wp=0, Wn=0, pp=None, np_=None, cp=None, tp=None) == 0

    U, n_occ = 5, 40
    seg = torch.tensor([0, 8, 16, 24, 32, 40], dtype=torch.int64, device=DEV)
    occ = torch.zeros(n_occ, dtype=torch.int32, device=DEV)
    grad = torch.full((U, dim), -7.0, dtype=torch.float32, device=DEV)
    scratch = torch.full((1, dim), -7.0, dtype=torch.float32, device=DEV)
    op, gp, sgp, scp = occ.data_ptr(), grad.data_ptr(), seg.data_ptr(), scratch.data_ptr()

    def grad_call(n=n, dim=dim, tp=tp, ldt=dim, M=M, cp=cp, n_occ=n_occ, oo=op, opair=op, U=U, sgp=sgp, gp=gp, ldg=dim,
                  scp=scp, srows=1, groups=0):
        return hip.lpf_skipgram_grad_rows_f32(n, dim, tp, ldt, M, cp, n_occ, oo, opair, U, sgp, gp, ldg, scp, srows,
                                              groups, 0)
    for bad in (dict(n=-1), dict(dim=34), dict(dim=516), dict(tp=None), dict(ldt=dim - 4), dict(M=-1), dict(cp=None),
                dict(n_occ=-1), dict(oo=None), dict(opair=None), dict(U=-1), dict(sgp=None), dict(gp=None),
                dict(gp=gp + 4), dict(ldg=dim - 4), dict(scp=None), dict(srows=0), dict(groups=-1)):
        assert grad_call(**bad) == -1, bad
    assert grad_call(U=0) == 0 and grad_call(U=0, sgp=None, gp=None, scp=None, tp=None) == 0

    m = torch.full((n, dim), -7.0, dtype=torch.float32, device=DEV)
    v = torch.full((n, dim), -7.0, dtype=torch.float32, device=DEV)
    rows = torch.arange(U, dtype=torch.int32, device=DEV)
    keep = table.clone()
    mp, vp, rp = m.data_ptr(), v.data_ptr(), rows.data_ptr()

    def adam_call(n=n, dim=dim, tp=tp, ldt=dim, mp=mp, vp=vp, lds=dim, U=U, rp=rp, gp=gp, ldg=dim, lr=0.01, b1=0.9,
                  b2=0.999, eps=1e-8, step=1, bias1=0.1, bias2=0.001):
        return hip.lpf_sparse_adam_rows_f32(n, dim, tp, ldt, mp, vp, lds, U, rp, gp, ldg, lr, b1, b2, eps, step, bias1,
                                            bias2, 0)
    for bad in (dict(n=-1), dict(dim=34), dict(dim=516), dict(tp=None), dict(ldt=dim - 4), dict(mp=None), dict(vp=None),
                dict(lds=dim + 1), dict(U=-1), dict(rp=None), dict(gp=None), dict(ldg=dim - 4), dict(lr=-1.0),
                dict(b1=1.0), dict(b2=-0.1), dict(eps=-1.0), dict(step=0), dict(bias1=0.0), dict(bias2=1.5)):
        assert adam_call(**bad) == -1, bad
    assert adam_call(U=0) == 0 and adam_call(U=0, rp=None, gp=None) == 0
    torch.cuda.synchronize()
    for t in (coef, ids, partial, loss, grad, scratch, m, v):
        assert (t == -7).all()                                                 # nothing ran
    assert torch.equal(table, keep)
