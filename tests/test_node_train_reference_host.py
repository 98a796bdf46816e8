"""The references and inputs of tests/node_train_reference.py checked on the CPU, so that the GPU tests of the node-stage
training kernels compare with something that is itself pinned: the closed-form fp64 LayerNorm / ReLU / dropout backward
is what torch autograd gives in fp64, the inputs have the properties the GPU tests rely on (at most 1 % of the elements
within the kink margin, the never- and the always-active column, constant rows), a one-pass variance in fp32 does miss
the bound on them, the restated launch arithmetic gives the numbers the cases were chosen for, and the integer product
is exact in fp32."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.nn.functional as F

from lpformer_amd import train
from tests import node_train_reference as R

VARIANTS = ("plain", "relu", "drop")


def _autograd64(c, variant, keep):
    """Gradients of sum(y dy), y = [dropout(ReLU(]LN(x0 + b0)[))], by torch autograd in fp64; b0 = 0 is a bias added in
    front of the LayerNorm, whose gradient is what the kernels call dxsum."""
    x0, gamma, beta = (t.double().requires_grad_() for t in (c.x, c.gamma, c.beta))
    b0 = torch.zeros(c.d, dtype=torch.float64, requires_grad=True)
    y = F.layer_norm(x0 + b0, (c.d,), gamma, beta, eps=R.LN_EPS)
    if variant != "plain":
        y = torch.relu(y)
    if variant == "drop":
        y = y * keep.double() / (1 - R.LN_DROP_P)
    (y * c.dy.double()).sum().backward()
    return x0.grad, gamma.grad, beta.grad, b0.grad


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("d,m", [(36, 300), (132, 257)])
def test_closed_form_backward_is_fp64_autograd(d, m, variant):
    """dx, dgamma, dbeta and dxsum of ``ln_bwd64`` against autograd to 1e-11 of each tensor's largest entry, on the
    inputs the GPU test draws (scaled and shifted rows, three constant rows, gamma with an exact 0 and negative
    entries, the -10 and +10 columns), the dropout mask being ``train.drop_keep_mask`` at the GPU test's seed."""
    c = R.ln_case(d, m)
    keep = train.drop_keep_mask(R.LN_DROP_SEED, R.LN_DROP_P, m, d, "cpu") if variant == "drop" else None
    assert R.LN_DROP_SEED >> 32 != 0
    if keep is not None:
        assert abs(float(keep.double().mean()) - (1 - R.LN_DROP_P)) < 0.02
    got = R.ln_bwd64(c.x, c.dy, c.gamma, c.beta, relu=variant != "plain", keep=keep, drop_p=R.LN_DROP_P)
    want = _autograd64(c, variant, keep)
    for name, g, w in zip(("dx", "dgamma", "dbeta", "dxsum"), got, want):
        assert g.dtype == torch.float64 and g.shape == w.shape
        assert float((g - w).abs().max()) <= 1e-11 * max(1.0, float(w.abs().max())), (name, variant)
    if variant != "plain":
        assert float(got[1][R.COL_OFF]) == 0.0 and float(got[2][R.COL_OFF]) == 0.0      # the never-active column
        assert float(got[1][R.COL_ON]) != 0.0 and float(got[2][R.COL_ON]) != 0.0        # the always-active one


@pytest.mark.parametrize("d", R.LN_WIDTHS)
def test_layernorm_inputs_stay_clear_of_the_kink(d):
    """Every (width, M) input of the GPU test: at most 1 % of the elements lie within LN_KINK of the ReLU's kink (the
    expectation is 2 * 1e-4 * 0.4, the density of a unit normal at 0), dy is 0 there and nowhere else by design, and
    the row counts are the edges of the launch arithmetic they are meant to be."""
    lanes, per_wg = R.ln_lanes(d), 256 // R.ln_lanes(d)
    assert lanes in (8, 16, 32, 64) and 4 * lanes >= d and (lanes == 8 or 2 * lanes < d)
    counts = R.ln_row_counts(d)
    assert counts[:3] == (0, 1, per_wg + 1)
    above = counts[3] - R.LN_BLOCK_CAP * per_wg
    assert counts[3] % 2 == 1 and 500 <= above <= 1500 and above < per_wg * R.LN_BLOCK_CAP // 2
    for m in counts:
        c = R.ln_case(d, m)
        assert c.x.shape == (m, d) and c.x.dtype == c.dy.dtype == torch.float32
        assert c.undecided <= R.UNDECIDED_CAP, (d, m, c.undecided)
        if m > 1000:
            assert c.undecided < 1e-3                  # (the expectation, with room: the cap is never what holds)
        near = R.ln_pre64(c.x, c.gamma, c.beta).abs() <= R.LN_KINK
        assert bool((c.dy[near] == 0).all()) and int((c.dy == 0).sum()) == int(near.sum())
        if m >= 4:
            assert int(c.const.sum()) == 3 and bool((c.x[c.const] == 1.0).all())
            _, rstd = R.ln_stats64(c.x)
            assert bool((rstd[c.const] == 1.0 / torch.sqrt(torch.tensor(R.LN_EPS, dtype=torch.float64))).all())


def _ln_bwd32(c, one_pass):
    """The plain backward restated in fp32 torch; ``one_pass``: the variance as E[x^2] - mean^2."""
    x, dy, gamma = c.x, c.dy, c.gamma
    mean = x.mean(1, keepdim=True)
    var = ((x * x).mean(1, keepdim=True) - mean * mean).clamp_min(0) if one_pass else ((x - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + np.float32(R.LN_EPS))
    xh = (x - mean) * rstd
    g = dy * gamma
    return rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))


@pytest.mark.parametrize("d", [w for w in R.LN_WIDTHS if w >= 32])
def test_a_one_pass_variance_misses_the_row_bound_on_these_inputs(d):
    """The row-by-row bound the GPU test holds dx to at D >= 32 (``ln_row_tol``: 1e-4 max(1, max|want_i|) per row)
    passes a two-pass fp32 restatement with a factor 5 to spare and fails a one-pass one, on the rows with a small
    scale and a large mean.  Taken over the whole tensor the same 1e-4 is set by the constant rows, whose rstd of 316
    makes max|dx| several hundred, and the one-pass variance passes it: hence the rows.  (At D = 4 a row's own spread
    can by chance be a hundredth of its scale, the fp32 rounding of the mean is no longer small against it and the
    two-pass restatement itself reaches the row bound: the GPU test holds D = 4 to the whole-tensor bound, taken
    separately over the constant rows and the others.)"""
    c = R.ln_case(d, R.ln_row_counts(d)[3])
    want = R.ln_bwd64(c.x, c.dy, c.gamma)[0]
    two, one = ((_ln_bwd32(c, p).double() - want).abs() for p in (False, True))
    tol = R.ln_row_tol(want)
    # (here: two-pass 0.007 .. 0.043, one-pass 2.5 .. 5.9 of the row bound and 0.06 .. 0.28 of the whole-tensor bound;
    # the asserted figures leave room for another order of the fp32 sums)
    assert float((two / tol).max()) <= 0.2 and float((one / tol).max()) > 1.5
    whole = 1e-4 * float(want.abs().max())
    assert float(one.max()) <= whole and float(want[c.const].abs().max()) > 5 * float(want[~c.const].abs().max())


def test_gemm_tn_launch_arithmetic_and_exactness():
    """The numbers the row counts of (B) were chosen for, and the premise of the bitwise comparison: the int64 product is
    what fp64 and -- in two different summation orders -- fp32 give, bit for bit."""
    assert [R.tn_chunk_rows(m) for m in R.TN_ROWS] == [64, 64, 64, 64, 64, 72]
    assert [R.tn_chunks(m) for m in R.TN_ROWS] == [1, 1, 1, 2, 5, 457]
    assert 32837 - 456 * 72 == 5                              # the last chunk: five rows of one round
    assert [R.tn_groups(n) for n, _ in R.TN_SHAPES] == [4, 2, 2, 1, 4, 4]
    assert [k <= 64 for _, k in R.TN_SHAPES] == [True, True, False, False, True, False]
    assert R.tn_workspace_floats(0, 7, 5) == 0 and R.tn_workspace_floats(65, 36, 64) == 2 * 2 * (36 * 64 + 36)
    m, n, k = 32837, 36, 64
    a, b = R.tn_case(m, n, k)
    assert set(a.unique().tolist()) == set(b.unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    want, cs = R.tn_exact(a, b)
    assert want.dtype == torch.int64 and int(want.abs().max()) < 2 ** 24 and int(cs.abs().max()) < 2 ** 24
    assert not torch.equal(want[:, :n], want[:, :n].t()) and int(cs.min()) > 0       # asymmetric, no cancelling sums
    assert torch.equal((a.double().t() @ b.double()).long(), want)
    assert torch.equal(a.t() @ b, want.float())
    assert torch.equal(a[:20000].t() @ b[:20000] + a[20000:].t() @ b[20000:], want.float())
    assert torch.equal(a.sum(0), cs.float())


def _gcn_u64(dim):
    r, c, v = R.gcn_graph()
    n = R.GCN_NODES
    p = R.layer_params(n, R.GCN_IN, dim, 300 + dim)
    a = sp.csr_matrix((v.astype(np.float64), (r, c)), shape=(n, n))
    u = a @ (p.x.double() @ p.w.double().t()).numpy() + p.b.double().numpy()
    return torch.from_numpy(u), p, a


@pytest.mark.parametrize("dim", [36, 256])
def test_gcn_layer_inputs_stay_clear_of_the_kink(dim):
    """The ``GcnLayerFn`` inputs of the GPU test (D = 36 as asked; D = 256 too, it costs nothing): with u = A (x W^T) + b
    from a scipy sparse A in fp64, at most 1 % of the elements lie within the margin that covers an fp32 u.  The graph
    has what the GPU test asserts: a hub row and an empty row in A and in A^T, no duplicate entry, 4603 rows = 507 above
    one trip of the capped LayerNorm backward at D = 256."""
    u, p, a = _gcn_u64(dim)
    assert R.GCN_NODES - R.ln_trip_rows(256) == 507
    for deg in (np.diff(a.indptr), np.diff(a.tocsc().indptr)):
        assert deg.max() > R.LONG_ROW and deg.min() == 0
    near = R.relu_ln_undecided(u, p.g, p.be)
    share = float(near.double().mean())
    assert 0 < share <= R.UNDECIDED_CAP, share
    # the margin is the stated one: at the largest |pre| still undecided, 10 x the forward tolerance of u, as rstd gamma
    xh, rstd = R.ln_stats64(u)
    pre = xh * p.g.double() + p.be.double()
    bound = 10 * 2e-5 * max(1.0, float(u.abs().max())) * rstd * p.g.double().abs()
    assert torch.equal(near, pre.abs() <= bound)


def test_planting_gives_hub_and_empty_rows_both_ways():
    """``_plant`` on a ring (every row and column one entry): afterwards A and A^T each have a row of more than 128
    entries and an empty row, and no entry is double."""
    n = 400
    r = np.arange(n, dtype=np.int64)
    c = (r + 1) % n
    v = np.full(n, 0.1, np.float32)
    r2, c2, v2 = R._plant(r, c, v, n, np.random.default_rng(0))
    assert r2.size == c2.size == v2.size and np.unique(r2 * n + c2).size == r2.size
    for ends in (r2, c2):
        deg = np.bincount(ends, minlength=n)
        assert deg.max() > R.LONG_ROW and deg.min() == 0
