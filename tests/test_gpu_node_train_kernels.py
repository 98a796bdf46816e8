"""The node-stage training kernels -- the LayerNorm backward family of csrc/rowwise.hip, C = A^T B of csrc/gemm_f32.hip,
and the operators of train.py that the one-launch layer does not take -- against the fp64 restatements of
tests/node_train_reference.py, at the row counts where their launch arithmetic changes, with padded leading dimensions
and with workspaces and outputs preset to NaN (an unwritten or over-read partial becomes a NaN).

Reach map -- entry point: test: the cap or edge it crosses.
  lpf_layernorm_bwd_f32              test_layernorm_backward_direct (A), once per width.  G lanes own a row (8 / 16 / 32 /
  lpf_layernorm_relu_bwd_f32           64 at D <= 32 / 64 / 128 / above), a workgroup holds 256 / G rows, ln_bwd_launch
  lpf_layernorm_relu_drop_bwd_f32      starts at most 1024 workgroups: one trip holds 32768 / 16384 / 8192 / 4096 rows.
                                       Widths 4 (one live lane of 8), 32, 36 (9 of 16 lanes), 64, 128, 132 (33 of 64), 256.
                                       M = 0 (no kernel but the reduction: exact zeros, dx untouched); 1; 256 / G + 1 (one
                                       row into a second workgroup, whose other groups are dead); one trip + 701 / 1001 /
                                       777 / 1233 / 907 / 555 / 1499 rows (odd: a second trip taken by a few groups only).
                                       ldx = D + 4, ldy = D + 8, lddx = D + 12; the third partial (dxsum); p = 0.25 with
                                       a seed whose high half is not 0; drop_p = 0 through the drop entry.
  lpf_gemm_tn_f32                    test_gemm_tn_exact (B), once per (N, K); M = 0, 1, 9, 63, 65, 257, 32837.  A chunk is
  lpf_gemm_tn_colsum_f32               max(64, ceil(M / 512)) rows in whole rounds of 8: 64 up to M = 257 (1, 1, 1, 2, 5
                                       chunks; 1 / 9 / 63: a partial round, two rounds, all but one row of the chunk;
                                       65: one row into a second chunk; the four-deep pipeline prefetches past every one
                                       of these ends), 72 at M = 32837 (457 chunks, the last of 5 rows).  (32, 32): 4 row
                                       groups, <2, 4>; (36, 64): 2 groups, a second 32-row tile of 4 live rows, K = 64
                                       the last <2, 4>; (64, 128): 2 groups, <4, 3>; (132, 260): 1 group, a second 128-row
                                       tile of 4 rows whose wavefronts 1 .. 3 leave early, three column tiles, the last
                                       of 4 columns; (7, 5): one ragged tile; (1, 1433): 12 column tiles.  lda = N + 3,
                                       ldb = K + 1, ldc = K + 5 (no alignment left); N = 0, K = 0.
  train.GcnLayerFn                   test_gcn_layer_fn (C) at D = 256 (n = 4603 = 4096 + 507: the LayerNorm backward's
                                       second trip; gemm_tn with K = 40) and D = 36 (9 of 16 lanes; N = 36: 2 row groups);
                                       hub rows (> 128 entries) and empty rows in A and in A^T.
  train.SpmmFn                       test_spmm_fn (C) at D = 36, same graph.
  train.LnReluFn                     test_ln_relu_fn (C) at D = 256, M = 1 and 4603 (behind train.linear: gemm_tn_colsum).

Tolerances are the ones the suite already holds these kernels to: (A) 1e-4 max(1, max|want|) for dx, dgamma, dbeta and
dxsum (test_layernorm_backward_kernel); (B) none, the inputs are small integers and every sum is exact; (C) outputs
2e-5 max(1, max|ref|), gradients 1e-4 max(1, max|want|) (test_fused_layer_backward_matches_fp64_autograd).  On top of
the whole-tensor bound (A) holds dx to the same 1e-4 taken over the constant rows and over the other rows separately,
and at D >= 32 row by row -- the constant rows' rstd of 316 sets the whole-tensor bound, which a one-pass variance would
pass (tests/test_node_train_reference_host.py shows both).  Every test prints its worst err / tolerance, and every
launch is made twice and compared bitwise: each reduction here has a fixed order.

The ReLU kink: the backward recomputes the ReLU's mask from x in fp32; where the fp64 argument lies within a stated
margin of 0 the upstream gradient is set to 0 -- chosen from the reference alone --, so that either side gives the same
gradients.  No element is left out of a comparison and no mask is read back.  At most 1 % of a case's elements may be
undecided (asserted; measured 0 .. 0.8 % in (A), a single element of 132 at M = 1, and 0.4 % in (C)).

No number in this file was known before it was written; what the card measured is recorded in the docstrings.
"""
import pytest
import torch

from lpformer_amd import _lib, graph, train
from tests import node_train_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SENTINEL = 7.0
FWD_TOL, GRAD_TOL = 2e-5, 1e-4


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _tol(want, rel):
    return rel * max(1.0, float(want.abs().max())) if want.numel() else rel


def _err(got, want):
    return float((got.double() - want.double()).abs().max()) if want.numel() else 0.0


def _padded(t, pad, fill):
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=torch.float32, device=DEV)
    buf[:, :t.shape[1]] = t
    return buf


# ------------------------------------------------------------------------------------------------ (A) LayerNorm backward
LN_ENTRIES = ("plain", "relu", "drop")


def _ln_launch(entry, m, d, xb, dyb, gamma, beta, ws, drop_p=R.LN_DROP_P):
    """One launch of a LayerNorm backward entry point on padded buffers -> (dx buffer, [dgamma, dbeta, dxsum]); the
    workspace and the three outputs are NaN when the launch starts, dx holds the sentinel (three rows of it at M = 0)."""
    lib, P, st = _lib.hip(), _lib.ptr, _stream()
    dxb = torch.full((max(m, 3), d + 12), SENTINEL, dtype=torch.float32, device=DEV)
    outs = torch.full((3, d), NAN, dtype=torch.float32, device=DEV)
    ws.fill_(NAN)
    ld = (xb.stride(0), dyb.stride(0), dxb.stride(0))
    assert ld == (d + 4, d + 8, d + 12)
    if entry == "plain":
        rc = lib.lpf_layernorm_bwd_f32(m, d, P(xb), ld[0], P(dyb), ld[1], P(gamma), P(dxb), ld[2], P(outs[0]), P(outs[1]),
                                       P(ws), st)
    elif entry == "relu":
        rc = lib.lpf_layernorm_relu_bwd_f32(m, d, P(xb), ld[0], P(dyb), ld[1], P(gamma), P(beta), P(dxb), ld[2],
                                            P(outs[0]), P(outs[1]), P(outs[2]), P(ws), st)
    else:
        rc = lib.lpf_layernorm_relu_drop_bwd_f32(m, d, P(xb), ld[0], P(dyb), ld[1], P(gamma), P(beta), drop_p,
                                                 R.LN_DROP_SEED, P(dxb), ld[2], P(outs[0]), P(outs[1]), P(outs[2]), P(ws), st)
    _lib.check(rc, entry)
    torch.cuda.synchronize()
    return dxb, outs


@pytest.mark.parametrize("d", R.LN_WIDTHS)
def test_layernorm_backward_direct(d):
    """(A) The three entry points through the C ABI at M = 0, 1, 256 / G + 1 and just above one trip of the capped grid,
    on rows with a scale of 0.1 .. 10 and a mean of -5 .. 5, three constant rows, gamma with an exact 0 and negative
    entries, a never-active (beta = -10) and an always-active (beta = +10) column: dx, dgamma, dbeta and dxsum against
    the closed-form fp64 backward within 1e-4 max(1, max|want|) -- dx also over the constant and the other rows
    separately and, D >= 32, row by row --, the never-active column's dgamma and dbeta exactly 0, the padding of dx
    untouched, two runs bitwise equal, drop_p = 0 through the drop entry bitwise the relu entry.

    Measured on an MI355X, worst err / tolerance over the row counts and every asserted bound (all three entries within
    a factor 1.5 of each other):
        D        4       32      36      64      128     132     256
        plain    0.365   0.021   0.025   0.018   0.010   0.006   0.004
        relu     0.377   0.018   0.021   0.014   0.007   0.006   0.005
        drop     0.374   0.016   0.023   0.012   0.006   0.005   0.004
    The worst is always dx at the largest M -- by row at D >= 32, over the non-constant rows at D = 4, where a row of four
    values can by chance lie a hundredth of its scale apart and the fp32 mean is no longer exact against that (by row,
    printed and not asserted there: 0.62 .. 0.99, as for torch's own fp32 two-pass LayerNorm backward, 1.007).  dx over
    the whole tensor stays below 0.002 (0.17 at D = 4), dgamma below 0.013, dbeta below 0.004, dxsum below 0.005 (0.10
    at D = 4)."""
    lib = _lib.hip()
    lanes, per_wg = R.ln_lanes(d), 256 // R.ln_lanes(d)
    trip = R.LN_BLOCK_CAP * per_wg
    counts = R.ln_row_counts(d)
    # the launch arithmetic this test was sized for: a changed cap changes the workspace the library asks for
    assert int(lib.lpf_layernorm_bwd_workspace_floats(d)) == R.LN_BLOCK_CAP * 3 * d
    assert 4 * lanes >= d and (lanes == 8 or 2 * lanes < d) and trip == {8: 32768, 16: 16384, 32: 8192, 64: 4096}[lanes]
    assert counts[:3] == (0, 1, per_wg + 1) and counts[3] % 2 == 1 and 500 <= counts[3] - trip <= 1500
    ws = torch.empty(int(lib.lpf_layernorm_bwd_workspace_floats(d)), dtype=torch.float32, device=DEV)
    worst = {e: 0.0 for e in LN_ENTRIES}
    for m in counts:
        c = R.ln_case(d, m)
        assert c.undecided <= R.UNDECIDED_CAP, (d, m, c.undecided)
        x, dy, gamma, beta = (t.to(DEV) for t in (c.x, c.dy, c.gamma, c.beta))
        const = c.const.to(DEV)
        xb, dyb = _padded(x, 4, NAN), _padded(dy, 8, NAN)
        keep = train.drop_keep_mask(R.LN_DROP_SEED, R.LN_DROP_P, m, d, DEV)
        assert R.LN_DROP_SEED >> 32 != 0 and (m < 1000 or abs(float(keep.double().mean()) - 0.75) < 0.01)
        got = {}
        for entry in LN_ENTRIES:
            dxb, outs = _ln_launch(entry, m, d, xb, dyb, gamma, beta, ws)
            dxb2, outs2 = _ln_launch(entry, m, d, xb, dyb, gamma, beta, ws)
            n_out = 2 if entry == "plain" else 3
            assert torch.equal(dxb, dxb2) and torch.equal(outs[:n_out], outs2[:n_out]), (entry, m)
            assert bool((dxb[:, d:] == SENTINEL).all()), (entry, m)                  # nothing stored past D
            assert bool(torch.isnan(outs[n_out:]).all())
            got[entry] = (dxb, outs)
            if m == 0:
                assert bool((dxb == SENTINEL).all()) and int(torch.count_nonzero(outs[:n_out])) == 0, entry
                assert not bool(torch.isnan(outs[:n_out]).any())
                continue
            want = R.ln_bwd64(x, dy, gamma, beta, relu=entry != "plain", keep=keep if entry == "drop" else None,
                              drop_p=R.LN_DROP_P)
            dx = dxb[:m, :d]
            assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(outs[:n_out]).all()), (entry, m)
            ratios = {"dx": _err(dx, want[0]) / _tol(want[0], GRAD_TOL)}
            for rows, name in ((const, "dx const rows"), (~const, "dx other rows")):
                if bool(rows.any()):
                    ratios[name] = _err(dx[rows], want[0][rows]) / _tol(want[0][rows], GRAD_TOL)
            by_row = float(((dx.double() - want[0]).abs() / R.ln_row_tol(want[0], GRAD_TOL)).max())
            if d >= 32:
                ratios["dx by row"] = by_row
            for i, name in enumerate(("dgamma", "dbeta", "dxsum")[:n_out]):
                ratios[name] = _err(outs[i], want[1 + i]) / _tol(want[1 + i], GRAD_TOL)
            print(f"ln bwd D={d} M={m} {entry}: undecided {c.undecided:.2e}; err / tolerance " +
                  " ".join(f"{k} {v:.4f}" for k, v in ratios.items()) + ("" if d >= 32 else f" (dx by row {by_row:.4f})"))
            for name, r in ratios.items():
                assert r <= 1.0, (entry, m, name, r)
            worst[entry] = max(worst[entry], max(ratios.values()))
            if entry != "plain":
                assert float(outs[0][R.COL_OFF]) == 0.0 and float(outs[1][R.COL_OFF]) == 0.0, (entry, m)
                assert m < 1000 or (float(outs[0][R.COL_ON]) != 0.0 and float(outs[1][R.COL_ON]) != 0.0)
        # drop_p = 0 through the drop entry: the relu entry, bit for bit
        dxb0, outs0 = _ln_launch("drop", m, d, xb, dyb, gamma, beta, ws, drop_p=0.0)
        assert torch.equal(dxb0, got["relu"][0]) and torch.equal(outs0, got["relu"][1]), m
        if m > 1000:
            assert not torch.equal(got["drop"][0], got["relu"][0])
    print(f"ln bwd D={d}: worst err / tolerance " + " ".join(f"{k} {v:.4f}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------ (B) C = A^T B, exact
def _tn_launch(colsum, m, n, k, ab, bb, ws):
    """lpf_gemm_tn_f32 / _colsum_f32 on padded buffers -> (C buffer [n, k + 5] over the sentinel, colsum [n] over NaN)."""
    lib, P = _lib.hip(), _lib.ptr
    cb = torch.full((max(n, 2), k + 5), SENTINEL, dtype=torch.float32, device=DEV)
    cs = torch.full((max(n, 1),), NAN, dtype=torch.float32, device=DEV)
    ws.fill_(NAN)
    if colsum:
        rc = lib.lpf_gemm_tn_colsum_f32(m, n, k, P(ab), n + 3, P(bb), k + 1, P(cb), k + 5, P(cs), P(ws), _stream())
    else:
        rc = lib.lpf_gemm_tn_f32(m, n, k, P(ab), n + 3, P(bb), k + 1, P(cb), k + 5, P(ws), _stream())
    _lib.check(rc, "lpf_gemm_tn_colsum_f32" if colsum else "lpf_gemm_tn_f32")
    torch.cuda.synchronize()
    return cb, cs


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("n,k", R.TN_SHAPES)
def test_gemm_tn_exact(n, k):
    """(B) C = A^T B and the column sums of A for integer-valued A, B in {-2 .. 2} (every partial sum below 2^24: exact in
    fp32 in any order) against the int64 product, bit for bit, at M = 0, 1, 9, 63, 65, 257 and 32837 with lda = N + 3,
    ldb = K + 1, ldc = K + 5 over NaN padding in A and B, a sentinel in C and a NaN workspace: both entries give the same
    C, the padding of C is untouched, M = 0 gives exact zeros, N = 0 or K = 0 returns OK and writes nothing.  A misplaced,
    dropped or doubled row or column changes an integer.

    Measured on an MI355X: no element differs in bits, in any of the 6 x 7 cases (err / tolerance 0)."""
    lib = _lib.hip()
    assert (R.tn_chunk_rows(32837), R.tn_chunks(32837), 32837 - 456 * 72) == (72, 457, 5)
    assert [R.tn_chunks(m) for m in R.TN_ROWS[:5]] == [1, 1, 1, 2, 5] and R.tn_chunk_rows(257) == 64
    assert R.tn_groups(n) == (4 if n <= 32 else 2 if n <= 64 else 1)
    differ = 0
    for m in (0,) + R.TN_ROWS:
        # the launch arithmetic restated in the reference is the library's: it sizes the workspace by it
        floats = int(lib.lpf_gemm_tn_workspace_floats(m, n, k))
        assert floats == R.tn_workspace_floats(m, n, k), (m, floats)
        a, b = R.tn_case(m, n, k)
        want, want_cs = R.tn_exact(a, b)
        assert int(want.abs().max() if m else 0) < 2 ** 24
        want, want_cs = want.float().to(DEV), want_cs.float().to(DEV)
        ab, bb = _padded(a.to(DEV), 3, NAN), _padded(b.to(DEV), 1, NAN)
        ws = torch.empty(max(floats, 1), dtype=torch.float32, device=DEV)
        c0, cs0 = _tn_launch(False, m, n, k, ab, bb, ws)
        c1, cs1 = _tn_launch(True, m, n, k, ab, bb, ws)
        c2, cs2 = _tn_launch(True, m, n, k, ab, bb, ws)
        bad = int((_bits(c0[:n, :k]) != _bits(want)).sum()) + int((_bits(c1[:n, :k]) != _bits(want)).sum()) + \
            int((_bits(cs1[:n]) != _bits(want_cs)).sum())
        differ += bad
        print(f"gemm tn N={n} K={k} M={m}: chunks {R.tn_chunks(m) if m else 0} x {R.tn_groups(n)} groups, "
              f"{bad} of {2 * n * k + n} elements differ in bits (err / tolerance {float(bad > 0):.1f})")
        assert bad == 0, (m, torch.nonzero(c1[:n, :k] != want)[:5].tolist())
        assert torch.equal(_bits(c0), _bits(c1)) and torch.equal(_bits(c1), _bits(c2)) and torch.equal(_bits(cs1), _bits(cs2))
        assert bool((c0[:, k:] == SENTINEL).all()) and bool((c0[n:] == SENTINEL).all())
        assert bool(torch.isnan(cs0).all())                              # the plain entry has no column sums to write
        if m == 0:
            assert int(torch.count_nonzero(c1[:n, :k])) == 0 and int(torch.count_nonzero(cs1[:n])) == 0
    # nothing to compute: OK, and nothing written
    a, b = R.tn_case(9, n, k)
    ws = torch.empty(64, dtype=torch.float32, device=DEV)
    for nn, kk in ((0, k), (n, 0)):
        ab, bb = _padded(a[:, :nn].to(DEV), 3, NAN), _padded(b[:, :kk].to(DEV), 1, NAN)
        for colsum in (False, True):
            cb, cs = _tn_launch(colsum, 9, nn, kk, ab, bb, ws)
            assert bool((cb == SENTINEL).all()) and bool(torch.isnan(cs).all()) and bool(torch.isnan(ws).all())
    assert differ == 0


# ------------------------------------------------------------------------------------------------ (C) operators
_graph_cache = {}


def _gcn_graph():
    """The graph of (C) on the device, made once: (a, dense fp64 A)."""
    if not _graph_cache:
        n = R.GCN_NODES
        r, c, v = R.gcn_graph()
        a = graph.csr_from_coo(r, c, v, n).to_device(DEV)
        at = train._transpose_csr(a)
        deg, deg_t = a.rowptr[1:] - a.rowptr[:-1], at.rowptr[1:] - at.rowptr[:-1]
        long_row = _lib.CONST["LPF_SPMM_LONG_ROW"]
        assert long_row == R.LONG_ROW == 128
        assert int(deg.max()) > long_row and int(deg_t.max()) > long_row and int(deg.min()) == 0 and int(deg_t.min()) == 0
        dense = torch.zeros(n, n, dtype=torch.float64, device=DEV)
        rows = torch.repeat_interleave(torch.arange(n, device=DEV), deg)
        dense.index_put_((rows, a.col.long()), a.val.double(), accumulate=True)
        assert int(torch.count_nonzero(dense)) == r.size and not torch.equal(dense, dense.t())
        _graph_cache["g"] = (a, dense)
    return _graph_cache["g"]


def _leaves(*ts, dtype=torch.float32):
    return [t.to(DEV, dtype).requires_grad_() for t in ts]


def _compare(tag, out, ref, names, got, want, extra=""):
    ratios = {"out": _err(out, ref) / _tol(ref, FWD_TOL)}
    for name, g, w in zip(names, got, want):
        assert g.shape == w.shape, name
        ratios[name] = _err(g, w) / _tol(w, GRAD_TOL)
    w_name = max(ratios, key=ratios.get)
    print(f"{tag}: {extra}worst err / tolerance {ratios[w_name]:.4f} ({w_name}); " +
          " ".join(f"{k} {v:.4f}" for k, v in ratios.items()))
    for name, r in ratios.items():
        assert r <= 1.0, (tag, name, r)


def _zero_undecided(up, u64, g, be):
    """``up`` with zeros where the ReLU's side is undecided (from the fp64 u alone) -> (up, share)."""
    near = R.relu_ln_undecided(u64, g.to(DEV), be.to(DEV))
    share = float(near.double().mean())
    assert share <= R.UNDECIDED_CAP, share
    return torch.where(near, torch.zeros_like(up), up), share


@pytest.mark.parametrize("dim", [256, 36])
def test_gcn_layer_fn(dim):
    """(C) ``train.GcnLayerFn`` behind ``train.linear`` -- the first layer of every model and every D = 256 layer:
    r = ReLU(LN(A (x W^T) + b)), x [4603, 40], on a directed weighted graph with hub rows and empty rows both ways.
    Output and dx, dW, dconv_bias, dgamma, dbeta against fp64 autograd on a dense fp64 A; two runs bitwise equal.
    At D = 256 the LayerNorm backward takes a second trip with 507 rows (4603 = 4096 + 507), at D = 36 nine of a row's
    sixteen lanes are live.

    Measured on an MI355X, err / tolerance (out | dx | dW | dconv_bias | dgamma | dbeta), 0.43 % / 0.40 % undecided:
        D = 256   0.0138  0.0041  0.0026  0.0022  0.0019  0.0014
        D = 36    0.0154  0.0023  0.0022  0.0015  0.0013  0.0011"""
    n = R.GCN_NODES
    assert (n - R.ln_trip_rows(dim) == 507) if dim == 256 else (n < R.ln_trip_rows(dim) and R.ln_lanes(dim) * 4 > dim)
    a, dense = _gcn_graph()
    p = R.layer_params(n, R.GCN_IN, dim, 300 + dim)
    xs = _leaves(p.x, p.w, p.b, p.g, p.be, dtype=torch.float64)
    u64 = dense @ (xs[0] @ xs[1].t()) + xs[2]
    ref = torch.relu(torch.nn.functional.layer_norm(u64, (dim,), xs[3], xs[4]))
    up, share = _zero_undecided(p.up.to(DEV), u64.detach(), p.g, p.be)
    (ref * up.double()).sum().backward()

    def run():
        x, w, b, g, be = _leaves(p.x, p.w, p.b, p.g, p.be)
        out = train.GcnLayerFn.apply(train.linear(x, w), a, b, g, be)
        (out * up).sum().backward()
        return out.detach(), [t.grad for t in (x, w, b, g, be)]
    out, got = run()
    out2, got2 = run()
    assert torch.equal(out, out2) and all(torch.equal(g, g2) for g, g2 in zip(got, got2))
    _compare(f"GcnLayerFn D={dim}", out, ref.detach(), ("dx", "dW", "dconv_bias", "dgamma", "dbeta"), got,
             [t.grad for t in xs], extra=f"undecided {share:.2e}; ")
    empty = (a.rowptr[1:] == a.rowptr[:-1])
    assert int(empty.sum()) > 0 and int(torch.count_nonzero(got[0])) > 0


def test_spmm_fn():
    """(C) ``train.SpmmFn`` at D = 36: out = A t + bias and dt = A^T dout against a dense fp64 A (hub rows and empty rows
    in both directions); the rows of dt that no entry of A names are exactly 0.

    Measured on an MI355X, err / tolerance: out 0.0079, dt 0.0018, dbias 0.0014."""
    n, dim = R.GCN_NODES, 36
    a, dense = _gcn_graph()
    g = torch.Generator().manual_seed(36)
    t_cpu, bias_cpu, up = torch.randn(n, dim, generator=g), 0.1 * torch.randn(dim, generator=g), torch.randn(n, dim, generator=g).to(DEV)
    t64, bias64 = _leaves(t_cpu, bias_cpu, dtype=torch.float64)
    ref = dense @ t64 + bias64
    (ref * up.double()).sum().backward()

    def run():
        t, bias = _leaves(t_cpu, bias_cpu)
        out = train.SpmmFn.apply(t, a) + bias
        (out * up).sum().backward()
        return out.detach(), [t.grad, bias.grad]
    out, got = run()
    out2, got2 = run()
    assert torch.equal(out, out2) and torch.equal(got[0], got2[0])
    _compare("SpmmFn D=36", out, ref.detach(), ("dt", "dbias"), got, [t64.grad, bias64.grad])
    unnamed = dense.abs().sum(0) == 0
    assert int(unnamed.sum()) > 0 and int(torch.count_nonzero(got[0][unnamed])) == 0


@pytest.mark.parametrize("m", [1, R.GCN_NODES])
def test_ln_relu_fn(m):
    """(C) ``train.LnReluFn`` behind ``train.linear`` with a bias -- every MLP hidden layer -- at D = 256, one row and
    4603 rows (the backward's second trip): output and dx, dW, db, dgamma, dbeta against fp64 autograd; bitwise
    repeatable.

    Measured on an MI355X, err / tolerance (out | dx | dW | db | dgamma | dbeta; 0 and 0.09 % undecided):
        M = 1      0.0085  0.0058  0.0009  0.0007  0.0016  0.0000
        M = 4603   0.0154  0.0058  0.0020  0.0016  0.0018  0.0023"""
    dim = 256
    p = R.layer_params(m, R.GCN_IN, dim, 500 + m)
    xs = _leaves(p.x, p.w, p.b, p.g, p.be, dtype=torch.float64)
    u64 = xs[0] @ xs[1].t() + xs[2]
    ref = torch.relu(torch.nn.functional.layer_norm(u64, (dim,), xs[3], xs[4]))
    up, share = _zero_undecided(p.up.to(DEV), u64.detach(), p.g, p.be)
    (ref * up.double()).sum().backward()

    def run():
        x, w, b, g, be = _leaves(p.x, p.w, p.b, p.g, p.be)
        out = train.LnReluFn.apply(train.linear(x, w, b), g, be)
        (out * up).sum().backward()
        return out.detach(), [t.grad for t in (x, w, b, g, be)]
    out, got = run()
    out2, got2 = run()
    assert torch.equal(out, out2) and all(torch.equal(g, g2) for g, g2 in zip(got, got2))
    _compare(f"LnReluFn M={m}", out, ref.detach(), ("dx", "dW", "db", "dgamma", "dbeta"), got, [t.grad for t in xs],
             extra=f"undecided {share:.2e}; ")
