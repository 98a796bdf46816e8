"""The encoder's forward kernels -- csrc/spmm_csr.hip, csrc/gcn_fused.hip and the forward part of csrc/rowwise.hip --
straight through the C ABI against the fp64 restatements of tests/node_forward_reference.py, at the shapes where their
launch arithmetic changes, on graphs whose row lengths are planted at those edges.

House rules (those of tests/test_gpu_node_train_kernels.py): inputs and outputs sit in padded buffers whose padding
columns hold NaN, the D output columns are preset to a sentinel, nothing may be written outside them, every launch is
made twice and compared bitwise, every test prints its worst err / tolerance per row class.  The tolerance is the
project's forward one, 2e-5 max(1, max|ref|), taken over the whole tensor AND over every row class with the class's own
max|ref| (``node_forward_reference.compare``): the hub rows set the whole-tensor bound and would let every short row
off.  tests/test_node_forward_reference_host.py shows that this comparison rejects eleven planted faults.

Reach map -- entry point: test: the edge it crosses.
  lpf_gcn_norm_csr          test_gcn_norm (A): n = 1 (one wavefront of a workgroup of four live) and 4099 (n % 4 = 3);
                              rows of 0 (dis = 0, and every entry that names such a row), 1 (the diagonal alone), 63, 64,
                              65 (a lane's second entry) and 700 entries; stored diagonals of weight 3 (counted as 1), rows
                              without one; weighted and w_in = NULL.
  lpf_spmm_csr_f32          test_spmm_f32 (B), once per width: 4 (one live lane of 16), 24 (three of 8, two float4 each),
                              36 (9 of 16, one float4), 64, 96, 128, 132 (33 of 64, one row per wavefront), 256.  Row
                              lengths 0, 1, 3, 4, 5 (the four gathers of a step), G - 1, G, G + 1, 2 G + 3 (chunks), 127,
                              128, 129 (SPMM_LONG: the first row the main kernel skips), 255, 256, 257, 775 (the hub
                              kernel's rounds of NG x G = 256 entries), each planted.  ldh = D + 4, ldo = D + 8, ldr = D +
                              12.  Hub rows through the main kernel (long_rows = NULL), through the hub kernel
                              (Structure.long_rows) and in a row block [37, n - 29) through ops.spmm.
                            test_spmm_second_trip: D = 132, n = 32768 + 5 and D = 128, n = 131072 + 7.
                            test_spmm_unsupported_widths: D = 260, 6 (and 4 for the bf16 table).
  lpf_spmm_csr_bf16         test_spmm_bf16 (C): 8 (one live lane of 8), 64, 136 (17 of 32), 256; the same graph and forms;
                              ldh = D + 8 (bf16 rows are 16-byte aligned: D + 4 is not a legal ldh here).
  lpf_spmm_row_parts_f32    test_row_parts (D): D = 8, 24, 64 (G = 8, NG = 32), 128 (G = 16, NG = 16); slices of 1, G - 1,
  lpf_spmm_row_parts_bf16p    G + 1, 255, 256 = G NG entries starting anywhere; ldh = D + 8; one slice and 70,000; the
                              permuted bf16 table at D = 64, 128 with the sums in normal order; D = 136 / 32 unsupported.
  lpf_gcn_layer_fused_f32   test_fused_layer (E): D = 32, 64 (NBP = 2), 128 (NBP = 4); row lengths 0, 1, NBP - 1, NBP,
  lpf_gcn_layer_fused_bf16    NBP + 1, 2 NBP + 1, 63, 64, 65 (a hub of one slice of 65), 256, 257 (256 + 1), 700; five hubs:
                              in fused_row_order's own order the last hub shares a lane pair with a row of 64 entries, in
                              the rising order with an empty row; a shuffle with -1 codes inside; the bf16 table with hubs
                              and -1 alone in the hub tiles; whole graph and the row block [21, n - 14) with row_base = 21;
                              ldh = D + 8, ldo = D + 4, ldr = D + 8, ldpre = D + 12, ldob = D + 8; pre_out; out_bf16p.
                            test_fused_tile_counts: n_tiles = 1, 8, 9 (one wavefront of a second workgroup) and the first
                              round (8 wavefronts x 1 or 2 workgroups per CU x CUs, from lpf_device_info) + 11: the ticket.
  lpf_layernorm_f32         test_layernorm_forward (F): D = 1, 3, 63, 64, 65 (a lane's second element), 1000, 1024 (16 per
                              lane), 1025 unsupported; with and without affine and ReLU; near-constant rows (rstd 287);
                              the drawn rows of D = 3 by the bound fp32 can meet (see the test).
  lpf_pair_gather_f32       test_pair_gather: D = 4, 36, 64 (G = 16), 132, 256 (G = 64); ids -1, n_rows, 2^40 read row 0;
                              mul only, sum only, both; batch_ld = M + 3.
  lpf_rowdot_sigmoid_f32    test_rowdot_sigmoid: K = 1, 63, 64, 65, 130; logits 100.3 / -99.7 give exactly 1 and 0.
                              Each of the three at M = 1, 5 and 32768 + 5 (the gather also at its own trip + 5), padded ld.

One contract is pinned on the way (test_spmm_*, test_row_parts, test_fused_layer): lanes past the end of a row gather
(row 0, weight 0).  The planted columns never name row 0, and with H[0] (and row 0 of the slice sums) at 1e30 every
output is bitwise what it is with 0 there.  DESIGN.md (the encoder) states the precondition this implies.

Measured on an MI355X: see the docstring of each test; the worst err / tolerance per entry point is 0.107 for
lpf_gcn_norm_csr, 0.123 for lpf_spmm_csr_f32, 0.049 for _bf16, 0.015 for the slice sums, 0.031 / 0.026 for the one-launch
layer from an fp32 / bf16 table, 0.105 for lpf_layernorm_f32 (D >= 63), 0.003 for the gather, 0.035 for dot + sigmoid.
No kernel had to change.  No number in this file was known before it was written."""
import types

import pytest
import torch

from lpformer_amd import _lib, fold, graph, ops
from tests import node_forward_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SENT = R.SENTINEL
UNSUPPORTED = _lib.CONST["LPF_ERR_UNSUPPORTED"]
P = _lib.ptr


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _padded(t, pad, dtype=torch.float32):
    """``t`` [rows, D] in a [rows, D + pad] buffer whose padding columns hold NaN."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), NAN, dtype=dtype, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf


def _out_buf(rows, d, pad, dtype=torch.float32):
    """An output buffer: the D columns hold the sentinel, the padding NaN."""
    buf = torch.full((rows, d + pad), NAN, dtype=dtype, device=DEV)
    buf[:, :d] = SENT
    return buf


def _written(buf, d, tag):
    """Every element of the D columns written, nothing in the padding touched -> the [rows, D] view."""
    assert bool(torch.isnan(buf[:, d:]).all()), f"{tag}: written past the D columns"
    assert not bool((buf[:, :d] == SENT).any()), f"{tag}: a row was left at the sentinel"
    return buf[:, :d]


def _dev(c):
    return types.SimpleNamespace(**{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in vars(c).items()})


def _classes(c, lo=0, hi=None):
    return {k: m[lo:hi].to(DEV) for k, m in c.classes.items()}


def _report(tag, ratios, worst_of):
    print(f"{tag}: err / tolerance {R.show(ratios)}")
    for name, r in ratios.items():
        assert r <= 1.0, (tag, name, r)
    worst_of.append(max(ratios.values()))


def _ep_ptrs(g, ep, res):
    """The epilogue arguments of the spmm / fused entry points from bias on: (bias, ln_g, ln_b, residual, ldr, ln2_g,
    ln2_b, flags)."""
    ln, relu, use_res, ln2 = ep
    return (P(g.bias), P(g.g1) if ln else None, P(g.b1) if ln else None, P(res) if use_res else None,
            res.stride(0) if use_res else 0, P(g.g2) if ln2 else None, P(g.b2) if ln2 else None, 1 if relu else 0)


def _ep_ref(g, ep, agg_or_pre, res, w=None):
    ln, relu, use_res, ln2 = ep
    kw = dict(bias=g.bias, ln=(g.g1, g.b1) if ln else None, relu=relu, residual=res if use_res else None,
              ln2=(g.g2, g.b2) if ln2 else None)
    return R.epilogue64(agg_or_pre, **kw) if w is None else R.fused_layer64(agg_or_pre, w, **kw)


# ------------------------------------------------------------------------------------------------ (A) GCN normalisation
@pytest.mark.parametrize("n", [1, 4099])
def test_gcn_norm(n):
    """(A) w_out against ``gcn_norm64`` at the suite's rtol 2e-6 / atol 1e-7 (test_spmm_fused_epilogue), dis of the empty
    rows exactly 0, of the others within rtol 2e-6; weighted and with w_in = NULL; two runs bitwise equal.

    Measured on an MI355X, worst |err| / (atol + rtol |want|): n = 1: 0 (w_out = dis = 1 exactly); n = 4099: w_out 0.107,
    dis 0.057 weighted, 0.027 and 0.016 with w_in = NULL."""
    c = _dev(R.norm_case(n))
    lib = _lib.hip()
    nnz = c.col.numel()
    empty = torch.from_numpy(c.lengths == 0).to(DEV)
    for w_in in (c.val, None):
        def run():
            w_out = torch.full((nnz + 1,), SENT, dtype=torch.float32, device=DEV)
            dis = torch.full((n + 1,), SENT, dtype=torch.float32, device=DEV)
            _lib.check(lib.lpf_gcn_norm_csr(n, P(c.rowptr), P(c.col), P(w_in), P(w_out), P(dis), _stream()), "lpf_gcn_norm_csr")
            torch.cuda.synchronize()
            return w_out, dis
        (w_out, dis), (w2, dis2) = run(), run()
        assert torch.equal(w_out, w2) and torch.equal(dis, dis2)
        assert float(w_out[nnz]) == SENT and float(dis[n]) == SENT           # nothing behind the arrays
        want_w, want_dis = R.gcn_norm64(c.rowptr, c.col, w_in)
        assert bool((dis[:n][empty] == 0).all()) and bool(torch.isfinite(w_out).all())
        r_w = float(((w_out[:nnz].double() - want_w).abs() / (1e-7 + 2e-6 * want_w.abs())).max())
        r_d = float(((dis[:n].double() - want_dis).abs() / (1e-7 + 2e-6 * want_dis.abs())).max())
        print(f"gcn_norm n={n} {'weighted' if w_in is not None else 'w_in=NULL'}: err / tolerance w_out {r_w:.4f} dis {r_d:.4f}")
        assert r_w <= 1.0 and r_d <= 1.0
        if n > 1:
            assert int(empty.sum()) > 0 and bool((w_out[:nnz][empty[c.col.long()]] == 0).all())
        else:
            assert w_out[:1].tolist() == [1.0] and dis[:1].tolist() == [1.0]


# ------------------------------------------------------------------------------------------------ (B), (C) SpMM
def _table(h, pad, bf16, row0=None):
    """The gathered table in its padded buffer (``row0``: a value for the whole of row 0)."""
    buf = _padded(h, pad, torch.bfloat16 if bf16 else torch.float32)
    if row0 is not None:
        buf[0, :h.shape[1]] = row0
    return buf


def _spmm_direct(name, g, n, d, hb, ep, resb, long_rows, tag):
    lib = _lib.hip()
    ob = _out_buf(n, d, 8)
    rc = getattr(lib, name)(n, d, P(g.rowptr), P(g.col), P(g.val), P(hb), hb.stride(0), P(ob), ob.stride(0),
                            *_ep_ptrs(g, ep, resb), P(long_rows), 0 if long_rows is None else long_rows.numel(), _stream())
    _lib.check(rc, name)
    torch.cuda.synchronize()
    return _written(ob, d, tag)


def _spmm_forms(d, bf16):
    c = R.spmm_case(d, bf16)
    g = _dev(c)
    name = "lpf_spmm_csr_bf16" if bf16 else "lpf_spmm_csr_f32"
    pad_h = 8 if bf16 else 4
    hb, resb = _table(c.h, pad_h, bf16), _padded(c.res, 12)
    hb_zero, hb_huge = _table(c.h, pad_h, bf16, 0.0), _table(c.h, pad_h, bf16, 1e30)
    assert hb.stride(0) == d + pad_h and resb.stride(0) == d + 12
    long_rows = graph.Structure(g.rowptr, g.col, c.n).long_rows()
    assert long_rows.dtype == torch.int32 and long_rows.numel() == int((c.lengths > R.LONG_ROW).sum()) >= 5
    agg = R.spmm64(g.rowptr, g.col, g.val, g.h)
    a = graph.DeviceCSR(g.rowptr, g.col, g.val, c.n)
    worst = []
    for ep in R.EPILOGUES:
        ref = _ep_ref(g, ep, agg, g.res)
        outs = {}
        for form, lr in (("main", None), ("hubs", long_rows)):
            tag = f"{name} D={d} ep={ep} {form}"
            out = _spmm_direct(name, g, c.n, d, hb, ep, resb, lr, tag)
            assert torch.equal(out, _spmm_direct(name, g, c.n, d, hb, ep, resb, lr, tag)), tag
            _report(tag, R.compare(out, ref, _classes(c)), worst)
            # rows past their end gather (row 0, weight 0): whatever row 0 holds, no output bit changes
            for other in (hb_zero, hb_huge):
                assert torch.equal(out, _spmm_direct(name, g, c.n, d, other, ep, resb, lr, tag)), f"{tag}: H[0] reached a row"
            outs[form] = out
        ln = types.SimpleNamespace(weight=g.g1, bias=g.b1) if ep[0] else None
        fin = types.SimpleNamespace(weight=g.g2, bias=g.b2) if ep[3] else None
        blk = ops.spmm(a, hb[:, :d], c.lo, c.hi, bias=g.bias, ln=ln, res=resb[c.lo:c.hi, :d] if ep[2] else None,
                       final_ln=fin, relu=ep[1])
        torch.cuda.synchronize()
        tag = f"{name} D={d} ep={ep} block [{c.lo}, {c.hi})"
        _report(tag, R.compare(blk, ref[c.lo:c.hi], _classes(c, c.lo, c.hi)), worst)
        assert torch.equal(blk, outs["hubs"][c.lo:c.hi]), f"{tag}: a row's result depends on the block it is launched in"
    print(f"{name} D={d}: worst err / tolerance {max(worst):.4f}")


@pytest.mark.parametrize("d", R.SPMM_F32_WIDTHS)
def test_spmm_f32(d):
    """(B) Every epilogue x {hub rows in the main kernel, in the hub kernel, a row block through ops.spmm}.

    Measured on an MI355X, worst err / tolerance over epilogues, forms and classes:
        D    4      24     36     64     96     128    132    256
             0.123  0.050  0.021  0.056  0.034  0.038  0.048  0.041"""
    _spmm_forms(d, False)


@pytest.mark.parametrize("d", R.SPMM_BF16_WIDTHS)
def test_spmm_bf16(d):
    """(C) The same from a bf16 table: the RNE image of an fp32 table, whose rounded values the fp64 reference uses.

    Measured on an MI355X, worst err / tolerance over epilogues, forms and classes:
        D    8      64     136    256
             0.023  0.049  0.027  0.049"""
    _spmm_forms(d, True)


@pytest.mark.parametrize("d,above", R.SPMM_TRIP_CASES)
def test_spmm_second_trip(d, above):
    """(B) One trip of the capped grid (8192 workgroups x 4 wavefronts x rows per wavefront) and a few rows more.

    Measured on an MI355X, worst err / tolerance: D = 132: 0.012 (rows of three entries; the second trip 0.005);
    D = 128: 0.009 (second trip 0.005)."""
    c = R.spmm_trip_case(d, above)
    assert c.n == R.BLOCK_CAP * 4 * R.spmm_shape(d)[2] + above
    g = _dev(c)
    hb, resb = _table(c.h, 4, False), _padded(c.res, 12)
    ep = R.EPILOGUES[0]
    tag = f"lpf_spmm_csr_f32 D={d} n={c.n}"
    out = _spmm_direct("lpf_spmm_csr_f32", g, c.n, d, hb, ep, resb, None, tag)
    assert torch.equal(out, _spmm_direct("lpf_spmm_csr_f32", g, c.n, d, hb, ep, resb, None, tag))
    assert torch.equal(out, _spmm_direct("lpf_spmm_csr_f32", g, c.n, d, _table(c.h, 4, False, 1e30), ep, resb, None, tag))
    ref = _ep_ref(g, ep, R.spmm64(g.rowptr, g.col, g.val, g.h), g.res)
    _report(tag, R.compare(out, ref, _classes(c)), [])


def test_spmm_unsupported_widths():
    """D = 260 and 6 (fp32 table), 260 and 4 (bf16 table: D % 8) return LPF_ERR_UNSUPPORTED and write nothing."""
    c = R.spmm_case(4)
    g = _dev(c)
    lib = _lib.hip()
    for name, d, dtype in (("lpf_spmm_csr_f32", 260, torch.float32), ("lpf_spmm_csr_f32", 6, torch.float32),
                           ("lpf_spmm_csr_bf16", 260, torch.bfloat16), ("lpf_spmm_csr_bf16", 4, torch.bfloat16)):
        hb = torch.ones(c.n_cols, 264, dtype=dtype, device=DEV)
        ob = torch.full((c.n, 264), SENT, device=DEV)
        rc = getattr(lib, name)(c.n, d, P(g.rowptr), P(g.col), P(g.val), P(hb), 264, P(ob), 264, None, None, None, None, 0,
                                None, None, 0, None, 0, _stream())
        torch.cuda.synchronize()
        assert rc == UNSUPPORTED and bool((ob == SENT).all()), (name, d, rc)


# ------------------------------------------------------------------------------------------------ (D) slices of hub rows
def _parts_launch(d, bf16p, parts, col, val, hb, n_rows_out):
    lib = _lib.hip()
    out = torch.full((n_rows_out + 1, d), SENT, dtype=torch.float32, device=DEV)
    name = "lpf_spmm_row_parts_bf16p" if bf16p else "lpf_spmm_row_parts_f32"
    _lib.check(getattr(lib, name)(d, P(parts), parts.shape[0], P(col), P(val), P(hb), hb.stride(0), P(out), _stream()), name)
    torch.cuda.synchronize()
    assert bool((out[n_rows_out] == SENT).all()), f"{name}: written behind the last slice"
    assert not bool((out[:n_rows_out] == SENT).any()), f"{name}: a slice was left at the sentinel"
    return out[:n_rows_out]


@pytest.mark.parametrize("d,bf16p", [(d, False) for d in R.PARTS_F32_WIDTHS] + [(d, True) for d in R.PARTS_BF16_WIDTHS])
def test_row_parts(d, bf16p):
    """(D) One slice and 70,000 slices against ``row_parts64``, classes by slice length; the bf16 table is the permuted
    image and the sums come out in normal order; H[0] reaches no sum; D = 136 (fp32) / 32 (bf16) are unsupported.

    Measured on an MI355X, worst err / tolerance: fp32 table D = 8: 0.015, 24: 0.013, 64: 0.013, 128: 0.012; permuted bf16
    table D = 64: 0.014, 128: 0.011."""
    worst = []
    for n_parts in (1, R.PARTS_MANY):
        c = R.parts_case(d, n_parts, bf16p)
        g = _dev(c)
        image = R.permute_bf16p(c.h) if bf16p else c.h
        hb = _table(image, 8, bf16p)
        if bf16p:
            assert torch.equal(R.unpermute_bf16p(hb[:, :d].float()), g.h)      # the image holds the reference's values
        out = _parts_launch(d, bf16p, g.parts, g.col, g.val, hb, n_parts)
        assert torch.equal(out, _parts_launch(d, bf16p, g.parts, g.col, g.val, hb, n_parts))
        for row0 in (0.0, 1e30):
            assert torch.equal(out, _parts_launch(d, bf16p, g.parts, g.col, g.val, _table(image, 8, bf16p, row0), n_parts))
        ref = R.row_parts64(g.parts, g.col, g.val, g.h)
        _report(f"row_parts{'_bf16p' if bf16p else '_f32'} D={d} slices={n_parts}", R.compare(out, ref, _classes(c)), worst)
    lib = _lib.hip()
    out = torch.full((2, 136), SENT, device=DEV)
    hb = torch.ones(1025, 136, dtype=torch.bfloat16 if bf16p else torch.float32, device=DEV)
    bad = 32 if bf16p else 136
    fn = lib.lpf_spmm_row_parts_bf16p if bf16p else lib.lpf_spmm_row_parts_f32
    assert fn(bad, P(g.parts), 1, P(g.col), P(g.val), P(hb), 136, P(out), _stream()) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
    print(f"row_parts D={d} bf16p={bf16p}: worst err / tolerance {max(worst):.4f}")


# ------------------------------------------------------------------------------------------------ (E) the one-launch layer
def _fused_tables(c, g, d, bf16, row0=None):
    image = R.permute_bf16p(c.h) if bf16 else c.h
    return _table(image, 8, bf16, row0)


def _fused_run(g, d, bf16, hb, wp, order, hubs, parts, lo, hi, ep, resb, extra, tag, slice0=None):
    """Slice sums (the kernels of (D)), then the layer -> (out, pre_out or the bf16 image, t_parts)."""
    lib = _lib.hip()
    t_parts = None
    if hubs is not None:
        t_parts = _parts_launch(d, bf16, parts, g.col, g.val, hb, parts.shape[0])
        if slice0 is not None:
            t_parts[0] = slice0
    rows = hi - lo
    ob = _out_buf(rows, d, 4)
    common = (d, order.numel() // 16, P(order), lo, P(g.rowptr), P(g.col), P(g.val), P(hb), hb.stride(0), P(wp), P(ob),
              ob.stride(0), *_ep_ptrs(g, ep, resb), P(hubs), P(t_parts))
    second = None
    if bf16:
        if extra:
            second = torch.full((rows, d + 8), SENT, dtype=torch.bfloat16, device=DEV)
        rc = lib.lpf_gcn_layer_fused_bf16(*common, P(second), d + 8 if extra else 0, _stream())
    else:
        if extra:
            second = _out_buf(rows, d, 12)
        rc = lib.lpf_gcn_layer_fused_f32(*common, P(second), d + 12 if extra else 0, _stream())
    _lib.check(rc, tag)
    torch.cuda.synchronize()
    out = _written(ob, d, tag)
    if extra and bf16:
        assert bool((second[:, d:] == SENT).all()), f"{tag}: out_bf16p written past the D columns"
        second = second[:, :d]
    elif extra:
        second = _written(second, d, tag + " pre_out")
    return out, second, t_parts


def _bits16(t):
    return t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def _fused_layer(d, bf16):
    c = R.fused_case(d, bf16)
    g = _dev(c)
    name = "lpf_gcn_layer_fused_bf16" if bf16 else "lpf_gcn_layer_fused_f32"
    hb = _fused_tables(c, g, d, bf16)
    wp = torch.from_numpy(fold.pack_dense(c.w.numpy(), 1)).to(DEV)
    agg = R.spmm64(g.rowptr, g.col, g.val, g.h)
    worst = []
    for lo, hi in ((0, c.n), (c.lo, c.hi)):
        orders, hubs, parts = R.fused_orders(c.rowptr, lo, hi, bf16, 17 + d)
        hubs, parts = hubs.to(DEV), parts.to(DEV)
        resb = _padded(c.res[lo:hi], 8)
        cls = _classes(c, lo, hi)
        for ep in R.EPILOGUES:
            ref = _ep_ref(g, ep, agg[lo:hi], g.res[lo:hi], g.w)
            pre_ref = agg[lo:hi] @ g.w.double().t() + g.bias.double()
            first = None
            for kind, order in orders.items():
                order = order.to(DEV)
                tag = f"{name} D={d} rows [{lo}, {hi}) ep={ep} order={kind}"
                out, second, _ = _fused_run(g, d, bf16, hb, wp, order, hubs, parts, lo, hi, ep, resb, True, tag)
                out2, second2, _ = _fused_run(g, d, bf16, hb, wp, order, hubs, parts, lo, hi, ep, resb, True, tag)
                assert torch.equal(out, out2) and torch.equal(_bits16(second) if bf16 else second,
                                                              _bits16(second2) if bf16 else second2), tag
                ratios = R.compare(out, ref, cls)
                if bf16:    # the image for the next layer: the kernel's own fp32 rows, rounded to nearest even, permuted
                    assert torch.equal(_bits16(second), R.permute_bf16p(R.bf16_bits(out))), f"{tag}: out_bf16p"
                else:
                    ratios.update({f"pre {k}": v for k, v in R.compare(second, pre_ref, cls).items()})
                _report(tag, ratios, worst)
                plain, _, _ = _fused_run(g, d, bf16, hb, wp, order, hubs, parts, lo, hi, ep, resb, False, tag)
                assert torch.equal(plain, out), f"{tag}: the second output changes the first"
                # a row's result does not depend on the rows it shares a tile or a lane pair with
                first = out if first is None else first
                assert torch.equal(out, first), f"{tag}: a row's bits depend on the order"
        if (lo, hi) == (0, c.n):
            # lanes past the end of a row -- and of a hub's slice list -- gather (row 0, weight 0): with an empty slice 0
            # that no hub names, row 0 of the table and of the slice sums may hold anything
            h2, p2 = R.with_dummy_slice(hubs.cpu(), parts.cpu())
            h2, p2 = h2.to(DEV), p2.to(DEV)
            order = orders["own"].to(DEV)
            for ep in R.EPILOGUES[:2]:
                tag = f"{name} D={d} ep={ep} row 0"
                base, _, _ = _fused_run(g, d, bf16, hb, wp, order, hubs, parts, lo, hi, ep, resb, False, tag)
                zero, _, tp = _fused_run(g, d, bf16, _fused_tables(c, g, d, bf16, 0.0), wp, order, h2, p2, lo, hi, ep, resb,
                                         False, tag, slice0=0.0)
                huge, _, _ = _fused_run(g, d, bf16, _fused_tables(c, g, d, bf16, 1e30), wp, order, h2, p2, lo, hi, ep, resb,
                                        False, tag, slice0=1e30)
                assert tp.shape[0] == parts.shape[0] + 1
                assert torch.equal(zero, huge), f"{tag}: H[0] or t_parts[0] reached a row"
                assert torch.equal(zero, base), f"{tag}: the empty slice changed a row"
    print(f"{name} D={d}: worst err / tolerance {max(worst):.4f}")


@pytest.mark.parametrize("d", R.FUSED_F32_WIDTHS)
def test_fused_layer_f32(d):
    """(E) Whole graph and a row block x three orders x four epilogues, out and pre_out (product + bias) against
    ``fused_layer64``; the same bits in every order and with or without pre_out; row 0 of the tables reaches no row.

    Measured on an MI355X, worst err / tolerance over everything: D = 32: 0.015, 64: 0.031, 128: 0.024."""
    _fused_layer(d, False)


@pytest.mark.parametrize("d", R.FUSED_BF16_WIDTHS)
def test_fused_layer_bf16(d):
    """(E) The same from the permuted bf16 table (hub tiles: hubs and -1 only), slice sums from
    lpf_spmm_row_parts_bf16p; out_bf16p bitwise the permuted RNE image of the kernel's own fp32 rows.

    Measured on an MI355X, worst err / tolerance over everything: D = 64: 0.016, 128: 0.026."""
    _fused_layer(d, True)


@pytest.mark.parametrize("d,bf16", [(d, False) for d in R.FUSED_F32_WIDTHS] + [(d, True) for d in R.FUSED_BF16_WIDTHS])
def test_fused_tile_counts(d, bf16):
    """(E) n_tiles = 1, 8, 9 and the first round + 11 (tiles drawn from the LDS ticket), rows of 1 .. 3 entries, five -1
    codes in the last tile; the rows of the ticket round are a class of their own.

    Measured on an MI355X (256 CUs), worst err / tolerance: fp32 table D = 32: 0.010, 64: 0.017, 128: 0.020; bf16 table
    D = 64: 0.016, 128: 0.019."""
    cu = _lib.device_info()["cu_count"]
    cap = R.fused_cap_tiles(d, cu)
    worst = []
    for n_tiles in R.FUSED_SMALL_TILES + (cap + 11,):
        c = R.fused_tiles_case(d, n_tiles)
        if bf16:
            c.h = R.bf16_rne(c.h)
        g = _dev(c)
        order, hubs, _ = graph.fused_row_order(g.rowptr, 0, c.n, pad_hubs=bf16)
        assert hubs is None and order.numel() == 16 * n_tiles and n_tiles > (0 if n_tiles < cap else 8 * (cap // 8))
        ticket = torch.zeros(c.n, dtype=torch.bool, device=DEV)
        late = order[16 * cap:].long()
        ticket[late[late >= 0]] = True
        assert int(ticket.sum()) == (16 * 11 - 5 if n_tiles > cap else 0)
        hb = _fused_tables(c, g, d, bf16)
        wp = torch.from_numpy(fold.pack_dense(c.w.numpy(), 1)).to(DEV)
        resb = _padded(c.res, 8)
        ep = R.EPILOGUES[0]
        tag = f"fused{'_bf16' if bf16 else '_f32'} D={d} n_tiles={n_tiles}"
        out, _, _ = _fused_run(g, d, bf16, hb, wp, order, None, None, 0, c.n, ep, resb, False, tag)
        out2, _, _ = _fused_run(g, d, bf16, hb, wp, order, None, None, 0, c.n, ep, resb, False, tag)
        assert torch.equal(out, out2), tag
        ref = _ep_ref(g, ep, R.spmm64(g.rowptr, g.col, g.val, g.h), g.res, g.w)
        cls = _classes(c)
        cls["ticket round"] = ticket
        _report(tag, R.compare(out, ref, cls), worst)
    print(f"fused tile counts D={d} bf16={bf16}: worst err / tolerance {max(worst):.4f}")


def test_fused_unsupported_widths():
    c = R.fused_tiles_case(32, 1)
    g = _dev(c)
    order, _, _ = graph.fused_row_order(g.rowptr, 0, c.n)
    lib = _lib.hip()
    ob = torch.full((c.n, 160), SENT, device=DEV)
    hb = torch.ones(c.n_cols, 160, device=DEV)
    wp = torch.zeros(16 * 2048, device=DEV)
    for fn, d in ((lib.lpf_gcn_layer_fused_f32, 96), (lib.lpf_gcn_layer_fused_f32, 16), (lib.lpf_gcn_layer_fused_bf16, 32)):
        rc = fn(d, 1, P(order), 0, P(g.rowptr), P(g.col), P(g.val), P(hb), 160, P(wp), P(ob), 160, None, None, None, None, 0,
                None, None, 0, None, None, None, 0, _stream())
        torch.cuda.synchronize()
        assert rc == UNSUPPORTED and bool((ob == SENT).all()), (d, rc)


# ------------------------------------------------------------------------------------------------ (F) row-wise kernels
@pytest.mark.parametrize("d", R.LN_WIDTHS)
def test_layernorm_forward(d):
    """(F) lpf_layernorm_f32 at M = 1, 5 and one trip + 5, ldx = D + 3, ldy = D + 5, with and without affine (without:
    the rows unchanged, or their ReLU) and ReLU; classes: near-constant rows, the others, the second trip.

    Measured on an MI355X, worst err / tolerance:
        D    1      3        63     64     65     1000   1024
             0      (1.79)   0.105  0.082  0.091  0.081  0.059
    D = 3 misses 2e-5 on its drawn rows (1.79 at M = 32773; torch's own fp32 LayerNorm gives the same 1.79 on that case)
    for the reason ``node_forward_reference.ln_cond_ratio`` derives: three draws can lie within 1e-3 of each other around
    a mean of 5, and fp32 holds that mean to 2^-24 x 5 only.  Those rows are held to K 2^-24 max|x_i| rstd_i |gamma_j|
    with K = 16: measured 3.63, 3.74 and 3.76 over the case's seed, + 1000 and + 2000, x 4, rounded up to a power of
    two; asserted here for all three seeds.  The near-constant rows of D = 3 stay at 2e-5 (measured 0.0014)."""
    lib = _lib.hip()
    worst = []
    for m in (1, 5, R.rowwise_trip_rows() + 5):
        c = R.ln_case(d, m)
        g = _dev(c)
        xb = _padded(c.x, 3)
        for affine in (True, False):
            for relu in (False, True):
                def run():
                    yb = _out_buf(m, d, 5)
                    _lib.check(lib.lpf_layernorm_f32(m, d, P(xb), d + 3, P(g.gamma) if affine else None,
                                                     P(g.beta) if affine else None, P(yb), d + 5, 1 if relu else 0, _stream()),
                               "lpf_layernorm_f32")
                    torch.cuda.synchronize()
                    return yb
                yb, yb2 = run(), run()
                tag = f"layernorm D={d} M={m} affine={affine} relu={relu}"
                assert torch.equal(yb[:, :d], yb2[:, :d]) and bool(torch.isnan(yb[:, d:]).all()), tag
                ref = R.layernorm64(g.x, g.gamma if affine else None, g.beta if affine else None, relu)
                if affine:
                    assert not bool((yb[:, :d] == SENT).any()), tag
                else:
                    assert torch.equal(yb[:, :d].double(), ref), tag          # nothing to round
                ratios = R.compare(yb[:, :d], ref, _classes(c))
                if affine and d in R.LN_COND_WIDTHS:
                    # the drawn rows of this width: the bound fp32 can meet (``ln_cond_ratio``), not 2e-5; the
                    # near-constant rows, whose mean is exact, stay at 2e-5
                    print(f"{tag}: at 2e-5 it would be {R.show(ratios)}")
                    cond = R.ln_cond_ratio(yb[:, :d], ref, g.x, g.gamma) / R.LN_COND_K
                    ratios.update({k: float(cond[m_].max()) if bool(m_.any()) else 0.0 for k, m_ in _classes(c).items()
                                   if k != "near-constant rows"})
                    ratios["all"] = max(float(cond[~g.const].max()) if bool((~g.const).any()) else 0.0,
                                        ratios["near-constant rows"])
                _report(tag, ratios, worst)
    if d in R.LN_COND_WIDTHS:      # the constant of the bound: 4 x the worst of three seeds, rounded up to a power of two
        m, measured = R.rowwise_trip_rows() + 5, []
        for seed in (0, 1000, 2000):
            g = _dev(R.ln_case(d, m, seed))
            xb, yb = _padded(g.x, 3), _out_buf(m, d, 5)
            _lib.check(lib.lpf_layernorm_f32(m, d, P(xb), d + 3, P(g.gamma), P(g.beta), P(yb), d + 5, 0, _stream()), "ln")
            torch.cuda.synchronize()
            ref = R.layernorm64(g.x, g.gamma, g.beta)
            measured.append(float(R.ln_cond_ratio(yb[:, :d], ref, g.x, g.gamma)[~g.const].max()))
        print(f"layernorm D={d}: |err| / (2^-24 max|x_i| rstd_i |gamma_j|) over three seeds {measured}, K = {R.LN_COND_K}")
        assert 4 * max(measured) <= R.LN_COND_K
    yb = _out_buf(2, 1025, 3)
    xb = torch.ones(2, 1028, device=DEV)
    assert lib.lpf_layernorm_f32(2, 1025, P(xb), 1028, None, None, P(yb), 1028, 0, _stream()) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((yb[:, :1025] == SENT).all())
    print(f"layernorm D={d}: worst err / tolerance {max(worst):.4f}")


@pytest.mark.parametrize("d", R.GATHER_WIDTHS)
def test_pair_gather(d):
    """(F) lpf_pair_gather_f32 at M = 1, 5, 32768 + 5 and its own trip + 5; ids -1, n_rows and 2^40 read row 0; mul only,
    sum only and both; ldx = D + 12, ldm = D + 4, lds = D + 8, batch_ld = M + 3.

    Measured on an MI355X, worst err / tolerance: D = 4: 0.0023, 36: 0.0017, 64: 0.0028, 132: 0.0026, 256: 0.0025."""
    lib = _lib.hip()
    worst = []
    for m in sorted({1, 5, R.rowwise_trip_rows() + 5, R.gather_trip_rows(d) + 5}):
        c = R.gather_case(d, m)
        g = _dev(c)
        xb = _padded(c.x, 12)
        bb = torch.full((2, m + 3), 2 ** 62, dtype=torch.int64, device=DEV)
        bb[:, :m] = g.batch
        ref_mul, ref_sum = R.pair_gather64(g.x, g.batch, R.GATHER_ROWS)
        got = {}
        for want_mul, want_sum in ((True, False), (False, True), (True, True)):
            def run():
                mb, sb = _out_buf(m, d, 4), _out_buf(m, d, 8)
                _lib.check(lib.lpf_pair_gather_f32(m, d, P(bb), m + 3, R.GATHER_ROWS, P(xb), d + 12,
                                                   P(mb) if want_mul else None, d + 4, P(sb) if want_sum else None, d + 8,
                                                   _stream()), "lpf_pair_gather_f32")
                torch.cuda.synchronize()
                return mb, sb
            (mb, sb), (mb2, sb2) = run(), run()
            tag = f"pair_gather D={d} M={m} mul={want_mul} sum={want_sum}"
            assert torch.equal(mb[:, :d], mb2[:, :d]) and torch.equal(sb[:, :d], sb2[:, :d]), tag
            for buf, wanted, ref, what in ((mb, want_mul, ref_mul, "mul"), (sb, want_sum, ref_sum, "sum")):
                assert bool(torch.isnan(buf[:, d:]).all()), tag
                if not wanted:
                    assert bool((buf[:, :d] == SENT).all()), tag             # an output that was not asked for
                    continue
                _report(f"{tag} {what}", R.compare(buf[:, :d], ref, _classes(c)), worst)
                assert got.setdefault(what, buf[:, :d]).equal(buf[:, :d]), tag   # the same bits alone and beside the other
    for bad in (6, 260):
        mb = _out_buf(2, 264, 0)
        xb = torch.ones(R.GATHER_ROWS, 264, device=DEV)
        assert lib.lpf_pair_gather_f32(1, bad, P(bb), m + 3, R.GATHER_ROWS, P(xb), 264, P(mb), 264, None, 0,
                                       _stream()) == UNSUPPORTED
        torch.cuda.synchronize()
        assert bool((mb == SENT).all())
    print(f"pair_gather D={d}: worst err / tolerance {max(worst):.4f}")


@pytest.mark.parametrize("k", R.ROWDOT_WIDTHS)
def test_rowdot_sigmoid(k):
    """(F) lpf_rowdot_sigmoid_f32 at M = 1, 5 and one trip + 5, lda = K + 3; logit only, prob only, both; the planted
    logits of 100.3 and -99.7 give probabilities of exactly 1 and 0, never NaN.

    Measured on an MI355X, worst err / tolerance: K = 1: 0.004, 63: 0.029, 64: 0.028, 65: 0.021, 130: 0.035."""
    lib = _lib.hip()
    worst = []
    for m in (1, 5, R.rowwise_trip_rows() + 5):
        c = R.rowdot_case(k, m)
        g = _dev(c)
        ab = _padded(c.a, 3)
        ref_logit, ref_prob = R.rowdot64(g.a, g.w, c.bias)
        got = {}
        for want_logit, want_prob in ((True, False), (False, True), (True, True)):
            def run():
                lb = torch.full((m + 1,), SENT, device=DEV)
                pb = torch.full((m + 1,), SENT, device=DEV)
                _lib.check(lib.lpf_rowdot_sigmoid_f32(m, k, P(ab), k + 3, P(g.w), c.bias, P(lb) if want_logit else None,
                                                      P(pb) if want_prob else None, _stream()), "lpf_rowdot_sigmoid_f32")
                torch.cuda.synchronize()
                return lb, pb
            (lb, pb), (lb2, pb2) = run(), run()
            tag = f"rowdot K={k} M={m} logit={want_logit} prob={want_prob}"
            assert torch.equal(lb, lb2) and torch.equal(pb, pb2), tag
            for buf, wanted, ref, what in ((lb, want_logit, ref_logit, "logit"), (pb, want_prob, ref_prob, "prob")):
                assert float(buf[m]) == SENT, tag
                if not wanted:
                    assert bool((buf == SENT).all()), tag
                    continue
                _report(f"{tag} {what}", R.compare(buf[:m], ref, _classes(c)), worst)
                assert got.setdefault(what, buf[:m]).equal(buf[:m]), tag
            if want_prob and m >= 5:
                assert bool((pb[:m][g.sat > 0] == 1.0).all()) and bool((pb[:m][g.sat < 0] == 0.0).all()), tag
                assert int((g.sat != 0).sum()) >= 3
    print(f"rowdot K={k}: worst err / tolerance {max(worst):.4f}")
