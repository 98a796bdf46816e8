"""The references and inputs of tests/node_forward_reference.py checked on the CPU, so that the GPU tests of the encoder's
forward kernels compare with something that is itself pinned: the fp64 restatements are what the oracle, scipy and torch
give; every case the GPU file runs holds the row lengths, widths and row counts its reach map claims; and the comparison
has power -- each of eleven planted faults, applied to the fp64 result of the case that is meant to catch it, is rejected
at the forward tolerance (where one was not, the inputs were changed, never the tolerance)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.nn.functional as F

from lpformer_amd import _lib, graph
from oracle import lpformer_oracle as O
from tests import node_forward_reference as R

CU = 256                                  # an MI355X; the GPU file asks the device


def _rejected(ratios):
    return max(ratios.values()) > 1.0


def _ep(c, ep, lo=0, hi=None):
    ln, relu, res, ln2 = ep
    hi = c.n if hi is None else hi
    return dict(bias=c.bias, ln=(c.g1, c.b1) if ln else None, relu=relu, residual=c.res[lo:hi] if res else None,
                ln2=(c.g2, c.b2) if ln2 else None)


def _spmm_out(c, ep, val=None, h=None, extra=None):
    agg = R.spmm64(c.rowptr, c.col, c.val if val is None else val, c.h if h is None else h)
    return R.epilogue64(agg if extra is None else agg + extra, **_ep(c, ep))


# ------------------------------------------------------------------------------------------------ the restatements
def test_restatements_agree_with_the_oracle_scipy_and_torch():
    n, d = 300, 36
    rng = np.random.default_rng(1)
    ei = rng.integers(0, n, (2, 3000))
    ei[:, :200] = np.stack([np.full(200, 7), rng.integers(0, n, 200)])      # a row of more than 128 entries
    ei = np.unique(ei, axis=1)             # (no entry twice: "all ones" then means the same to the oracle and the kernel)
    w = (rng.random(ei.shape[1]) + 0.5).astype(np.float32)
    s = graph.gcn_structure_csr(ei, w, n)                                    # every diagonal stored, as the kernel wants
    rowptr, col, val = (torch.from_numpy(a) for a in (s.rowptr, s.col, s.val))
    o_rp, o_col, o_val = O.gcn_norm(ei, w, n)
    assert np.array_equal(o_rp, s.rowptr) and np.array_equal(o_col, s.col) and np.diff(s.rowptr).max() > R.LONG_ROW
    w_out, dis = R.gcn_norm64(rowptr, col, val)
    np.testing.assert_allclose(w_out.numpy(), o_val, rtol=2e-6, atol=1e-7)
    ones, _ = R.gcn_norm64(rowptr, col, None)
    np.testing.assert_allclose(ones.numpy(), O.gcn_norm(ei, None, n)[2], rtol=2e-6, atol=1e-7)
    # the diagonal counts as 1 whatever is stored; an empty row has dis = 0, and so has every entry that names it
    val3 = val.clone()
    val3[col.long() == R._row_ids(rowptr)] = 3.0
    assert torch.equal(R.gcn_norm64(rowptr, col, val3)[0], w_out)
    c = R.norm_case(4099)
    w4, dis4 = R.gcn_norm64(c.rowptr, c.col, c.val)
    empty = torch.from_numpy(c.lengths == 0)
    assert bool((dis4[empty] == 0).all()) and bool((dis4[~empty] > 0).all()) and bool(torch.isfinite(w4).all())
    assert bool((w4[empty[c.col.long()]] == 0).all()) and int(empty[c.col.long()].sum()) > 0

    h = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32))
    got = R.spmm64(rowptr, col, w_out.float(), h)
    a = sp.csr_matrix((w_out.float().double().numpy(), s.col, s.rowptr), shape=(n, n))
    assert np.abs(got.numpy() - a @ h.double().numpy()).max() <= 1e-12
    assert np.abs(got.numpy() - O.spmm(o_rp, o_col, w_out.float().numpy(), h.numpy())).max() <= 1e-5
    g, b = torch.from_numpy(rng.standard_normal((2, d)).astype(np.float32))
    ln = R.layernorm64(got, g, b)
    assert float((ln - F.layer_norm(got, (d,), g.double(), b.double(), R.LN_EPS)).abs().max()) <= 1e-12
    assert np.abs(ln.numpy() - O.layer_norm(got.numpy(), g.numpy(), b.numpy())).max() <= 2e-5
    assert torch.equal(R.layernorm64(got, None, None, True), got.clamp_min(0))
    res = torch.from_numpy(rng.standard_normal((n, d)))
    want = F.layer_norm(torch.relu(F.layer_norm(got + g.double(), (d,), g.double(), b.double())) + res, (d,), b.double(),
                        g.double())
    assert float((R.epilogue64(got, g, (g, b), True, res, (b, g)) - want).abs().max()) <= 1e-12
    wm = torch.from_numpy(rng.standard_normal((d, d)))
    assert torch.equal(R.fused_layer64(got, wm), got @ wm.t())
    # slices: a running sum against the sum taken slice by slice
    pc = R.parts_case(24, 50)
    direct = torch.stack([(pc.h.double()[pc.col[e0:e1].long()] * pc.val[e0:e1].double()[:, None]).sum(0)
                          for e0, e1 in pc.parts.tolist()])
    assert float((R.row_parts64(pc.parts, pc.col, pc.val, pc.h) - direct).abs().max()) <= 1e-11
    gc = R.gather_case(36, 5)
    mul, tot = R.pair_gather64(gc.x, gc.batch, R.GATHER_ROWS)
    assert torch.equal(mul[0], gc.x[0].double() * gc.x[int(gc.batch[1, 0])].double())       # id -1 reads row 0
    assert torch.equal(tot[4], gc.x[int(gc.batch[0, 4])].double() + gc.x[0].double())       # id 2^40 too
    rc = R.rowdot_case(63, 5)
    logit, prob = R.rowdot64(rc.a, rc.w, rc.bias)
    assert [round(float(v), 3) for v in logit[[1, 3]]] == [100.3, -99.7]
    assert float(torch.sigmoid(logit.float())[1]) == 1.0 and float(prob[3]) < 1e-40


def test_bf16_images():
    x = torch.randn(7, 128, generator=torch.Generator().manual_seed(2)) * 10.0 ** torch.arange(-3, 4).float()[:, None]
    assert torch.equal(R.bf16_rne(x), x.to(torch.bfloat16).float())
    ties = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 1e30])    # to even, both ways
    assert R.bf16_rne(ties).tolist()[:3] == [1.0, 1.0 + 2.0 ** -6, -1.0]
    assert torch.equal(R.bf16_bits(ties), ties.to(torch.bfloat16).view(torch.int16).to(torch.int32) & 0xFFFF)
    for d in (64, 128):
        idx = R.bf16p_index(d)
        assert sorted(idx.tolist()) == list(range(d))
        # element 32 i + 8 q + 4 h + u holds feature 16 (2 i + h) + 4 q + u -- spelled out, and the model's own reshape
        assert int(idx[32 * 1 + 8 * 2 + 4 * 1 + 3]) == 16 * 3 + 4 * 2 + 3
        f = torch.arange(d).float()[None]
        assert torch.equal(R.permute_bf16p(f), f.reshape(1, d // 32, 2, 4, 4).permute(0, 1, 3, 2, 4).reshape(1, d))
        assert torch.equal(R.unpermute_bf16p(R.permute_bf16p(x[:, :d])), x[:, :d])
        assert not torch.equal(R.permute_bf16p(x[:, :d]), x[:, :d])


# ------------------------------------------------------------------------------------------------ launch arithmetic, cases
def test_launch_arithmetic():
    assert _lib.CONST["LPF_SPMM_LONG_ROW"] == R.LONG_ROW == 128 and _lib.CONST["LPF_ERR_UNSUPPORTED"] == -2
    shapes = {d: R.spmm_shape(d) for d in R.SPMM_F32_WIDTHS}
    assert shapes == {4: (1, 16, 4, 16), 24: (2, 8, 8, 32), 36: (1, 16, 4, 16), 64: (2, 8, 8, 32), 96: (2, 16, 4, 16),
                      128: (2, 16, 4, 16), 132: (1, 64, 1, 4), 256: (1, 64, 1, 4)}
    assert {d: R.spmm_shape(d, True) for d in R.SPMM_BF16_WIDTHS} == {8: (2, 8, 8, 32), 64: (2, 8, 8, 32),
                                                                     136: (2, 32, 2, 8), 256: (2, 32, 2, 8)}
    for d in R.SPMM_F32_WIDTHS + R.SPMM_BF16_WIDTHS:
        for bf16 in (False, True):
            v, g, rpw, ng = R.spmm_shape(d, bf16)
            assert 4 * v * g >= d and g * rpw == 64 and g * ng == 256
    assert R.spmm_trip_rows(132) == 32768 and R.spmm_trip_rows(128) == 131072 and R.rowwise_trip_rows() == 32768
    assert [R.gather_trip_rows(d) for d in R.GATHER_WIDTHS] == [131072, 131072, 131072, 32768, 32768]
    assert [R.parts_shape(d) for d in R.PARTS_F32_WIDTHS] == [(8, 32), (8, 32), (8, 32), (16, 16)]
    assert [R.fused_nbp(d) for d in (32, 64, 128)] == [2, 2, 4]
    assert [R.fused_cap_tiles(d, CU) for d in (32, 64, 128)] == [4096, 4096, 2048]
    assert R.spmm_lengths(36) == [0, 1, 3, 4, 5, 15, 16, 17, 35, 127, 128, 129, 255, 256, 257, 775]
    assert R.spmm_lengths(64) == [0, 1, 3, 4, 5, 7, 8, 9, 19, 127, 128, 129, 255, 256, 257, 775]
    assert R.fused_lengths(128) == [0, 1, 3, 4, 5, 9, 63, 64, 65, 256, 257, 700]
    assert R.fused_lengths(32) == [0, 1, 2, 3, 5, 63, 64, 65, 256, 257, 700]
    assert R.parts_slice_lengths(8) == [1, 7, 9, 255, 256] and R.parts_slice_lengths(128) == [1, 15, 17, 255, 256]


def _check_graph(c):
    """The CSR of a case is what ``planted_graph`` promises, and holds every planted length."""
    deg = (c.rowptr[1:] - c.rowptr[:-1]).numpy()
    assert np.array_equal(deg, c.lengths) and c.rowptr.dtype == torch.int64 and c.col.dtype == torch.int32
    hist = np.bincount(deg)
    for length in c.planted:
        assert hist[length] >= 1, length
    col = c.col.long().numpy()
    assert col.min() >= 1 and col.max() < c.n_cols                           # never row 0 of the table
    rows = np.repeat(np.arange(c.n), deg)
    same = rows[1:] == rows[:-1]
    assert bool((col[1:][same] > col[:-1][same]).all())                      # ascending and distinct within a row
    assert 0.5 < float(c.val.min()) and float(c.val.max()) < 1.5
    return hist


def test_planted_graph():
    lengths = [0, 5, 0, 1024, 1, 3]
    rowptr, col, val = R.planted_graph(lengths, 1025, 4)
    assert rowptr.tolist() == [0, 0, 5, 5, 1029, 1030, 1033] and col.dtype == np.int32 and val.dtype == np.float32
    assert sorted(col[5:1029].tolist()) == list(range(1, 1025))              # a row as long as the table minus row 0
    again = R.planted_graph(lengths, 1025, 4)
    assert all(np.array_equal(a, b) for a, b in zip((rowptr, col, val), again))
    with pytest.raises(AssertionError):
        R.planted_graph([1025], 1025, 4)


@pytest.mark.parametrize("bf16,widths", [(False, R.SPMM_F32_WIDTHS), (True, R.SPMM_BF16_WIDTHS)])
def test_spmm_cases_hold_what_they_claim(bf16, widths):
    for d in widths:
        c = R.spmm_case(d, bf16)
        hist = _check_graph(c)
        _, g, _, ng = R.spmm_shape(d, bf16)
        assert set(R.spmm_lengths(d, bf16)) >= {0, 1, 3, 4, 5, g - 1, g, g + 1, 2 * g + 3, 127, 128, 129, 255, 256, 257, 775}
        assert hist[128] == 1 and hist[129] == 1 and int((c.lengths > R.LONG_ROW).sum()) == sum(k > 128 for k in c.planted) >= 5
        assert c.n == 300 + len(c.planted) and c.h.shape == (1025, d) and 0 < c.lo < c.hi < c.n
        inside = c.lengths[c.lo:c.hi]
        assert (inside > R.LONG_ROW).any() and (inside == 0).any()
        for name, mask in c.classes.items():
            assert int(mask.sum()) >= 1, name
        if bf16:
            assert torch.equal(c.h, c.h.to(torch.bfloat16).float())


def test_second_trip_cases_hold_what_they_claim():
    assert R.SPMM_TRIP_CASES == ((132, 5), (128, 7))
    for d, above in R.SPMM_TRIP_CASES:
        c = R.spmm_trip_case(d, above)
        assert c.n == R.spmm_trip_rows(d) + above and int(c.classes["second trip"].sum()) == above
        assert c.n > R.BLOCK_CAP * 4 * R.spmm_shape(d)[2] and set(np.unique(c.lengths)) == {0, 1, 2, 3}
        assert int(c.col.min()) >= 1
    m = R.rowwise_trip_rows() + 5
    assert int(R.ln_case(3, m).classes["second trip"].sum()) == 5
    assert int(R.rowdot_case(1, m).classes["second trip"].sum()) == 5
    assert int(R.gather_case(132, m).classes["second trip"].sum()) == 5
    assert int(R.gather_case(4, R.gather_trip_rows(4) + 5).classes["second trip"].sum()) == 5


def test_parts_cases_hold_what_they_claim():
    for d in R.PARTS_F32_WIDTHS:
        g, ng = R.parts_shape(d)
        c = R.parts_case(d, R.PARTS_MANY)
        length = (c.parts[:, 1] - c.parts[:, 0]).numpy()
        assert set(length.tolist()) == {1, g - 1, g + 1, g * ng, 255, 256} and c.parts.shape == (70000, 2)
        assert int(c.parts.min()) >= 0 and int(c.parts.max()) <= c.col.numel() and int(c.col.min()) >= 1
        assert int((c.parts[:, 0] % 1024 != 0).sum()) > 69000                # starts mid-row, aligned to nothing
        one = R.parts_case(d, 1)
        assert one.parts.tolist() == [[3, 259]]


@pytest.mark.parametrize("d,bf16", [(d, False) for d in R.FUSED_F32_WIDTHS] + [(d, True) for d in R.FUSED_BF16_WIDTHS])
def test_fused_cases_hold_what_they_claim(d, bf16):
    c = R.fused_case(d, bf16)
    hist = _check_graph(c)
    nbp = R.fused_nbp(d)
    assert set(c.planted) == {0, 1, nbp - 1, nbp, nbp + 1, 2 * nbp + 1, 63, 64, 65, 256, 257, 700}
    n_hub = int((c.lengths > R.FUSED_LONG).sum())
    assert n_hub == 5 and n_hub % 2 == 1 and hist[65] == 2 and hist[64] >= 1
    for lo, hi in ((0, c.n), (c.lo, c.hi)):
        orders, hubs, parts = R.fused_orders(c.rowptr, lo, hi, bf16, 17)
        n_in = int((c.lengths[lo:hi] > R.FUSED_LONG).sum())
        assert hubs.shape == (n_in, 3) and n_in >= 1
        sl = (parts[:, 1] - parts[:, 0]).tolist()
        assert max(sl) == 256 and ((lo, hi) != (0, c.n) or sorted(sl) == [1, 65, 65, 188, 256, 256, 256, 256])
        for name, order in orders.items():
            o = order.long()
            assert o.numel() % 16 == 0 and sorted(o[o >= 0].tolist()) == [r for r in range(lo, hi) if c.lengths[r] <= 64]
            assert sorted((-2 - o[o < -1]).tolist()) == list(range(n_in)), name
            pairs = o.reshape(-1, 2)
            mixed = ((pairs < -1).sum(1) == 1) & ((pairs >= 0).sum(1) == 1)    # a hub and an ordinary row in one lane pair
            tiles = o.reshape(-1, 16)
            hub_tiles = tiles[(tiles < -1).any(1)]
            if bf16:
                assert int(mixed.sum()) == 0 and bool((hub_tiles < 0).all())   # hub tiles: hubs and -1 only
            elif name != "shuffled" and (lo, hi) == (0, c.n):
                assert int(mixed.sum()) == 1
                partner = int(pairs[mixed][0].max())
                assert c.lengths[partner] == (64 if name == "own" else 0)
        sh = orders["shuffled"].long()
        assert int((sh[:-16] == -1).sum()) >= 5                               # -1 codes inside the order
        h2, p2 = R.with_dummy_slice(hubs, parts)
        assert p2[0].tolist() == [0, 0] and torch.equal(p2[1:], parts) and int(h2[:, 1].min()) == 1


def test_fused_tile_cases_cross_the_ticket_round():
    for d in R.FUSED_F32_WIDTHS:
        for nt in R.FUSED_SMALL_TILES + (R.fused_cap_tiles(d, CU) + 11,):
            c = R.fused_tiles_case(d, nt)
            order, hubs, _ = graph.fused_row_order(c.rowptr, 0, c.n)
            assert hubs is None and order.numel() == 16 * nt and int((order == -1).sum()) == 5
            assert set(np.unique(c.lengths)) <= {1, 2, 3}
        assert c.n == {128: 32939, 64: 65707, 32: 65707}[d] and nt > 8 * (R.fused_cap_tiles(d, CU) // 8)


def test_norm_and_rowwise_cases_hold_what_they_claim():
    c = R.norm_case(4099)
    deg = (c.rowptr[1:] - c.rowptr[:-1]).numpy()
    assert np.array_equal(deg, c.lengths) and c.n % 4 == 3 and all((deg == k).any() for k in (0, 1, 63, 64, 65, 700))
    rows = np.repeat(np.arange(c.n), deg)
    col = c.col.long().numpy()
    diag = col == rows
    has = np.zeros(c.n, bool)
    has[rows[diag]] = True
    assert bool((c.val.numpy()[diag] == 3.0).all()) and int((~has & (deg > 0)).sum()) > 500 and int(has.sum()) > 2000
    assert deg[c.diag_only] == 1 and has[c.diag_only] and has[deg == 700].all()
    assert np.unique(rows * c.n + col).size == col.size
    one = R.norm_case(1)
    assert one.rowptr.tolist() == [0, 1] and one.col.tolist() == [0] and one.val.tolist() == [3.0]
    for d in R.LN_WIDTHS:
        row = R.near_constant_row(d).double()
        assert float(row.sum()) == 5.0 * d                                   # the mean is exactly 5
        var = float(((row - 5.0) ** 2).mean())
        lc = R.ln_case(d, 5)
        assert lc.const.tolist() == [True, False, True, False, True] and torch.equal(lc.x[0], row.float())
        if d > 1:
            assert 280 < (var + R.LN_EPS) ** -0.5 < 316
    gc = R.gather_case(64, 5)
    assert gc.batch[0, :3].tolist() == list(R.BAD_IDS) and gc.batch[1, 2:].tolist() == list(R.BAD_IDS)
    assert R.gather_case(64, 1).batch.tolist() == [[-1], [R.GATHER_ROWS]]


# ------------------------------------------------------------------------------------------------ the comparison has power
def test_compare_takes_each_class_by_its_own_scale():
    ref = torch.ones(4, 3, dtype=torch.float64)
    ref[0] = 1000.0
    got = ref.clone()
    got[2, 1] += 1e-3                                                         # 50 x the tolerance of a row of ones
    classes = {"big": torch.tensor([True, False, False, False]), "ones": torch.tensor([False, True, True, True]),
               "none": torch.zeros(4, dtype=torch.bool)}
    r = R.compare(got.float(), ref, classes)
    assert r["all"] < 0.1 and r["big"] == 0.0 and r["ones"] > 40 and r["none"] == 0.0
    got[3, 0] = float("nan")
    assert R.compare(got.float(), ref, classes)["all"] == float("inf")
    assert R.worst(r) == ("ones", r["ones"])


def _last_of_rows(c, keep_rows):
    """Index of the last entry of every row in ``keep_rows`` (bool over rows)."""
    return (c.rowptr[1:][keep_rows] - 1).long()


@pytest.mark.parametrize("ep", R.EPILOGUES)
@pytest.mark.parametrize("d,bf16", [(36, False), (64, False), (132, False), (136, True)])
def test_spmm_faults_are_rejected(d, bf16, ep):
    """Faults 1, 2, 3, 5 and 6 on the cases of (B) / (C), under each epilogue."""
    c = R.spmm_case(d, bf16)
    _, g, _, _ = R.spmm_shape(d, bf16)
    ref = _spmm_out(c, ep)
    assert not _rejected(R.compare(ref.float(), ref, c.classes))              # fp32 storage of the result passes
    lengths = torch.from_numpy(c.lengths)
    k = torch.arange(c.col.numel()) - c.rowptr[R._row_ids(c.rowptr)]         # an entry's position in its row
    len_e = lengths[R._row_ids(c.rowptr)]
    # 1: the last entry of every row with length % 4 == 1 dropped
    val = c.val.clone()
    val[_last_of_rows(c, lengths % 4 == 1)] = 0
    r = R.compare(_spmm_out(c, ep, val=val), ref, c.classes)
    assert _rejected(r) and r["len 1"] > 1 and r["len 5"] > 1 and r["len 129"] > 1 and r["len 4"] <= 1
    # 2: the last chunk of G entries dropped for rows longer than G
    val = torch.where((len_e > g) & (k >= (len_e - 1) // g * g), torch.zeros_like(c.val), c.val)
    r = R.compare(_spmm_out(c, ep, val=val), ref, c.classes)
    assert _rejected(r) and r[f"len {g + 1}"] > 1 and r["len 775"] > 1 and r[f"len {g}"] <= 1
    # 3: rows of exactly 129 entries left at the sentinel
    bad = ref.clone()
    bad[lengths == 129] = R.SENTINEL
    r = R.compare(bad, ref, c.classes)
    assert r["len 129"] > 1 and r["len 128"] == 0
    # 5: the lanes behind the end of a row carry lane 0's weight: they add w H[0]
    first = c.val[(c.rowptr[:-1] + (lengths - 1).clamp_min(0) // g * g).clamp_max(c.col.numel() - 1)].double()
    pad = torch.where(lengths > 0, (-lengths) % 4, torch.zeros_like(lengths)).double()
    r = R.compare(_spmm_out(c, ep, extra=(pad * first)[:, None] * c.h[0].double()), ref, c.classes)
    assert _rejected(r) and r["len 1"] > 1 and r["len 3"] > 1 and r["len 4"] <= 1
    # 6: LayerNorm's mean divided by the width the lanes cover and not by D
    if ep[0] and d in (36, 132):
        covered = 4 * R.spmm_shape(d)[0] * g
        assert covered > d
        pre = R.spmm64(c.rowptr, c.col, c.val, c.h) + c.bias.double()
        cen = pre - pre.sum(1, keepdim=True) / covered
        y = cen / torch.sqrt((cen * cen).mean(1, keepdim=True) + R.LN_EPS) * c.g1.double() + c.b1.double()
        e = _ep(c, ep)
        bad = R.epilogue64(y, None, None, e["relu"], e["residual"], e["ln2"])
        r = R.compare(bad, ref, c.classes)
        assert min(v for k_, v in r.items()) > 1


@pytest.mark.parametrize("d", R.FUSED_F32_WIDTHS)
def test_fused_faults_are_rejected(d):
    """Faults 4, 8, 9 and 10 on the cases of (E), the full epilogue and the plain one."""
    c = R.fused_case(d)
    lengths = torch.from_numpy(c.lengths)
    rows_e = R._row_ids(c.rowptr)
    k = torch.arange(c.col.numel()) - c.rowptr[rows_e]
    len_e = lengths[rows_e]
    hub_e = len_e > R.FUSED_LONG
    agg = R.spmm64(c.rowptr, c.col, c.val, c.h)
    for ep in R.EPILOGUES[:2]:
        ref = R.fused_layer64(agg, c.w, **_ep(c, ep))
        assert not _rejected(R.compare(ref.float(), ref, c.classes))
        # 4: a hub's last slice dropped; slices cut at 255 entries
        for drop in (hub_e & (k >= (len_e - 1) // 256 * 256), hub_e & (k % 256 == 255)):
            bad = R.fused_layer64(R.spmm64(c.rowptr, c.col, torch.where(drop, torch.zeros_like(c.val), c.val), c.h), c.w,
                                  **_ep(c, ep))
            r = R.compare(bad, ref, c.classes)
            assert r["hub rows"] > 1 and r["len 64"] <= 1 and (r["len 257"] > 1 or r["len 256"] > 1)
        # 8: the residual taken at `row` and not at `row - row_base` (a block's residual buffer starts at its first row)
        if ep[2]:
            blk = _ep(c, ep, c.lo, c.hi)
            ref_b = R.fused_layer64(agg[c.lo:c.hi], c.w, **blk)
            blk["residual"] = torch.roll(blk["residual"], -c.lo, 0)
            cls = {k_: m[c.lo:c.hi] for k_, m in c.classes.items()}
            r = R.compare(R.fused_layer64(agg[c.lo:c.hi], c.w, **blk), ref_b, cls)
            assert r["all"] > 1 and r["hub rows"] > 1 and all(v > 1 for v in r.values() if v > 0)
        # 9: the two k-groups of a 32-feature block swapped
        swap = agg.reshape(c.n, d // 32, 2, 16).flip(2).reshape(c.n, d)
        r = R.compare(R.fused_layer64(swap, c.w, **_ep(c, ep)), ref, c.classes)
        assert all(v > 1 for k_, v in r.items() if k_ != "empty rows" and k_ != "len 0")
    # 10: the bf16 image with q and h exchanged -- element 32 i + 16 h + 4 q + u, the normal order -- read as the
    # permuted one, or written where the permuted one is expected
    if d in R.FUSED_BF16_WIDTHS:
        cb = R.fused_case(d, True)
        aggb = R.spmm64(cb.rowptr, cb.col, cb.val, cb.h)
        ref = R.fused_layer64(aggb, cb.w, **_ep(cb, R.EPILOGUES[0]))
        wrong = R.spmm64(cb.rowptr, cb.col, cb.val, R.unpermute_bf16p(cb.h))
        r = R.compare(R.fused_layer64(wrong, cb.w, **_ep(cb, R.EPILOGUES[0])), ref, cb.classes)
        assert all(v > 1 for k_, v in r.items() if k_ != "empty rows" and k_ != "len 0")
        out = ref.float()
        assert not torch.equal(R.bf16_bits(out), R.permute_bf16p(R.bf16_bits(out)))
        pc = R.parts_case(d, 50, True)
        sums = R.row_parts64(pc.parts, pc.col, pc.val, pc.h)
        assert min(R.compare(R.permute_bf16p(sums), sums, pc.classes).values()) > 1


def _ln32(x, gamma, beta, one_pass):
    """LayerNorm restated in fp32 torch; ``one_pass``: the variance as E[x^2] - mean^2."""
    mean = x.mean(1, keepdim=True)
    var = ((x * x).mean(1, keepdim=True) - mean * mean).clamp_min(0) if one_pass else ((x - mean) ** 2).mean(1, keepdim=True)
    return (x - mean) / torch.sqrt(var + np.float32(R.LN_EPS)) * gamma + beta


@pytest.mark.parametrize("d", [w for w in R.LN_WIDTHS if w > 1])
def test_a_one_pass_variance_is_rejected_on_the_near_constant_rows(d):
    """Fault 7.  A two-pass fp32 LayerNorm passes every class with room; a one-pass variance fails the near-constant rows
    -- and, at the larger widths, only them: hence the class."""
    c = R.ln_case(d, 5)
    ref = R.layernorm64(c.x, c.gamma, c.beta)
    two = R.compare(_ln32(c.x, c.gamma, c.beta, False), ref, c.classes)
    one = R.compare(_ln32(c.x, c.gamma, c.beta, True), ref, c.classes)
    assert max(two.values()) <= 0.5, two
    assert one["near-constant rows"] > 1, one


def test_unwritten_second_trips_are_rejected():
    """Fault 11: the rows of a second trip, or the tiles of the ticket round, left at the sentinel."""
    for d, above in R.SPMM_TRIP_CASES:
        c = R.spmm_trip_case(d, above)
        ref = _spmm_out(c, R.EPILOGUES[0])
        bad = ref.clone()
        bad[R.spmm_trip_rows(d):] = R.SENTINEL
        r = R.compare(bad, ref, c.classes)
        assert r["second trip"] > 1 and all(v > 1 for v in r.values() if v > 0)
    d = 128
    c = R.fused_tiles_case(d, R.fused_cap_tiles(d, CU) + 11)
    order, _, _ = graph.fused_row_order(c.rowptr, 0, c.n)
    ticket = torch.zeros(c.n, dtype=torch.bool)
    late = order[16 * R.fused_cap_tiles(d, CU):].long()
    ticket[late[late >= 0]] = True
    assert int(ticket.sum()) == 16 * 11 - 5
    ref = R.fused_layer64(R.spmm64(c.rowptr, c.col, c.val, c.h), c.w, **_ep(c, R.EPILOGUES[0]))
    bad = ref.clone()
    bad[ticket] = R.SENTINEL
    assert R.compare(bad, ref, {"ticket round": ticket})["ticket round"] > 1
    lc = R.ln_case(3, R.rowwise_trip_rows() + 5)
    ref = R.layernorm64(lc.x, lc.gamma, lc.beta, True)
    bad = ref.clone()
    bad[R.rowwise_trip_rows():] = R.SENTINEL
    assert R.compare(bad, ref, lc.classes)["second trip"] > 1


@pytest.mark.parametrize("d", R.LN_COND_WIDTHS)
def test_the_conditioned_bound_keeps_its_power(d):
    """The drawn rows of D = 3 are held to K 2^-24 max|x_i| rstd_i |gamma_j| (``ln_cond_ratio``), not to 2e-5: three draws
    can lie so close together that no fp32 mean is exact against their spread.  That bound is a statement about fp32: a
    two-pass fp32 LayerNorm meets it on the GPU test's largest case with room, some drawn row does miss 2e-5 (so the bound
    is needed), and it still rejects an unwritten second trip and a one-pass variance on the drawn rows; the near-constant
    rows stay at 2e-5, where the one-pass variance fails too."""
    assert R.LN_COND_K == 2.0 ** round(np.log2(R.LN_COND_K)) and R.LN_COND_K <= 64
    c = R.ln_case(d, R.rowwise_trip_rows() + 5)
    ref = R.layernorm64(c.x, c.gamma, c.beta)
    other = ~c.const
    two, one = (_ln32(c.x, c.gamma, c.beta, p) for p in (False, True))
    assert float(R.ln_cond_ratio(two, ref, c.x, c.gamma)[other].max()) <= R.LN_COND_K / 2
    assert R.compare(two, ref, c.classes)["other rows"] > 1
    assert float(R.ln_cond_ratio(one, ref, c.x, c.gamma)[other].max()) > R.LN_COND_K
    assert R.compare(one, ref, c.classes)["near-constant rows"] > 1
    bad = ref.clone()
    bad[R.rowwise_trip_rows():] = R.SENTINEL
    assert float(R.ln_cond_ratio(bad, ref, c.x, c.gamma)[c.classes["second trip"]].min()) > R.LN_COND_K
