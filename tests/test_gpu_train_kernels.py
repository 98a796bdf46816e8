"""The training kernels of the pair stage (csrc/pair_train.hip), one by one, against the fp64 restatements of
tests/train_kernel_reference.py -- at the batch sizes a real training step has (above the 512-workgroup launch cap, where
the grid-stride loops and the carry of the per-wave partial sums start), at d != dh, at a score range of 80 units, with
padded leading dimensions, and at the edges of the run walk of the by-key row sum.

Reach map -- entry point: test: the cap or edge it crosses.  ``pt_blocks(units, per_block)`` launches
ceil(units / per_block) workgroups of 4 waves, at most 512; G = D / 4 lanes own a row, a wave takes 64 / G rows a trip.
  lpf_pair_attention_train_fwd_f32   test_attention_above_the_block_cap (a): per_block = 4 * (64 / G) pairs, so 512
  lpf_pair_attention_train_bwd_f32     workgroups hold 512 * 16 * 128 / D pairs: 16384 / 8192 / 4096 / 2048 at D = 32 /
                                       64 / 128 / 256; bs = 17001 / 9001 / 5003 / 2601 lies 617 / 809 / 907 / 553 above
                                       it: the first waves take a second trip (and carry datt / dbias over it), the last
                                       wave of that trip is ragged (bs is odd), most waves take one trip.
                                     test_attention_with_keys_wider_than_the_hidden_layer (b): d = 2 dh.
                                     test_attention_at_a_wide_score_range (c): the online softmax's rescales and
                                       exp(score - pmax) * pinv at a range of 80.
                                     test_attention_c_abi_padded_leading_dimensions_and_dz_atomics (d): every ld* = D + 8
                                       and the dZ != NULL branch (float atomics), which has no Python caller.
  lpf_pe_hidden_fwd_f32              (a), (b), (c) through train.PairAttentionFn; direct in
  lpf_pe_hidden_bwd_f32                test_pe_hidden_direct (g): per_block = 64 entries, 512 workgroups hold 32768;
                                       n = 40003 = 32768 + 7235 (odd: no multiple of the 8 / 4 / 2 / 1 entries a wave
                                       takes), pa / pb at element offsets 1 and 3 (not 16-byte aligned), n = 0, 1, 3.
  lpf_segment_rows_sum_f32           test_segment_rows_sum_direct (e): runs of 1 .. 9 and 5000, the last run ending at n
                                       with every length mod 4, unnamed rows, ldd = D + 4; bit-exact.  Also (a), (b), (d),
                                       (f).
  lpf_pair_scatter_add_f32           test_pair_gather_fn_both_backward_paths (f): ``PairGatherFn`` with end_sort = None.
  lpf_colsum_f32                     test_colsum (h) through train._colsum, its only caller: per_block = 256 rows, 512
                                       workgroups hold 131072; M = 140001 = 131072 + 8929; row stride D + 4.
  lpf_train_partial_blocks           sizes every workspace above (512).

Tolerances at benign ranges are the ones tests/test_gpu_train.py holds the same kernels to: forward
2e-5 max(1, max|ref|), gradients 2e-4 max(1, max|want|).  Every test prints its worst err / tolerance.  The capped
batches of (a) draw {0, 0, 1, 2, 3} entries per (type, pair) with 30 % of the pairs emptied, as asked: 2.5 entries a pair,
43 k entries at D = 32 (above the "about 35 k" the same request hoped for; the reference takes a product per type and
does not mind).

No number in this file was known before it was written: the sizes follow from the launch arithmetic above, the
tolerances from the existing test and the reference's own error; what the card measured is recorded in the docstrings.
"""
import types

import numpy as np
import pytest
import torch

from lpformer_amd import _lib, train
from tests import train_kernel_reference as R
from tests.test_gpu_f32_reference import WIDE_RANGE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_TOL, GRAD_TOL = 2e-5, 2e-4
NAMES = ("dz", "dq", "datt", "dbias", "dwfold", "dbfold", "dw1", "db1", "dgamma", "dbeta")
WIDTHS = (32, 64, 128, 256)
CAP_BLOCKS = 512
CAPPED_BS = {32: 17001, 64: 9001, 128: 5003, 256: 2601}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _tol(want, rel):
    return rel * max(1.0, float(want.abs().max())) if want.numel() else rel


def _err(got, want):
    return float((got.double() - want.double()).abs().max()) if want.numel() else 0.0


# ------------------------------------------------------------------------------------------------ attention cases
def _case(d, dh, bs, counts, rng, n_nodes=500):
    """Inputs of ``PairAttentionFn`` for ``counts`` [3, bs]; draws in the order of the existing test
    (test_attention_stage_training_kernels_match_fp64_autograd), from ``rng`` / the torch generator as they stand."""
    n_t = counts.shape[0]
    seg, tbase, n = R.layout(counts)
    c = types.SimpleNamespace(d=d, dh=dh, bs=bs, n=n, n_t=n_t, counts=counts, seg=seg, tbase=tbase)
    c.e_node = torch.from_numpy(rng.integers(0, n_nodes, n).astype(np.int32)).to(DEV)
    c.e_pa, c.e_pb = (torch.from_numpy(rng.random(n).astype(np.float32) * 0.05).to(DEV) for _ in range(2))
    mk = lambda *shape, s=1.0: (s * torch.randn(*shape, device=DEV)).requires_grad_()
    z, q = mk(n_nodes, d), mk(bs, d)
    att, bias = mk(d, s=0.3), mk(d, s=0.1)
    wfold, bfold = mk(n_t, d, dh, s=dh ** -0.5), mk(n_t, d, s=0.1)
    w1s, b1s = mk(n_t, dh, 2, s=3.0), mk(n_t, dh, s=0.2)
    gams, bets = (1 + 0.1 * torch.randn(n_t, dh, device=DEV)).requires_grad_(), mk(n_t, dh, s=0.1)
    c.params = [z, q, att, bias, wfold, bfold, w1s, b1s, gams, bets]
    c.up = torch.randn(bs, d, device=DEV)
    c.seg_dev = torch.from_numpy(seg.reshape(-1)).to(DEV)
    c.pair = R.pair_of_entries(seg, DEV)
    c.empty = torch.from_numpy(counts.sum(0) == 0).to(DEV)
    return c


def _existing_case(d, dh=None):
    """The batch of the existing test at width d (bs = 301, 0 .. 6 entries per (type, pair), 30 % of the pairs empty,
    hub pairs of 37, 130 and 41 entries); dh != d: the same batch with a narrower hidden layer."""
    torch.manual_seed(d)
    rng = np.random.default_rng(d)
    bs = 301
    counts = rng.integers(0, 7, (3, bs))
    counts[:, rng.random(bs) < 0.3] = 0
    counts[0, 5], counts[1, 17], counts[2, 200] = 37, 130, 41
    return _case(d, d if dh is None else dh, bs, counts, rng)


def _capped_case(d):
    bs, cap = CAPPED_BS[d], CAP_BLOCKS * 4 * (64 // (d // 4))
    assert cap < bs and (bs - cap) * 2 < cap and bs % 2 == 1      # few waves take a second trip; its last wave is ragged
    torch.manual_seed(1000 + d)
    rng = np.random.default_rng(1000 + d)
    counts = rng.choice(np.array([0, 0, 1, 2, 3]), size=(3, bs))
    counts[:, rng.random(bs) < 0.3] = 0
    # hub pairs: in the first trip, in the last live lane group of the batch, in the second trip
    counts[0, 5], counts[1, bs - 1], counts[2, cap + 200] = 37, 130, 41
    assert cap + 200 < bs - 1
    c = _case(d, d, bs, counts, rng)
    assert 0.25 < float(c.empty.float().mean()) < 0.4 and c.n < 48000
    return c


def _kernels(c, params=None):
    """One forward + backward of ``PairAttentionFn`` -> (out, the ten gradients, the saved raw scores)."""
    params = c.params if params is None else params
    for p in params:
        p.grad = None
    out = train.PairAttentionFn.apply(*params, c.e_node, c.e_pa, c.e_pb, c.seg_dev, tuple(c.tbase))
    score = out.grad_fn.saved_tensors[-3][:c.n].clone()       # (..., out, score, pmax, pinv)
    (out * c.up).sum().backward()
    return out.detach().clone(), [p.grad.clone() for p in params], score


def _restated(c, dtype, params=None):
    """The restatement and its autograd gradients in ``dtype`` -> (out, the ten gradients, scores)."""
    P = [p.detach().to(dtype).requires_grad_() for p in (c.params if params is None else params)]
    out, s, _ = R.attention64(*P, c.e_node, c.e_pa.to(dtype), c.e_pb.to(dtype), c.pair, c.tbase, detail=True)
    (out * c.up.to(dtype)).sum().backward()
    return out.detach(), [p.grad for p in P], s.detach()


def _check_against_fp64(tag, c, params=None):
    """Output and all ten gradients at the benign tolerances, two runs bitwise equal, rows without entries."""
    params = c.params if params is None else params
    out, got, score = _kernels(c, params)
    out2, got2, score2 = _kernels(c, params)
    ref, want, s_ref = _restated(c, torch.float64, params)
    ratios = {"out": _err(out, ref) / _tol(ref, FWD_TOL)}
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape, name
        ratios[name] = _err(g, w) / _tol(w, GRAD_TOL)
    worst = max(ratios, key=ratios.get)
    print(f"{tag}: n = {c.n}, worst err / tolerance {ratios[worst]:.3f} ({worst}); " +
          " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert torch.isfinite(score).all() and _err(score, s_ref) <= FWD_TOL * max(1.0, float(s_ref.abs().max()))
    for name, r in ratios.items():
        assert r <= 1.0, (tag, name, r)
    # every reduction has a fixed order
    assert torch.equal(out, out2) and torch.equal(score, score2)
    for name, g, g2 in zip(NAMES, got, got2):
        assert torch.equal(g, g2), (tag, name)
    # pairs without entries: the bias, and no gradient to their query
    n_empty = int(c.empty.sum())
    assert n_empty > 0
    assert torch.equal(out[c.empty], params[3].detach().expand(n_empty, c.d))
    assert int(torch.count_nonzero(got[1][c.empty])) == 0
    assert int(torch.count_nonzero(got[1][~c.empty])) > 0
    return ratios


@pytest.mark.parametrize("dim", WIDTHS)
def test_attention_above_the_block_cap(dim):
    """(a) ``PairAttentionFn`` with bs just above the 512-workgroup cap of both attention kernels: forward and all ten
    gradients against the fp64 restatement at the benign tolerances, bitwise repeatable, empty pairs exact."""
    _check_against_fp64(f"capped D={dim} bs={CAPPED_BS[dim]}", _capped_case(dim))


@pytest.mark.parametrize("d,dh", [(64, 32), (128, 64), (256, 128)])
def test_attention_with_keys_wider_than_the_hidden_layer(d, dh):
    """(b) The first of two attention layers: keys, queries and output 2 dim wide, the PE hidden layer dim wide
    (wfold [3, d, dh]; pe_hidden_* at dh, the attention kernels at d)."""
    _check_against_fp64(f"d={d} dh={dh}", _existing_case(d, dh))


@pytest.mark.parametrize("dim", [64, 256])
def test_attention_at_a_wide_score_range(dim):
    """(c) The existing test's inputs with ``att`` scaled so that the widest pair's score range in the fp64 reference is
    80 (scores are linear in att): exp(-80) ... 1 inside one softmax, in the forward's online rescales and in the
    backward's exp(score - pmax) * pinv.

    Tolerance per tensor: max(8 x the error of the restatement run in fp32 torch against fp64, the benign tolerance).
    The yardstick is measured against the reference only; 8 covers the other summation orders and the hardware
    exponential's extra ulps at arguments of magnitude 80.

    Measured on an MI355X (max |error| against fp64: kernel, yardstick, their ratio; none of it was known when the test
    was written, and the yardstick's last digits move from run to run with the order of torch's atomic index_add):

                 D = 64 (gain 5.56)                D = 256 (gain 2.57)
      out        5.45e-06  4.58e-06  1.19          8.84e-06  1.38e-05  0.64
      dz         8.93e-05  9.79e-05  0.91          1.73e-04  1.51e-04  1.15
      dq         9.94e-05  8.08e-05  1.23          1.33e-04  3.03e-04  0.44
      datt       9.99e-05  6.94e-05  1.44          4.21e-04  4.19e-04  1.00
      dbias      4.19e-06  3.19e-06  1.31          5.38e-06  6.79e-06  0.79
      dwfold     4.44e-04  3.53e-04  1.26          1.07e-03  1.24e-03  0.87
      dbfold     7.96e-05  8.88e-05  0.90          1.79e-04  1.86e-04  0.96
      dw1        1.72e-05  1.24e-05  1.38          2.55e-05  2.52e-05  1.01
      db1        5.55e-04  4.38e-04  1.27          7.89e-04  8.01e-04  0.98
      dgamma     1.43e-04  8.53e-05  1.67          3.83e-04  2.74e-04  1.40
      dbeta      1.06e-04  7.70e-05  1.37          1.82e-04  1.80e-04  1.01

    The kernels are as good as torch's own fp32 (ratios 0.4 ... 1.7 against the 8 allowed).  With max|gradient| of
    14 ... 560 the benign floor is the larger term for every tensor here (worst err / tolerance 0.05): at this range the
    floor, not the factor, is what holds the kernels."""
    c = _existing_case(dim)
    _, _, s1 = _restated(c, torch.float64)
    widest = float(R.score_ranges(s1, c.pair, c.bs).max())
    assert widest > 0
    att_wide = (c.params[2].detach() * (WIDE_RANGE / widest)).requires_grad_()
    params = c.params[:2] + [att_wide] + c.params[3:]
    ref, want, s_ref = _restated(c, torch.float64, params)
    rng_wide = float(R.score_ranges(s_ref, c.pair, c.bs).max())
    assert abs(rng_wide - WIDE_RANGE) <= 1.0, rng_wide
    y_out, y_grads, _ = _restated(c, torch.float32, params)
    out, got, score = _kernels(c, params)
    assert torch.isfinite(score).all() and torch.isfinite(out).all()
    worst = 0.0
    rows = [("out", out, y_out, ref, FWD_TOL)] + [(n_, g, y, w, GRAD_TOL) for n_, g, y, w in zip(NAMES, got, y_grads, want)]
    fails = []
    for name, g, y, w, rel in rows:
        assert torch.isfinite(g).all(), name
        ek, ey = _err(g, w), _err(y, w)
        tol = max(8.0 * ey, _tol(w, rel))
        worst = max(worst, ek / tol)
        print(f"wide D={dim} {name}: kernel {ek:.3e} yardstick {ey:.3e} ratio {ek / ey if ey > 0 else float('inf'):.2f} "
              f"max|ref| {float(w.abs().max()):.3e} err/tol {ek / tol:.3f}")
        if ek > tol:
            fails.append((name, ek, ey, tol))
    print(f"wide D={dim}: range {rng_wide:.3f} (gain {WIDE_RANGE / widest:.2f}), worst err / tolerance {worst:.3f}")
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ (d) C ABI, padded
def _padded(t, pad, fill=7.0):
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=torch.float32, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf


def _attention_abi(c, z, kp, q, att, bias, dout, pad, with_dz):
    """lpf_pair_attention_train_fwd_f32 + _bwd_f32 with every matrix in a buffer ``pad`` floats wider than D."""
    lib, st = _lib.hip(), _stream()
    d, bs, n, ld = c.d, c.bs, c.n, c.d + pad
    zb, kb, qb, db = (_padded(t, pad) for t in (z, kp, q, dout))
    new = lambda rows: torch.full((rows, ld), 7.0, dtype=torch.float32, device=DEV)
    out, dk, dq = new(bs), new(n), new(bs)
    dz = None
    if with_dz:
        dz = new(z.shape[0])
        dz[:, :d] = 0
    score = torch.empty(n, dtype=torch.float32, device=DEV)
    pmax, pinv = torch.empty(bs, dtype=torch.float32, device=DEV), torch.empty(bs, dtype=torch.float32, device=DEV)
    dab = torch.empty(2, d, dtype=torch.float32, device=DEV)
    ws = torch.empty(int(lib.lpf_train_partial_blocks(bs)) * 2 * d, dtype=torch.float32, device=DEV)
    P = _lib.ptr
    _lib.check(lib.lpf_pair_attention_train_fwd_f32(bs, n, d, P(c.seg_dev), P(c.e_node), P(zb), ld, P(kb), ld, P(qb), ld,
                                                    P(att), P(bias), P(out), ld, P(score), P(pmax), P(pinv), st),
               "lpf_pair_attention_train_fwd_f32")
    _lib.check(lib.lpf_pair_attention_train_bwd_f32(bs, n, d, P(c.seg_dev), P(c.e_node), P(zb), ld, P(kb), ld, P(qb), ld,
                                                    P(att), P(bias), P(out), ld, P(score), P(pmax), P(pinv), P(db), ld,
                                                    P(dk), ld, P(dz), ld, P(dq), ld, P(dab), P(ws), st),
               "lpf_pair_attention_train_bwd_f32")
    torch.cuda.synchronize()
    return dict(Z=zb, KP=kb, q=qb, dout=db, out=out, dK=dk, dq=dq, dZ=dz, score=score, pmax=pmax, pinv=pinv, dab=dab)


@pytest.mark.parametrize("dim", [32, 128])
def test_attention_c_abi_padded_leading_dimensions_and_dz_atomics(dim):
    """(d) Both attention entry points through the C ABI with Z, KP, q, out, dout, dK, dq and dZ in buffers 8 floats
    wider than D (prefilled with 7.0) and a non-NULL dZ: the padding is untouched, everything but dZ is bitwise what the
    contiguous call gives, and the float-atomics dZ is the by-node sum of dK (fp64 index_add, and
    lpf_segment_rows_sum_f32 of the same dK) within the gradient tolerance -- the atomics' order is free."""
    c = _existing_case(dim)
    torch.manual_seed(7 + dim)
    n_nodes = c.params[0].shape[0]
    z, q, att, bias = (p.detach() for p in c.params[:4])
    kp = torch.randn(c.n, dim, device=DEV)
    a = _attention_abi(c, z, kp, q, att, bias, c.up, 8, True)
    b = _attention_abi(c, z, kp, q, att, bias, c.up, 0, False)
    for name in ("Z", "KP", "q", "dout", "out", "dK", "dq", "dZ"):
        pad = a[name][:, dim:]
        assert pad.shape[1] == 8 and bool((pad == 7.0).all()), name
    for name in ("Z", "KP", "q", "dout"):
        assert torch.equal(a[name][:, :dim], b[name]), name            # (inputs: not written to)
    for name in ("out", "dK", "dq"):
        assert torch.equal(a[name][:, :dim], b[name]), name
    for name in ("score", "pmax", "pinv", "dab"):
        assert torch.equal(a[name], b[name]), name
    assert float(b["dK"].abs().max()) > 0 and float(b["dab"].abs().min()) > 0
    # dZ: the by-node sum of dK
    dk = b["dK"]
    want = torch.zeros(n_nodes, dim, dtype=torch.float64, device=DEV).index_add(0, c.e_node.long(), dk.double())
    dz = a["dZ"][:, :dim]
    keys, order = torch.sort(c.e_node, stable=True)
    by_key = torch.zeros(n_nodes, dim, dtype=torch.float32, device=DEV)
    _lib.check(_lib.hip().lpf_segment_rows_sum_f32(c.n, dim, _lib.ptr(keys), _lib.ptr(order), _lib.ptr(dk), dim,
                                                   _lib.ptr(by_key), dim, _stream()), "lpf_segment_rows_sum_f32")
    tol = _tol(want, GRAD_TOL)
    e1, e2, e3 = _err(dz, want), _err(by_key, want), _err(dz, by_key)
    print(f"abi D={dim}: dZ atomics err/tol {e1 / tol:.4f}, by-key sum {e2 / tol:.4f}, atomics vs by-key {e3 / tol:.4f}")
    assert e1 <= tol and e2 <= tol and e3 <= tol
    untouched = torch.ones(n_nodes, dtype=torch.bool, device=DEV)
    untouched[c.e_node.long()] = False
    assert int(torch.count_nonzero(dz[untouched])) == 0


# ------------------------------------------------------------------------------------------------ (e) rows by key
@pytest.mark.parametrize("rem", [0, 1, 2, 3])
@pytest.mark.parametrize("dim", WIDTHS)
def test_segment_rows_sum_direct(dim, rem):
    """(e) lpf_segment_rows_sum_f32 against the sequential float32 restatement, bit for bit: runs of 1 .. 9 (three of
    each, shuffled), a hub run of 5000, the last run ending exactly at n with 8 + rem rows (so the four-row walk leaves
    by ``j0 < n`` / by ``!in[3]`` at every offset), keys that name two thirds of the destination rows, a random
    ``order``, ldd = D + 4 over a destination prefilled with 7.0."""
    rng = np.random.default_rng(100 * dim + rem)
    lengths = list(rng.permutation(np.repeat(np.arange(1, 10), 3)))
    lengths.insert(11, 5000)
    lengths.append(8 + rem)
    n_dst = (3 * len(lengths)) // 2
    key_vals = np.sort(rng.choice(n_dst, size=len(lengths), replace=False))
    keys_np = np.repeat(key_vals.astype(np.int32), lengths)
    n = keys_np.size
    assert n == 135 + 5000 + 8 + rem and keys_np[-1] == keys_np[n - 8 - rem] != keys_np[n - 9 - rem]
    order_np = rng.permutation(n).astype(np.int64)
    src_np = rng.standard_normal((n, dim)).astype(np.float32)
    want_keys, want = R.segment_sum_seq32(keys_np, order_np, src_np)
    assert np.array_equal(want_keys, key_vals)
    keys, order, src = (torch.from_numpy(a).to(DEV) for a in (keys_np, order_np, src_np))
    ld = dim + 4

    def run():
        dst = torch.full((n_dst, ld), 7.0, dtype=torch.float32, device=DEV)
        _lib.check(_lib.hip().lpf_segment_rows_sum_f32(n, dim, _lib.ptr(keys), _lib.ptr(order), _lib.ptr(src), dim,
                                                       _lib.ptr(dst), ld, _stream()), "lpf_segment_rows_sum_f32")
        torch.cuda.synchronize()
        return dst
    dst, dst2 = run(), run()
    got = dst.cpu().numpy()
    named = np.zeros(n_dst, bool)
    named[key_vals] = True
    assert 0.3 < 1 - named.mean() < 0.37
    diff = got[key_vals, :dim] != want
    print(f"segment sum D={dim} last run {8 + rem}: {int(diff.sum())} of {diff.size} elements differ in bits "
          f"(err / tolerance {float(diff.any()):.1f})")
    assert not diff.any(), np.argwhere(diff)[:5]
    assert (got[~named] == 7.0).all() and (got[:, dim:] == 7.0).all()
    assert torch.equal(dst, dst2)


# ------------------------------------------------------------------------------------------------ (f) endpoint gathers
@pytest.mark.parametrize("dim", WIDTHS)
def test_pair_gather_fn_both_backward_paths(dim):
    """(f) ``train.PairGatherFn``: forward bitwise x[a] * x[b] / x[a] + x[b]; backward by the sorted endpoint list
    (lpf_segment_rows_sum_f32: bitwise repeatable) and, end_sort = None, by float atomics (lpf_pair_scatter_add_f32), both
    against fp64 autograd -- 3001 pairs (a ragged last wave at every D) over 700 nodes, pairs with a == b, node 13 an
    endpoint of 2500 pairs."""
    n, bs, hub = 700, 3001, 13
    rng = np.random.default_rng(dim + 1)
    torch.manual_seed(dim + 1)
    batch_np = rng.integers(0, n, (2, bs))
    shuffled = rng.permutation(bs)
    hub_pairs, same = shuffled[:2500], shuffled[2500:2540]
    batch_np[rng.integers(0, 2, 2500), hub_pairs] = hub
    batch_np[1, same] = batch_np[0, same]
    batch_np[:, hub_pairs[:3]] = hub                                      # (the hub paired with itself, too)
    assert int(((batch_np[0] == hub) | (batch_np[1] == hub)).sum()) >= 2500 and int((batch_np[0] == batch_np[1]).sum()) >= 30
    batch = torch.from_numpy(batch_np).to(DEV)
    x = torch.randn(n, dim, device=DEV)
    up = torch.randn(bs, dim, device=DEV)
    k, o = torch.sort(batch.reshape(-1), stable=True)
    end_sort = (k.to(torch.int32), o)
    worst = 0.0
    for product in (True, False):
        x64 = x.double().requires_grad_()
        (R.pair_gather64(x64, batch, product) * up.double()).sum().backward()
        want = x64.grad
        tol = _tol(want, GRAD_TOL)
        fwd = R.pair_gather64(x, batch, product)                      # float32: one rounding, as the kernel's

        def grad(sort):
            xg = x.clone().requires_grad_()
            out = train.PairGatherFn.apply(xg, batch, product, sort)
            assert torch.equal(out.detach(), fwd), product
            (out * up).sum().backward()
            return xg.grad
        g_sorted, g_sorted2, g_atomic = grad(end_sort), grad(end_sort), grad(None)
        assert torch.equal(g_sorted, g_sorted2), product
        e1, e2, e3 = _err(g_sorted, want), _err(g_atomic, want), _err(g_sorted, g_atomic)
        worst = max(worst, e1 / tol, e2 / tol, e3 / tol)
        print(f"pair gather D={dim} product={product}: sorted {e1 / tol:.4f} atomics {e2 / tol:.4f} "
              f"sorted vs atomics {e3 / tol:.4f} (err / tolerance; max|want| {float(want.abs().max()):.1f})")
        assert e1 <= tol and e2 <= tol and e3 <= tol, (product, e1, e2, e3, tol)
    print(f"pair gather D={dim}: worst err / tolerance {worst:.4f}")


# ------------------------------------------------------------------------------------------------ (g) PE hidden layer
KINK = 1e-5


@pytest.mark.parametrize("dim", WIDTHS)
def test_pe_hidden_direct(dim):
    """(g) lpf_pe_hidden_fwd_f32 / _bwd_f32 of one type for 1, 3 and 40003 entries (above the 32768 the 512 workgroups
    hold), pa / pb at element offsets 0, 1 and 3 of a longer array (1 and 3: not 16-byte aligned, what ``PairAttentionFn``
    passes for the second and third type), values in [0, 0.05] with exact zeros and pa == pb: H elementwise and the five
    gradient rows (dw1[:, 0], dw1[:, 1], db1, dgamma, dbeta) against fp64 autograd of (H * dH).sum(); no entries: five
    rows of zeros.

    The ReLU's derivative jumps at 0: where an argument of the fp64 reference lies within 1e-5 of it (a few hundred of
    the 2 x 40003 x D arguments; fp32 rounds the argument by some 1e-7) float32 and float64 may take different sides,
    and either is right.  dH is set to 0 at those elements -- chosen from the reference alone -- so that the comparison
    sees the kernel's arithmetic and not that tie."""
    lib, st, P = _lib.hip(), _stream(), _lib.ptr
    torch.manual_seed(50 + dim)
    rng = np.random.default_rng(50 + dim)
    w1 = 3.0 * torch.randn(dim, 2, device=DEV)
    b1, gam, bet = 0.2 * torch.randn(dim, device=DEV), 1 + 0.1 * torch.randn(dim, device=DEV), 0.1 * torch.randn(dim, device=DEV)
    ws = torch.empty(int(lib.lpf_train_partial_blocks(0)) * 5 * dim, dtype=torch.float32, device=DEV)
    worst = 0.0
    for n in (1, 3, 40003):
        assert n <= 3 or (n > CAP_BLOCKS * 64 and n % 2 == 1)
        for off in (0, 1, 3):
            a_np, b_np = (rng.random(n + 3) * 0.05).astype(np.float32), (rng.random(n + 3) * 0.05).astype(np.float32)
            a_np[rng.random(n + 3) < 0.1] = 0.0
            b_np[rng.random(n + 3) < 0.1] = 0.0
            eq = rng.random(n + 3) < 0.1
            b_np[eq] = a_np[eq]
            if n == 3:
                a_np[off], b_np[off], b_np[off + 1] = 0.0, 0.0, a_np[off + 1]    # (the small cases hold both edges too)
            pa_all, pb_all = torch.from_numpy(a_np).to(DEV), torch.from_numpy(b_np).to(DEV)
            pa, pb = pa_all[off:off + n], pb_all[off:off + n]
            assert pa.data_ptr() == pa_all.data_ptr() + 4 * off and (off == 0 or pa.data_ptr() % 16 != 0)
            # fp64
            p64 = [t.double().requires_grad_() for t in (w1, b1, gam, bet)]
            h64, a1, a2 = R.pe_hidden64(*p64, pa.double(), pb.double(), relu_args=True)
            dh = torch.randn(n, dim, device=DEV)
            near = (a1.detach().abs() < KINK) | (a2.detach().abs() < KINK)
            assert float(near.float().mean()) < 1e-3
            dh[near] = 0.0
            (h64 * dh.double()).sum().backward()
            want = torch.stack([p64[0].grad[:, 0], p64[0].grad[:, 1], p64[1].grad, p64[2].grad, p64[3].grad])
            # kernels
            h = torch.full((n, dim), 7.0, dtype=torch.float32, device=DEV)
            _lib.check(lib.lpf_pe_hidden_fwd_f32(n, dim, P(w1), P(b1), P(gam), P(bet), pa.data_ptr(), pb.data_ptr(), P(h),
                                                 dim, st), "lpf_pe_hidden_fwd_f32")
            g5 = torch.full((5, dim), 7.0, dtype=torch.float32, device=DEV)
            _lib.check(lib.lpf_pe_hidden_bwd_f32(n, dim, P(w1), P(b1), P(gam), P(bet), pa.data_ptr(), pb.data_ptr(), P(dh),
                                                 dim, P(g5), P(ws), st), "lpf_pe_hidden_bwd_f32")
            torch.cuda.synchronize()
            rf = _err(h, h64.detach()) / _tol(h64.detach(), FWD_TOL)
            rg = max(_err(g5[i], want[i]) / _tol(want[i], GRAD_TOL) for i in range(5))
            worst = max(worst, rf, rg)
            print(f"pe hidden D={dim} n={n} offset={off}: H {rf:.4f} gradients {rg:.4f} (err / tolerance; "
                  f"{int(near.sum())} elements near the kink)")
            assert rf <= 1.0 and rg <= 1.0, (n, off, rf, rg)
    g5 = torch.full((5, dim), 7.0, dtype=torch.float32, device=DEV)
    _lib.check(lib.lpf_pe_hidden_bwd_f32(0, dim, P(w1), P(b1), P(gam), P(bet), None, None, None, dim, P(g5), P(ws), st),
               "lpf_pe_hidden_bwd_f32")
    assert int(torch.count_nonzero(g5)) == 0
    print(f"pe hidden D={dim}: worst err / tolerance {worst:.4f}")


# ------------------------------------------------------------------------------------------------ (h) column sums
@pytest.mark.parametrize("dim", [4, 36, 256])
def test_colsum(dim):
    """(h) ``train._colsum`` (lpf_colsum_f32) over 0, 1, 257 and 140001 rows (above the 131072 the 512 workgroups hold) of
    a matrix with row stride D + 4, against an fp64 column sum at test_gemm_tn_weight_gradient's form of tolerance,
    2e-5 max(1, max|want|) max(1, sqrt(M) / 30); bitwise repeatable.  (A width the kernel does not take: the next test.)"""
    torch.manual_seed(dim)
    worst = 0.0
    for m in (0, 1, 257, 140001):
        assert m <= 257 or m > CAP_BLOCKS * 256
        buf = torch.randn(m, dim + 4, device=DEV)
        x = buf[:, :dim]
        assert x.stride(0) == dim + 4 and x.stride(1) == 1
        got, got2 = train._colsum(x), train._colsum(x)
        want = x.double().sum(0)
        tol = 2e-5 * max(1.0, float(want.abs().max())) * max(1.0, m ** 0.5 / 30)
        e = _err(got, want)
        worst = max(worst, e / tol)
        print(f"colsum D={dim} M={m}: err / tolerance {e / tol:.4f}")
        assert got.shape == (dim,) and got.dtype == torch.float32 and e <= tol, (m, e, tol)
        assert torch.equal(got, got2)
        if m == 0:
            assert int(torch.count_nonzero(got)) == 0
    print(f"colsum D={dim}: worst err / tolerance {worst:.4f}")


def test_colsum_routes_other_widths_to_torch(monkeypatch):
    """A width lpf_colsum_f32 does not take (D = 6) returns torch's own sum, bit for bit, without a kernel call; the
    widths of test_colsum do call the kernel."""
    calls = []
    real = _lib.hip

    class _Lib:
        def __getattr__(self, name):
            if name == "lpf_colsum_f32":
                calls.append(name)
            return getattr(real(), name)
    monkeypatch.setattr(train._lib, "hip", lambda: _Lib())
    torch.manual_seed(6)
    x = torch.randn(257, 10, device=DEV)[:, :6]
    assert torch.equal(train._colsum(x), x.sum(dim=0)) and not calls
    y = torch.randn(257, 40, device=DEV)[:, :36]
    train._colsum(y)
    assert calls == ["lpf_colsum_f32"]
