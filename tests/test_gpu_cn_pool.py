"""The common-neighbour pooling kernels (csrc/cn_pool.hip) on the MI355X: the C entries called directly against
``cn_pool_reference`` / ``cn_entries_reference`` with the derived bounds of tests/cn_pool_cases.py, exact integer sums,
one summation order whatever the class, the position, the orientation or the launch, the entry list and its clamping,
``CnPoolFn``'s backward, ``NCNPredictor`` end to end and the argument checks.  The tests print their worst
error / bound ratio; the header of tests/cn_pool_cases.py records them."""
import copy

import numpy as np
import pytest
import torch

import lpformer_amd
from lpformer_amd import _lib, data as D, ncn
from tests import cn_pool_cases as CC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_GRAPHS = {}


def _graph(name):
    """(rowptr, col) of a case on the device, uploaded once."""
    name = "C" if name == "C2" else name
    if name not in _GRAPHS:
        c = CC.case(name)
        _GRAPHS[name] = (torch.from_numpy(c.csr.rowptr).to(DEV), torch.from_numpy(c.csr.col).to(DEV))
    return _GRAPHS[name]


def _dev_w(name, kind):
    w = CC.weights(name, kind)
    return None if w is None else w.to(DEV)


def _pool(name, pairs, table, w=None, thr=-1, ldp=None, fill=float("nan"), want_cn=True):
    """lpf_cn_pool_f32 alone on device pairs [2, P] (contiguous): (pool float32 [P, ldp], cn int32 [P])."""
    rowptr, col = _graph(name)
    P, dim = pairs.shape[1], table.shape[1]
    ldp = dim if ldp is None else ldp
    pool = torch.full((P, ldp), fill, dtype=torch.float32, device=DEV)
    cn = torch.full((P,), -7, dtype=torch.int32, device=DEV) if want_cn else None
    scratch = torch.empty(P + 1, dtype=torch.int32, device=DEV)
    rc = _lib.hip().lpf_cn_pool_f32(P, CC.case(name).n, pairs.data_ptr(), P, rowptr.data_ptr(), col.data_ptr(),
                                    None if w is None else w.data_ptr(), dim, table.data_ptr(), table.stride(0), thr,
                                    scratch.data_ptr(), pool.data_ptr(), ldp, None if cn is None else cn.data_ptr(), 0)
    assert rc == 0
    torch.cuda.synchronize()
    return pool, cn


def _entries(name, pairs, seg, n_ent, thr=-1, guard=8):
    """lpf_cn_entries alone: the int32 buffer [guard + n_ent + guard] filled with -9 around and under the list."""
    rowptr, col = _graph(name)
    P = pairs.shape[1]
    buf = torch.full((guard + n_ent + guard,), -9, dtype=torch.int32, device=DEV)
    scratch = torch.empty(P + 1, dtype=torch.int32, device=DEV)
    rc = _lib.hip().lpf_cn_entries(P, CC.case(name).n, pairs.data_ptr(), P, rowptr.data_ptr(), col.data_ptr(), thr,
                                   scratch.data_ptr(), seg.data_ptr(), n_ent, buf.data_ptr() + 4 * guard, 0)
    assert rc == 0
    torch.cuda.synchronize()
    return buf


def _pairs(name):
    return CC.case(name).pairs.to(DEV).contiguous()


# ------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("name", CC.NAMES)
@pytest.mark.parametrize("dim", CC.DIMS)
def test_forward_against_the_reference(name, dim):
    c, pairs, table = CC.case(name), _pairs(name), CC.table(name, dim).to(DEV)
    k = CC.counts(name)
    rowptr, col = _graph(name)
    heur = torch.empty(pairs.shape[1], dtype=torch.int32, device=DEV)
    scratch = torch.empty(pairs.shape[1] + 1, dtype=torch.int32, device=DEV)
    assert _lib.hip().lpf_pair_heuristics_f32(pairs.shape[1], c.n, pairs.data_ptr(), pairs.shape[1], rowptr.data_ptr(),
                                              col.data_ptr(), None, None, -1, scratch.data_ptr(), heur.data_ptr(), None,
                                              None, 0) == 0
    for kind in CC.WEIGHT_KINDS:
        ref, mag = CC.reference(name, dim, kind)
        pool, cn = _pool(name, pairs, table, _dev_w(name, kind))
        assert torch.equal(cn, heur) and torch.equal(cn.cpu().to(torch.int64), k)
        got = pool.cpu()
        assert torch.isfinite(got).all()
        assert not got[k == 0].any() and not got[-c.n_bad:].any()                # exactly zero, written
        err, bound = (got.to(torch.float64) - ref).abs(), CC.forward_bound(name, mag)
        live = bound > 0
        ratio = float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0
        print(f"forward {name} D={dim} weights={kind}: worst error / bound = {ratio:.3f}")
        assert (err <= bound).all()


def test_padded_table_and_padded_output_keep_their_padding():
    name, dim = "fan", 36
    pairs = _pairs(name)
    wide = torch.full((CC.case(name).n, dim + 12), 1e30, dtype=torch.float32, device=DEV)
    wide[:, :dim] = CC.table(name, dim).to(DEV)
    plain, _ = _pool(name, pairs, CC.table(name, dim).to(DEV), _dev_w(name, "aa"), thr=8)
    padded, _ = _pool(name, pairs, wide[:, :dim], _dev_w(name, "aa"), thr=8, ldp=dim + 8, fill=-7.0)
    assert torch.equal(padded[:, :dim], plain) and (padded[:, dim:] == -7.0).all()
    assert (wide[:, dim:] == 1e30).all()


@pytest.mark.parametrize("name", CC.NAMES)
def test_integer_sums_are_exact(name):
    pairs, ref = _pairs(name), CC.int_reference(name)
    for thr in (-1, 0, 1 << 30):
        pool, _ = _pool(name, pairs, CC.int_table(name).to(DEV), CC.int_weights(name).to(DEV), thr=thr)
        assert torch.equal(pool.cpu().to(torch.float64), ref), thr


# ---------------------------------------------------------------------------------------------------------- one order
@pytest.mark.parametrize("name,dim", (("C", 128), ("H", 36), ("fan", 128), ("fan", 512)))
def test_every_threshold_gives_the_same_bits(name, dim):
    pairs, table, w = _pairs(name), CC.table(name, dim).to(DEV), _dev_w(name, "tensor")
    first, cn0 = _pool(name, pairs, table, w, thr=CC.THRESHOLDS[0])
    for thr in CC.THRESHOLDS[1:] + (-1,):
        pool, cn = _pool(name, pairs, table, w, thr=thr)
        assert torch.equal(pool, first) and torch.equal(cn, cn0), thr
    again, _ = _pool(name, pairs, table, w, thr=CC.THRESHOLDS[0])                # two runs
    assert torch.equal(again, first)
    swapped, _ = _pool(name, pairs.flip(0).contiguous(), table, w)               # (a, b) against (b, a)
    assert torch.equal(swapped, first)


def test_position_and_chunk_do_not_matter():
    name, dim = "fan", 128
    c, table = CC.case(name), CC.table(name, 128).to(DEV)
    csr = c.csr.to_device(DEV)
    whole, _ = _pool(name, _pairs(name), table, None)
    m = len(CC.fan_facts())
    filler = c.pairs[:, 2 * m:2 * m + 96]
    for j in range(2 * m):                                                       # every named pair, either orientation
        pair = c.pairs[:, j:j + 1]
        for at in (0, 63, 64, 130):
            batch = torch.cat([filler, filler], dim=1)[:, :131].clone()
            batch[:, at] = pair[:, 0]
            for thr in (0, 1 << 30):
                pool, _ = _pool(name, batch.to(DEV).contiguous(), table, None, thr=thr)
                assert torch.equal(pool[at], whole[j]), (j, at, thr)
    P = c.pairs.shape[1]
    for chunk in (1, 64, 65, P):
        pool, cn = ncn.cn_pool(csr, c.pairs, table, chunk=chunk, return_count=True)
        assert torch.equal(pool, whole) and torch.equal(cn.cpu().to(torch.int64), CC.counts(name)), chunk


# ------------------------------------------------------------------------------------------------------------ entries
@pytest.mark.parametrize("name", CC.NAMES)
def test_entries_equal_the_reference_at_every_threshold(name):
    pairs, ent = _pairs(name), CC.entries(name)
    seg, E, guard = ent.seg.to(DEV), ent.node.numel(), 8
    for thr in CC.THRESHOLDS + (-1,):
        buf = _entries(name, pairs, seg, E, thr=thr, guard=guard).cpu()
        assert torch.equal(buf[guard:guard + E], ent.node), thr
        assert (buf[:guard] == -9).all() and (buf[guard + E:] == -9).all(), thr       # the canaries
    got = ncn.cn_entries(CC.case(name).csr.to_device(DEV), CC.case(name).pairs.t())    # [P, 2] in
    assert torch.equal(got.seg.cpu(), ent.seg) and torch.equal(got.node.cpu(), ent.node)
    assert got.node.dtype == torch.int32 and got.seg.dtype == torch.int64


@pytest.mark.parametrize("name", ("C", "fan"))
def test_a_short_seg_writes_inside_its_segments_only(name):
    """Counts that are too small (every pair is granted at most 40 entries, every seventh none), a list shorter than
    the last segments, and offsets beyond it: each pair writes the first entries of C(p) into its own clamped segment
    and nothing else."""
    pairs, ent = _pairs(name), CC.entries(name)
    k = ent.seg[1:] - ent.seg[:-1]
    small = torch.minimum(k, torch.tensor(40))
    small[::7] = 0
    seg = torch.zeros(k.numel() + 1, dtype=torch.int64)
    torch.cumsum(small, 0, out=seg[1:])
    n_ent = int(seg[-1]) - 25                                                    # the last segments run past the list
    for thr in (0, 8, 1 << 30):
        buf = _entries(name, pairs, seg.to(DEV), n_ent, thr=thr).cpu()
        want = torch.full_like(buf, -9)
        for p in np.nonzero(small.numpy())[0]:
            lo, hi = int(seg[p]), min(int(seg[p + 1]), n_ent)
            if hi > lo:
                want[8 + lo:8 + hi] = ent.node[int(ent.seg[p]):int(ent.seg[p]) + hi - lo]
        assert torch.equal(buf, want), thr


# ----------------------------------------------------------------------------------------------------------- backward
def _backward(name, table, kind, g):
    c = CC.case(name)
    t = table.clone().requires_grad_(True)
    w = CC.weights(name, kind) if kind == "tensor" else kind
    pool = ncn.cn_pool(c.csr.to_device(DEV), c.pairs, t, weights=w if isinstance(w, str) else w.to(DEV))
    pool.backward(g)
    return pool.detach(), t.grad


@pytest.mark.parametrize("name", CC.BACKWARD_NAMES)
@pytest.mark.parametrize("dim", (36, 128))
def test_backward_against_the_reference(name, dim):
    c, table = CC.case(name), CC.table(name, dim).to(DEV)
    P = c.pairs.shape[1]
    g = torch.from_numpy(np.random.default_rng(5).standard_normal((P, dim)).astype(np.float32))
    for kind in ("none", "ra", "tensor"):
        pool, dT = _backward(name, table, kind, g.to(DEV))
        assert torch.equal(pool, _pool(name, _pairs(name), table, _dev_w(name, kind))[0])      # the fused forward
        ref, bound, occ = CC.backward_reference(c.n, CC.entries(name), g, CC.weights(name, kind))
        err = (dT.cpu().to(torch.float64) - ref).abs()
        live = bound > 0
        ratio = float((err[live] / bound[live]).max())
        print(f"backward {name} D={dim} weights={kind}: worst error / bound = {ratio:.3f}, "
              f"most occurrences {int(occ.max())}")
        assert (err <= bound).all()
        assert not dT.cpu()[occ == 0].any()                                      # nodes in no C(p): exactly zero
        again = _backward(name, table, kind, g.to(DEV))[1]
        assert torch.equal(again, dT)
    if name == "C2":
        assert int(occ.max()) >= 257                                             # three chunks of 128


def test_backward_is_exact_on_integers():
    name = "C"
    c = CC.case(name)
    g = torch.from_numpy(np.random.default_rng(6).integers(-3, 4, (c.pairs.shape[1], CC.INT_DIM)).astype(np.float32))
    t = CC.int_table(name).to(DEV).requires_grad_(True)
    ncn.cn_pool(c.csr.to_device(DEV), c.pairs, t, weights=CC.int_weights(name).to(DEV)).backward(g.to(DEV))
    ref, _, _ = CC.backward_reference(c.n, CC.entries(name), g, CC.int_weights(name))
    assert float(ref.abs().max()) < 2 ** 24
    assert torch.equal(t.grad.cpu().to(torch.float64), ref)


# --------------------------------------------------------------------------------------------------------- end to end
def test_predictor_trains_on_the_device_and_its_gradient_matches_the_host():
    c = CC.case("C")
    csr_d = c.csr.to_device(DEV)
    pairs, labels = CC.clique_pairs()
    torch.manual_seed(0)
    h0 = 0.1 * torch.randn(c.n, 16)
    model = ncn.NCNPredictor(16, hidden=32).to(DEV)
    bce = torch.nn.functional.binary_cross_entropy_with_logits

    # one step's gradient: the dense part in fp64 on the host gives dloss/dpool; the pooling's share of h.grad for that
    # upstream gradient is held to the backward bound, the whole h.grad to the fp32 dense part's accuracy
    host = copy.deepcopy(model).cpu().double()
    h64 = h0.double().requires_grad_(True)
    pool64 = ncn.cn_pool(c.csr, pairs, h64)
    pool64.retain_grad()
    z = host.mlp_ij(h64[pairs[0]] * h64[pairs[1]]) + host.beta * host.mlp_cn(pool64)
    bce(host.out(z).squeeze(-1), labels.double()).backward()
    g32 = pool64.grad.to(torch.float32)
    ent = ncn.cn_entries_reference(c.csr, pairs)
    ref, bound, _ = CC.backward_reference(c.n, ent, g32, None)
    hd = h0.to(DEV).requires_grad_(True)
    ncn.cn_pool(csr_d, pairs, hd).backward(g32.to(DEV))
    err = (hd.grad.cpu().to(torch.float64) - ref).abs()
    print("h.grad through the pooling: worst error / bound =", round(float((err[bound > 0] / bound[bound > 0]).max()), 3))
    assert (err <= bound).all()
    h = torch.nn.Parameter(h0.to(DEV))
    loss0 = bce(model(csr_d, h, pairs), labels.to(DEV))
    loss0.backward()
    assert float((h.grad.cpu().double() - h64.grad).abs().max()) <= 1e-3 * float(h64.grad.abs().max())
    assert all(p.grad is not None and bool(p.grad.abs().sum() > 0) for p in model.parameters())

    opt = torch.optim.Adam(list(model.parameters()) + [h], lr=0.01)
    for _ in range(30):
        opt.zero_grad()
        loss = bce(model(csr_d, h, pairs), labels.to(DEV))
        loss.backward()
        opt.step()
    scores = ncn.ncn_scores(csr_d, model, h.detach(), pairs, chunk=50)
    assert scores.shape == (pairs.shape[1],) and scores.is_cuda
    assert torch.allclose(scores, model(csr_d, h, pairs).detach(), atol=1e-5)
    print("loss", float(loss0.detach()), "->", float(loss.detach()))
    assert float(loss.detach()) < float(loss0.detach())
    assert float(scores[labels.to(DEV) == 1].mean()) > float(scores[labels.to(DEV) == 0].mean())


def test_a_model_source_pools_over_its_typing_adjacency():
    cfg = D.CONFIGS["tiny"]
    n = cfg["n"]
    ei, _ = D.chung_lu_graph(n, cfg["edges"], seed=1)
    x = np.random.default_rng(0).standard_normal((n, cfg["f_in"])).astype(np.float32)
    data = D.link_split(ei, x, n, eps=cfg["eps"], seed=2)
    torch.manual_seed(0)
    model = lpformer_amd.LinkTransformer(D.train_args_for(cfg), data, device=DEV).to(DEV).eval()
    h = model.propagate()
    assert h.shape[1] % 4 == 0
    edges = data["test_pos"][:300]
    for test_set, key in ((False, "adj_mask"), (True, "full_adj_mask")):
        pool, cn = ncn.cn_pool(model, edges, h, weights="ra", test_set=test_set, return_count=True)
        w = ncn._host_weights(data[key], "ra")
        ref = ncn.cn_pool_reference(data[key], edges, h, w)
        mag = ncn.cn_pool_reference(data[key], edges, h.abs(), w)
        k = cn.cpu().to(torch.float64)
        bound = 1.01 * CC.U24 * (torch.minimum(k, torch.tensor(64.0)) + torch.ceil(k / 64) + 1)[:, None] * mag
        assert ((pool.cpu().to(torch.float64) - ref).abs() <= bound).all() and int(cn.sum()) > 0
        assert torch.equal(k.to(torch.int64), ncn.cn_entries_reference(data[key], edges).seg.diff())


# ---------------------------------------------------------------------------------------------------- argument checks
def test_c_entries_reject_bad_arguments_without_a_launch():
    name, dim = "fan", 36
    c, pairs, table = CC.case(name), _pairs(name), CC.table(name, dim).to(DEV)
    rowptr, col = _graph(name)
    hip = _lib.hip()
    P, n = pairs.shape[1], c.n
    w = torch.ones(n, dtype=torch.float32, device=DEV)
    pool = torch.full((P, dim), -7.0, dtype=torch.float32, device=DEV)
    cn = torch.full((P,), -7, dtype=torch.int32, device=DEV)
    scratch = torch.full((P + 1,), -7, dtype=torch.int32, device=DEV)
    ent = CC.entries(name)
    seg, E = ent.seg.to(DEV), ent.node.numel()
    node = torch.full((E,), -7, dtype=torch.int32, device=DEV)
    pp, rp, cp, wp, tp, sp, op, kp, gp, np_ = (t.data_ptr() for t in (pairs, rowptr, col, w, table, scratch, pool, cn,
                                                                      seg, node))

    def pool_call(P=P, n=n, pp=pp, ld=P, rp=rp, cp=cp, wp=wp, dim=dim, tp=tp, ldt=dim, thr=-1, sp=sp, op=op, ldp=dim,
                  kp=kp):
        return hip.lpf_cn_pool_f32(P, n, pp, ld, rp, cp, wp, dim, tp, ldt, thr, sp, op, ldp, kp, 0)
    for bad in (dict(P=-1), dict(P=(1 << 31) - 1), dict(n=0), dict(n=-1), dict(n=1 << 31), dict(pp=None),
                dict(ld=P - 1), dict(rp=None), dict(cp=None), dict(dim=0), dict(dim=34), dict(dim=516), dict(dim=-4),
                dict(tp=None), dict(tp=tp + 4), dict(ldt=dim - 4), dict(ldt=dim + 2), dict(sp=None), dict(op=None),
                dict(op=op + 4), dict(ldp=dim - 4), dict(ldp=dim + 2)):
        assert pool_call(**bad) == -1, bad
    assert pool_call(P=0) == 0 and pool_call(P=0, pp=None, rp=None, cp=None, tp=None, sp=None, op=None, dim=7) == 0

    def ent_call(P=P, n=n, pp=pp, ld=P, rp=rp, cp=cp, thr=-1, sp=sp, gp=gp, E=E, np_=np_):
        return hip.lpf_cn_entries(P, n, pp, ld, rp, cp, thr, sp, gp, E, np_, 0)
    for bad in (dict(P=-1), dict(P=(1 << 31) - 1), dict(n=0), dict(n=1 << 31), dict(pp=None), dict(ld=P - 1),
                dict(rp=None), dict(cp=None), dict(sp=None), dict(gp=None), dict(E=-1), dict(E=(1 << 31) - 1),
                dict(np_=None)):
        assert ent_call(**bad) == -1, bad
    assert ent_call(P=0) == 0 and ent_call(P=0, pp=None, rp=None, cp=None, sp=None, gp=None, np_=None) == 0
    assert ent_call(E=0, np_=None) == 0
    torch.cuda.synchronize()
    for t in (pool, cn, scratch, node):
        assert (t == -7).all()                                                   # nothing ran
