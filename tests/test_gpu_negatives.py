"""negative_rows / negative_pairs (lpf_negative_rows, lpf_negative_pairs: csrc/neg_sample.hip) on the MI355X against the
numpy restatement of the written definition (``negatives_reference``; tests/test_negatives_host.py pins it on its own).
Every comparison is exact integer equality."""
import numpy as np
import pytest
import torch

import lpformer_amd
from lpformer_amd import _lib, data as D, negatives as N
from tests import negatives_cases as NC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.array(a, dtype=np.int64))


@pytest.fixture(scope="module")
def graphs():
    return {name: NC.case(name).csr.to_device(DEV) for name in ("S", "H", "C")}


def _rows(g, name, k, **kw):
    src = _t(NC.rows_for(name, k)).to(DEV)
    out = lpformer_amd.negative_rows(g, src, k, seed=NC.SEED, check=False, **kw)
    assert out.is_cuda and out.dtype == torch.int64 and out.shape == (src.numel(), k)
    return out


# ------------------------------------------------------------------------------------------------------------ rows
@pytest.mark.parametrize("name,k", [("S", 1), ("S", 63), ("S", 64), ("S", 65), ("H", 500), ("H", 1024), ("C", 3)])
def test_rows_match_the_restatement(graphs, name, k):
    want, short = NC.ref_rows(name, k)
    got = _rows(graphs[name], name, k)
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(got, _rows(graphs[name], name, k))                # two runs
    src = _t(NC.rows_for(name, k)).to(DEV)
    if short:
        with pytest.raises(ValueError, match=f"{short} of {src.numel()} rows"):
            lpformer_amd.negative_rows(graphs[name], src, k, seed=NC.SEED)
    else:
        assert torch.equal(lpformer_amd.negative_rows(graphs[name], src, k, seed=NC.SEED), got)
    if name == "C":
        assert (got == -1).all() and short == src.numel()


def test_rows_invariances(graphs):
    c, g = NC.case("S"), graphs["S"]
    full = _rows(g, "S", 65)
    src = _t(c.sources).to(DEV)
    # rows [lo, hi) with row_base = lo; single rows in another order
    assert torch.equal(lpformer_amd.negative_rows(g, src[9:], 65, seed=NC.SEED, check=False, row_base=9), full[9:])
    for r in np.random.default_rng(3).permutation(src.numel())[:8].tolist():
        one = lpformer_amd.negative_rows(g, src[r:r + 1], 65, seed=NC.SEED, check=False, row_base=r)
        assert torch.equal(one[0], full[r])
    assert torch.equal(_rows(g, "S", 63), full[:, :63])                  # the prefix
    # host CSR (uploaded), CPU sources, [R, k, 2]
    pairs = lpformer_amd.negative_rows(c.csr, _t(c.sources), 65, seed=NC.SEED, check=False, as_pairs=True)
    assert pairs.is_cuda and pairs.shape == (src.numel(), 65, 2)
    assert torch.equal(pairs[..., 1], full) and torch.equal(pairs[..., 0], src[:, None].expand(-1, 65))
    # exclude=, as [2, E] on the host, [E, 2] on the device and as a CSR
    want, _ = NC.ref_rows("S", 63, exclude=True)
    for ex in (_t(c.held), _t(c.held.T).to(DEV), lpformer_amd.graph.mask_csr(c.held, c.n, symmetric=False)):
        got = lpformer_amd.negative_rows(g, src, 63, seed=NC.SEED, check=False, exclude=ex)
        assert np.array_equal(got.cpu().numpy(), want)
    # max_draws: one round
    want = N.negatives_reference(c.csr, c.sources, 65, seed=NC.SEED, max_draws=64)
    assert torch.equal(lpformer_amd.negative_rows(g, src, 65, seed=NC.SEED, check=False, max_draws=64).cpu(), want)


# ----------------------------------------------------------------------------------------------------------- pairs
@pytest.mark.parametrize("name", ["S", "H", "C"])
@pytest.mark.parametrize("m", NC.PAIR_MS)
def test_pairs_match_the_restatement(graphs, name, m):
    g = graphs[name]
    for unique, rounds in ((False, 8), (True, 1), (True, 8)):
        want, short = NC.ref_pairs(name, m, unique, rounds)
        got = lpformer_amd.negative_pairs(g, m, seed=NC.SEED, unique=unique, rounds=rounds, check=False)
        assert got.is_cuda and got.dtype == torch.int64 and got.shape == (2, m)
        assert np.array_equal(got.cpu().numpy(), want), (unique, rounds)
        assert torch.equal(got, lpformer_amd.negative_pairs(g, m, seed=NC.SEED, unique=unique, rounds=rounds, check=False))
        if short:
            with pytest.raises(ValueError, match=f"{short} of {m} pairs"):
                lpformer_amd.negative_pairs(g, m, seed=NC.SEED, unique=unique, rounds=rounds)
        else:
            assert torch.equal(lpformer_amd.negative_pairs(g, m, seed=NC.SEED, unique=unique, rounds=rounds), got)
    if name == "C":
        assert (got == -1).all()


def test_pairs_exclude_and_slots(graphs):
    c, g = NC.case("S"), graphs["S"]
    want, _ = NC.ref_pairs("S", 1000, True, 8, exclude=True)
    got = lpformer_amd.negative_pairs(g, 1000, seed=NC.SEED, exclude=_t(c.held).to(DEV), check=False)
    assert np.array_equal(got.cpu().numpy(), want)
    plain, _ = NC.ref_pairs("S", 1000, False)
    part = lpformer_amd.negative_pairs(c.csr, 300, seed=NC.SEED, unique=False, slot_base=700)
    assert part.is_cuda and np.array_equal(part.cpu().numpy(), plain[:, 700:])


def test_pairs_active_mask_and_next_two_calls_equal_one(graphs):
    """The C entry itself: a first call that may draw once, then a second call over the slots it left at (-1, -1),
    which continue at their ``next``, equals one call."""
    g, m = graphs["S"], 1000
    hip = _lib.hip()
    want, _ = NC.ref_pairs("S", m, False)
    pairs = torch.full((2, m), -7, dtype=torch.int64, device=DEV)
    nxt = torch.zeros(m, dtype=torch.int32, device=DEV)
    lost = torch.full((1,), 99, dtype=torch.int64, device=DEV)

    def call(max_draws, active):
        return hip.lpf_negative_pairs(m, g.n, g.rowptr.data_ptr(), g.col.data_ptr(), NC.SEED, 0, max_draws,
                                      None if active is None else active.data_ptr(), nxt.data_ptr(), pairs.data_ptr(),
                                      m, lost.data_ptr(), 0)
    assert call(1, None) == 0
    torch.cuda.synchronize()
    first = pairs.clone()
    open_ = first[0] < 0
    n_open = int(open_.sum())
    assert 0 < n_open < 400 and int(lost) == n_open
    assert torch.equal(nxt, torch.ones_like(nxt))                        # accepted at draw 0 or stopped at max_draws = 1
    assert np.array_equal(first[:, ~open_].cpu().numpy(), want[:, (~open_).cpu().numpy()])
    active = open_.to(torch.uint8)
    assert call(N.PAIR_DRAWS, active) == 0
    torch.cuda.synchronize()
    assert np.array_equal(pairs.cpu().numpy(), want) and int(lost) == 0
    assert torch.equal(pairs[:, ~open_], first[:, ~open_])               # the inactive slots were not touched
    # bad options are refused without a launch
    assert call(0, None) == -1 and hip.lpf_negative_pairs(m, g.n, g.rowptr.data_ptr(), g.col.data_ptr(), 0, 0, 4, None,
                                                          nxt.data_ptr(), pairs.data_ptr(), m - 1, lost.data_ptr(), 0) == -1
    src = torch.zeros(4, dtype=torch.int64, device=DEV)
    out = torch.full((4, 8), -7, dtype=torch.int64, device=DEV)
    for k in (0, 1025):
        assert hip.lpf_negative_rows(4, g.n, src.data_ptr(), k, g.rowptr.data_ptr(), g.col.data_ptr(), 0, 0, 64,
                                     out.data_ptr(), lost.data_ptr(), 0) == -1
    torch.cuda.synchronize()
    assert (out == -7).all()


def test_check_false_reads_nothing_back(graphs):
    """With ``check=False`` no call may synchronise: torch's sync debug mode turns the read-backs it knows of (``item``,
    ``nonzero``, boolean indexing, copies to the host) into errors; the kernels' own entry points only enqueue."""
    c, g = NC.case("S"), graphs["S"]
    src = _t(c.sources).to(DEV)
    held = _t(c.held).to(DEV)
    lpformer_amd.negative_pairs(g, 8, seed=1, exclude=held, check=False)  # (the union with ``exclude`` is built once)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        rows = lpformer_amd.negative_rows(g, src, 63, seed=NC.SEED, check=False)
        pairs = lpformer_amd.negative_pairs(g, 1000, seed=NC.SEED, check=False)
        ex = lpformer_amd.negative_pairs(g, 1000, seed=NC.SEED, exclude=held, check=False)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.array_equal(rows.cpu().numpy(), NC.ref_rows("S", 63)[0])
    assert np.array_equal(pairs.cpu().numpy(), NC.ref_pairs("S", 1000, True, 8)[0])
    assert np.array_equal(ex.cpu().numpy(), NC.ref_pairs("S", 1000, True, 8, exclude=True)[0])


# ------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def tiny():
    cfg = D.CONFIGS["tiny"]
    n = cfg["n"]
    ei, _ = D.chung_lu_graph(n, cfg["edges"], seed=1)
    x = np.random.default_rng(0).standard_normal((n, cfg["f_in"])).astype(np.float32)
    data = D.link_split(ei, x, n, eps=cfg["eps"], seed=2)
    torch.manual_seed(0)
    model = lpformer_amd.LinkTransformer(D.train_args_for(cfg), data, device=DEV).to(DEV)
    score = lpformer_amd.mlp_score(model.out_dim, model.out_dim, 1, 2).to(DEV)
    return n, data, model, score


def test_sources_agree(tiny):
    n, data, model, _ = tiny
    csr = data["adj_mask"]
    src = torch.randint(0, n, (200,), generator=torch.Generator().manual_seed(1))
    want = N.negatives_reference(csr, src, 40, seed=7)
    for source in (csr, csr.to_device(DEV), model):
        assert torch.equal(lpformer_amd.negative_rows(source, src, 40, seed=7).cpu(), want)
    want = N.negatives_reference(csr, num=2000, seed=7)
    for source in (csr, csr.to_device(DEV), model):
        assert torch.equal(lpformer_amd.negative_pairs(source, 2000, seed=7).cpu(), want)
    # link_split drew its negatives on the device here: the same dict as the restatement gives
    both = np.concatenate([data[k].numpy() for k in ("train_pos", "valid_pos", "test_pos")]).T
    known = lpformer_amd.graph.mask_csr(both, n, symmetric=True)
    m_val = data["valid_neg"].shape[0]
    ref = N.negatives_reference(known, num=m_val + data["test_neg"].shape[0], seed=2).t()
    assert torch.equal(data["valid_neg"], ref[:m_val]) and torch.equal(data["test_neg"], ref[m_val:])


def test_uniform_negatives_and_fit(tiny):
    n, data, model, score = tiny
    keys = torch.from_numpy(NC.edge_keys(data["adj_mask"])).to(DEV)
    edges = data["train_pos"][:512].t().to(DEV)
    for mode, k in (("pairs", 1), ("tail", 3)):
        draw = lpformer_amd.UniformNegatives(model, seed=1, mode=mode, num_negative=k)
        steps = [draw(s, edges) for s in range(3)]
        for neg in steps:
            assert neg.is_cuda and neg.dtype == torch.int64 and neg.shape == (2, 512 * k)
            assert int(neg.min()) >= 0 and int(neg.max()) < n and (neg[0] != neg[1]).all()
            assert not torch.isin(neg[0] * n + neg[1], keys).any() and not torch.isin(neg[1] * n + neg[0], keys).any()
        assert not torch.equal(steps[0], steps[1]) and not torch.equal(steps[1], steps[2])
        if mode == "tail":
            assert torch.equal(steps[0][0], edges[0].repeat_interleave(k))
        again = lpformer_amd.UniformNegatives(model, seed=1, mode=mode, num_negative=k)
        assert torch.equal(again(0, edges), steps[0])
        assert not torch.equal(draw(0, edges), steps[0]) and draw.epoch == 1     # the next epoch draws afresh
    opt = torch.optim.Adam(list(model.parameters()) + list(score.parameters()), lr=5e-3)
    out = lpformer_amd.fit(model, score, data, opt, epochs=2, eval_steps=1, batch_size=4096,
                           negatives=lpformer_amd.UniformNegatives(model, seed=1))
    assert len(out["history"]) == 2
    for entry in out["history"]:
        assert np.isfinite(entry["loss"])
        for name, triple in entry["results"].items():
            if name.startswith("nan"):
                assert all(int(v) == 0 for v in triple), (name, triple)
            else:
                assert all(0.0 <= float(v) <= 1.0 for v in triple), (name, triple)
