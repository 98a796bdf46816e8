"""The set-up of ``pair_rows_kernel`` in its PT form at its edges: ``lpf_pair_attention_rows4_f32`` driven directly, at
D = 128, on synthetic ``pair_tab`` / ``blk_cnt`` / ``entries`` (tests/rows_setup_cases.py: ranges that start on lane 0 and
on lane 63 of a block, empty ranges beside a hub pair, a batch smaller than the grid, ranges of more than one chunk, table
entries that point outside the buffer), with a real model's folded tables, pattern tables, node keys and random queries.

Every case fills ``out`` with a sentinel and checks: every pair with entries has its row written and its count
features right; the rows agree with the fp64 restatement (tests/f32_error_model.py ``attention``) within the bound
tests/test_gpu_f32_reference.py holds this kernel to, C_ATT["rows"][128] x b_post; rows of pairs without entries are
untouched (the form with an order for the tail never writes them); ``perm`` is the pairs with entries in ascending order,
then -- from the back -- the others; ``n_nonempty`` is their number.
"""
import numpy as np
import pytest
import torch

from lpformer_amd import _lib
from lpformer_amd._lib import check, ptr
from tests import f32_error_model as E
from tests import rows_setup_cases as C
from tests.scoring_harness import DEV, _np, _setup
from tests.test_gpu_f32_reference import C_ATT

pytestmark = pytest.mark.gpu

D = 128
N_COUNTS = 4
LDO = D + N_COUNTS
SENTINEL = 12345.0
_ctx = {}


def _model():
    """Folded tables, pattern tables and node keys of one random-init model (built once, left unchanged)."""
    if not _ctx:
        model, _, _, _ = _setup(D, "all", seed=5)
        h = model.propagate()
        model._fold_memo = None
        w = model._fold()
        z = model._node_keys(h, w)
        pt = model._pattern_tables(w)
        layer = model.att_layers[0]
        torch.cuda.synchronize()
        _ctx.update(model=model, h=h, w=w, z=z, pt=pt, layer=layer,
                    w_np={k: _np(v) for k, v in w.items() if k in ("wfold", "bfold", "att", "pe_tab", "pe_stat")},
                    z_np=_np(z), att_bias=_np(layer.att.bias),
                    ln=(_np(layer.post_att_norm.weight), _np(layer.post_att_norm.bias)),
                    n_cu=_lib.device_info()["cu_count"])
    return _ctx


def _grid(bs):
    return C.grid_size(bs, _model()["n_cu"], _lib.ROWS_PERM_LB_WORDS - 1)


def _selection(counts3, rng, n_nodes, corrupt=None):
    """pair_tab / blk_cnt / entries of a batch whose pair p selects counts3[p] = (cn, one-hop, further) nodes, pair-major as
    select4 leaves them.  ``corrupt``: {pair: int4} table entries written over the consistent ones; those pairs count as
    empty everywhere else (``blk_cnt`` included)."""
    counts3 = np.asarray(counts3, np.int64)
    bs = counts3.shape[0]
    cnt = counts3.sum(axis=1)
    start = np.cumsum(cnt) - cnt
    n_ent = int(cnt.sum())
    ent_cap = n_ent + 8
    pair = np.repeat(np.arange(bs), cnt)
    j = np.arange(n_ent) - start[pair]
    typ = (j >= counts3[pair, 0]).astype(np.int64) + (j >= counts3[pair, 0] + counts3[pair, 1])
    node = rng.integers(0, n_nodes, n_ent)
    pa = np.exp(rng.uniform(np.log(1e-4), np.log(0.6), n_ent)).astype(np.float32)
    pb = np.exp(rng.uniform(np.log(1e-4), np.log(0.6), n_ent)).astype(np.float32)
    ent = np.zeros((ent_cap, 4), np.int32)
    ent[:n_ent, 0] = (pair | ((typ + 1) << 29)).astype(np.uint32).view(np.int32)
    ent[:n_ent, 1] = node
    ent[:n_ent, 2] = pa.view(np.int32)
    ent[:n_ent, 3] = pb.view(np.int32)
    tab = np.concatenate([start[:, None], counts3], axis=1).astype(np.int32)
    valid = cnt.copy()
    for p, rec in (corrupt or {}).items():
        tab[p] = rec
        valid[p] = 0
    nblk = (bs + C.SB - 1) // C.SB
    pad = np.zeros(nblk * C.SB, np.int64)
    pad[:bs] = valid
    blk = np.stack([pad.reshape(nblk, C.SB).sum(axis=1), (pad.reshape(nblk, C.SB) > 0).sum(axis=1)], axis=1).astype(np.int32)
    keep = valid[pair] > 0
    sel = [(np.stack([pair[keep & (typ == t)], node[keep & (typ == t)]]), pa[keep & (typ == t)], pb[keep & (typ == t)])
           for t in range(3)]
    return {"tab": tab, "blk": blk, "ent": ent, "ent_cap": ent_cap, "valid": valid, "sel": sel, "counts3": counts3}


def _launch(s, q, sel_err=0):
    m = _model()
    lib, w, pt, layer, z = _lib.hip(), m["w"], m["pt"], m["layer"], m["z"]
    bs = s["tab"].shape[0]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    tab, blk, ent = dev(s["tab"]), dev(s["blk"]), dev(s["ent"])
    ctl = torch.zeros(8, dtype=torch.int64, device=DEV)
    ctl[3] = sel_err
    units_cap = (s["ent_cap"] + 15) // 16 + 1
    pieces = torch.empty(units_cap * 2 * int(lib.lpf_pair_rows_piece_floats(D)), dtype=torch.float32, device=DEV)
    out = torch.full((bs, LDO), SENTINEL, dtype=torch.float32, device=DEV)
    perm = torch.full((bs,), -1, dtype=torch.int32, device=DEV)
    nfull = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    geo = pt["geo"]
    st = torch.cuda.current_stream().cuda_stream
    check(lib.lpf_pair_attention_rows4_f32(
        D, bs, ptr(tab), ptr(blk), ptr(ent), s["ent_cap"], ptr(z), z.stride(0), ptr(q), q.stride(0), ptr(w["flip_tab"]),
        ptr(w["pe_stat"]), ptr(pt["base"]), ptr(pt["grid"]), ptr(pt["sign"]), geo["n"], geo["shift"], geo["base"], geo["ofs"],
        ptr(w["wfold_t"]), ptr(w["att"]), ptr(layer.att.bias), ptr(layer.post_att_norm.weight),
        ptr(layer.post_att_norm.bias), N_COUNTS, ptr(ctl), ptr(pieces), units_cap, ptr(out), out.stride(0), ptr(perm),
        ptr(nfull), st), "lpf_pair_attention_rows4_f32")
    torch.cuda.synchronize()
    return out, perm.cpu().numpy(), int(nfull.item())


def _run(name, counts, seed=0, corrupt=None, sel_err=0):
    """One launch on a batch whose pair p has counts[p] entries, checked as the module docstring says."""
    m = _model()
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, np.int64)
    bs = counts.size
    s = _selection(C.split3(counts, rng), rng, m["z_np"].shape[0], corrupt)
    ne = np.flatnonzero(s["valid"] > 0)
    empty = np.flatnonzero(s["valid"] == 0)
    # queries: rows of the pairs with entries only (the kernel fetches no other)
    q_ne = rng.standard_normal((ne.size, D)).astype(np.float32)
    q = torch.zeros((bs, D), dtype=torch.float32, device=DEV)
    if ne.size:
        q[torch.from_numpy(ne).to(DEV)] = torch.from_numpy(q_ne).to(DEV)
    out, perm, nfull = _launch(s, q, sel_err)
    # the order for the tail
    assert nfull == ne.size, (name, nfull, ne.size)
    assert np.array_equal(perm[:ne.size], ne), name
    assert np.array_equal(perm[ne.size:][::-1], empty), name
    # pairs without entries: nothing written
    if empty.size:
        assert bool((out[torch.from_numpy(empty).to(DEV)] == SENTINEL).all()), name
    if not ne.size:
        return
    got = out[torch.from_numpy(ne).to(DEV)].cpu().numpy()
    assert np.array_equal(got[:, D:], np.stack([s["counts3"][ne, 0], s["counts3"][ne, 1], s["counts3"][ne, 2],
                                                s["counts3"][ne, 0] + s["counts3"][ne, 1]], axis=1)), name
    if sel_err:
        assert np.isnan(got[:, :D]).all(), name
        return
    assert not (got[:, :D] == SENTINEL).any(), name
    # fp64 restatement on the pairs with entries, renumbered (a pair's row depends on its own entries and query only)
    new_id = np.full(bs, -1, np.int64)
    new_id[ne] = np.arange(ne.size)
    sel = [(np.stack([new_id[ix[0]], ix[1]]), pa, pb) if ix.shape[1] else None for ix, pa, pb in s["sel"]]
    ref = E.attention(sel, m["z_np"], q_ne, m["w_np"], m["att_bias"], *m["ln"], ne.size)
    bnd = E.attention_bound(ref, m["z_np"], m["w_np"], q_ne, m["att_bias"], *m["ln"])
    err = np.abs(got[:, :D].astype(np.float64) - ref["post"])
    worst = float((err / bnd["b_post"]).max())
    print(f"{name}: {bs} pairs, {ne.size} with entries, {int(s['valid'].sum())} entries, grid {_grid(bs)}: "
          f"max |got - ref| {err.max():.3e}, worst err / bound(C = 1) {worst:.3f}")
    assert np.isfinite(got).all() and worst <= C_ATT["rows"][D], (name, worst)


@pytest.mark.parametrize("bs", [1, 63, 64, 65, 130])
def test_small_batches(bs):
    """A last block that is partial, a batch smaller than the grid (ranges of target 0, workgroups without pairs)."""
    _run(f"bs {bs}", C.random_counts(bs, np.random.default_rng(bs), empty=0.4, top=40) if bs > 1 else np.array([9]), seed=bs)
    _run(f"bs {bs}, sparse", C.random_counts(bs, np.random.default_rng(bs + 7), empty=0.9, top=3), seed=bs + 1)


@pytest.mark.parametrize("bs", [1, 130, 1000])
def test_all_pairs_empty(bs):
    _run(f"empty {bs}", np.zeros(bs, np.int64))


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("n", [1, 16, 17, 700])
def test_one_pair_with_entries(where, n):
    _run(f"one pair ({where} block, {n} entries)", C.one_pair(1000, where, n), seed=n)


def test_range_ends_on_lane_0_and_lane_63():
    bs = 3000
    grid = _grid(bs)
    counts, b0, b63 = C.lane_edges(grid, bs)
    p = C.range_starts(counts, grid)           # (the kernel's integer formula; pinned in tests/test_rows_setup_host.py)
    assert p[b0] % C.SB == 0 and p[b63] % C.SB == C.SB - 1
    _run("lane edges", counts, seed=1)


def test_hub_pair_beside_empty_ranges():
    bs = 2000
    grid = _grid(bs)
    counts, hp = C.hub(grid, bs)
    f = C.range_facts(counts, grid)
    b = int(f["wg"][np.flatnonzero(f["nonempty"] == hp)[0]])
    assert (f["len"][b + 1:b + 10] == 0).all() and counts[hp] > 64 * C.UNIT
    _run("hub", counts, seed=2)


def test_range_longer_than_a_chunk():
    """>= 140,000 pairs on a 256-CU device, almost all of them empty: the second chunk of a range goes through the chunk
    loop's own staging, the first one is cut at PR_CHUNK pairs."""
    grid = _model()["n_cu"]
    counts = C.long_ranges(grid)
    assert _grid(counts.size) == grid
    f = C.range_facts(counts, grid)
    long_ = f["len"] > C.PR_CHUNK
    second, first = long_[f["wg"]] & (f["ofs"] >= C.PR_CHUNK), long_[f["wg"]] & (f["ofs"] < C.PR_CHUNK)
    assert second.sum() >= 8 and len(set(f["wg"][second]) & set(f["wg"][first])) >= 4
    _run("long ranges", counts, seed=3)


def test_table_entries_outside_the_buffer_count_as_empty():
    bs = 500
    rng = np.random.default_rng(11)
    counts = C.random_counts(bs, rng, empty=0.3, top=30)
    where = [3, 64, 70, 127, 128, 300, 499]
    counts[where] = np.maximum(counts[where], 1)   # (their entries exist: it is the table that points elsewhere)
    total = int(counts.sum())                      # ent_cap = total + 8
    bad = {3: (total + 8 - 2, 2, 2, 1),            # ends behind ent_cap
           64: (-5, 1, 1, 1),                      # negative start
           70: (0, -1, 3, 0),                      # negative fields
           127: (10, 2, -2147483648, 1),
           128: (2147483000, 400, 300, 0),         # start + count beyond 2^31
           300: (0, 1, 2, -7),
           499: (total + 8, 1, 0, 0)}
    assert sorted(bad) == where
    _run("corrupt table entries", counts, seed=4, corrupt=bad)


def test_selection_error_gives_nan_rows():
    _run("sel_ctl[3] != 0", C.random_counts(130, np.random.default_rng(5)), seed=5, sel_err=1)
