"""Edge-aware negative sampling without a GPU: the bindings, the fixed definition of the draw, the properties of the
numpy restatement (``negatives_reference``, what the kernels are compared with on the device) and ``link_split``."""
import random

import numpy as np
import pytest
import torch

import lpformer_amd
from lpformer_amd import _lib, data as D, graph, negatives as N
from tests import negatives_cases as NC


# ------------------------------------------------------------------------------------------------------- bindings
def test_bindings():
    assert _lib.ABI_VERSION == 16
    assert "lpf_negative_rows" in _lib.HIP_PROTOTYPES and "lpf_negative_pairs" in _lib.HIP_PROTOTYPES
    assert len(_lib.HIP_PROTOTYPES["lpf_negative_rows"]) == 12 and len(_lib.HIP_PROTOTYPES["lpf_negative_pairs"]) == 13
    hip = _lib.hip()
    assert hasattr(hip, "lpf_negative_rows") and hasattr(hip, "lpf_negative_pairs")
    for name in ("negative_rows", "negative_pairs", "UniformNegatives", "negatives_reference", "link_split"):
        assert name in lpformer_amd.__all__ and hasattr(lpformer_amd, name)


# ------------------------------------------------------------------------------------------------------- the draw
def _chi2(counts, expected):
    return float(((counts - expected) ** 2 / expected).sum())


def test_node_draw_is_uniform():
    """Seed 0, n = 97, slots 0 .. 4095 x draws 0 .. 7: chi^2 on 96 degrees of freedom below dof + 4 sqrt(2 dof) = 151.4
    (measured: 94.1).  A condition on the fixed definition, not on a kernel."""
    n = 97
    key = N.draw_key(0, np.arange(4096, dtype=np.uint64))
    c = N.draw_node(N.draw_u(key[:, None], np.arange(8, dtype=np.uint64)[None, :]), n).ravel()
    assert c.min() >= 0 and c.max() < n
    chi2, dof = _chi2(np.bincount(c, minlength=n), c.size / n), n - 1
    print(f"node draw: chi2 = {chi2:.1f} on {dof} dof")
    assert chi2 < dof + 4 * np.sqrt(2 * dof)


def test_pair_draw_is_uniform():
    """The first pair draw of 200,000 slots over 97^2 cells: chi^2 on 9,408 dof below 9,956.7 (measured: 9,205.8)."""
    n = 97
    key = N.draw_key(0, np.arange(200_000, dtype=np.uint64))
    a, b = N.draw_node(N.draw_u(key, 0), n), N.draw_node(N.draw_u(key, 1), n)
    chi2, dof = _chi2(np.bincount(a * n + b, minlength=n * n), a.size / (n * n)), n * n - 1
    print(f"pair draw: chi2 = {chi2:.1f} on {dof} dof")
    assert chi2 < dof + 4 * np.sqrt(2 * dof)


def test_draw_against_python_integers():
    rng = random.Random(5)
    m64 = (1 << 64) - 1
    for _ in range(1000):
        u, n = rng.getrandbits(64), rng.randrange(1, 1 << 31)
        assert int(N.draw_node(u, n)[0]) == (u * n) >> 64
    assert int(N.draw_node(m64, (1 << 31) - 1)[0]) == (m64 * ((1 << 31) - 1)) >> 64
    g = 0x9E3779B97F4A7C15

    def mix(z):
        z &= m64
        z ^= z >> 30
        z = z * 0xBF58476D1CE4E5B9 & m64
        z ^= z >> 27
        z = z * 0x94D049BB133111EB & m64
        return z ^ (z >> 31)
    for _ in range(200):
        seed, i, j = rng.getrandbits(64), rng.getrandbits(40), rng.getrandbits(20)
        key = mix(seed + g * (i + 1))
        assert int(N.draw_key(seed, i)[0]) == key == N.step_seed(seed, i)
        assert int(N.draw_u(key, j)[0]) == mix(key + g * (j + 1))
    assert N.mix64(0) == 0 and N.mix64(1) == mix(1) != 1


# ------------------------------------------------------------------------------------------- the restatement: rows
@pytest.mark.parametrize("name,k", [("S", 1), ("S", 63), ("S", 64), ("S", 65), ("H", 500), ("H", 1024), ("C", 3)])
def test_rows_properties(name, k):
    c = NC.case(name)
    src = NC.rows_for(name, k)
    rows, short = NC.ref_rows(name, k)
    assert rows.shape == (src.size, k) and rows.dtype == np.int64
    NC.check_rows(c.csr, src, rows)
    # exactly min(k, avail) targets, then -1, and the counter
    deg = np.diff(c.csr.rowptr)
    want = []
    for s in src.tolist():
        if not 0 <= s < c.n:
            want.append(0)
        else:
            has_self = s in c.csr.col[c.csr.rowptr[s]:c.csr.rowptr[s + 1]]
            want.append(min(k, c.n - deg[s] - (0 if has_self else 1)))
    assert ((rows >= 0).sum(axis=1) == np.array(want)).all()
    assert short == int((np.array(want) < k).sum())
    if name == "C":
        assert (rows == -1).all() and short == src.size


def test_rows_exact_and_short_availability():
    """S: node 1 / 4 / 5 have avail = 65 / 64 / 63 exactly, node 0 has 29."""
    c = NC.case("S")
    for k, node in ((65, 1), (64, 4), (63, 5)):
        rows, _ = NC.ref_rows("S", k)
        r = int(np.flatnonzero(c.sources == node)[0])
        assert (rows[r] >= 0).all()
        full = set(range(c.n)) - {node} - set(c.csr.col[c.csr.rowptr[node]:c.csr.rowptr[node + 1]].tolist())
        assert set(rows[r].tolist()) == full                            # every free target, each once
        assert (rows[0] >= 0).sum() == 29 and (rows[0, 29:] == -1).all()


def test_rows_prefix_independence_and_repeats():
    c = NC.case("S")
    r65, _ = NC.ref_rows("S", 65)
    for k in (1, 63, 64):
        assert np.array_equal(NC.ref_rows("S", k)[0], r65[:, :k])       # the k'-prefix is the row for k'
    # a row depends on its slot only: the rows one at a time, in another order, with row_base bookkeeping
    perm = np.random.default_rng(3).permutation(c.sources.size)
    for r in perm[:12].tolist():
        one = N.negatives_reference(c.csr, c.sources[r:r + 1], 65, seed=NC.SEED, row_base=r)
        assert np.array_equal(one.numpy()[0], r65[r])
    lo = 9
    part = N.negatives_reference(c.csr, c.sources[lo:], 65, seed=NC.SEED, row_base=lo)
    assert np.array_equal(part.numpy(), r65[lo:])
    # the same source in three rows: three different rows
    at = np.flatnonzero(c.sources == 7)[:3]
    assert at.size == 3 and len({tuple(r65[i].tolist()) for i in at}) == 3
    # another seed, another draw
    assert not np.array_equal(N.negatives_reference(c.csr, c.sources, 65, seed=NC.SEED + 1).numpy(), r65)


def test_rows_max_draws_and_exclude():
    c = NC.case("S")
    rows, short = N.negatives_reference(c.csr, c.sources, 65, seed=NC.SEED, max_draws=64, return_short=True)
    r65, _ = NC.ref_rows("S", 65)
    rows = rows.numpy()
    for got, full in zip(rows, r65):                                    # 64 draws give a prefix of the full row
        m = int((got >= 0).sum())
        assert m < 65 and np.array_equal(got[:m], full[:m]) and (got[m:] == -1).all()
    assert short == c.sources.size
    ex, _ = NC.ref_rows("S", 63, exclude=True)
    NC.check_rows(c.csr, c.sources, ex, extra=c.held)
    assert not np.array_equal(ex, NC.ref_rows("S", 63)[0])
    # the same exclusion as [E, 2] and as a CSR
    as_rows = N.negatives_reference(c.csr, c.sources, 63, seed=NC.SEED, exclude=torch.from_numpy(c.held.T.copy()))
    as_csr = N.negatives_reference(c.csr, c.sources, 63, seed=NC.SEED, exclude=graph.mask_csr(c.held, c.n, symmetric=False))
    assert np.array_equal(as_rows.numpy(), ex) and np.array_equal(as_csr.numpy(), ex)


# ------------------------------------------------------------------------------------------ the restatement: pairs
@pytest.mark.parametrize("name", ["S", "H", "C"])
@pytest.mark.parametrize("m", NC.PAIR_MS)
def test_pairs_properties(name, m):
    c = NC.case(name)
    plain, lost = NC.ref_pairs(name, m, False)
    assert plain.shape == (2, m) and plain.dtype == np.int64
    NC.check_pairs(c.csr, plain, unique=False)
    assert lost == (m if name == "C" else 0) == int((plain[0] < 0).sum())
    for rounds in (1, 8):
        uniq, short = NC.ref_pairs(name, m, True, rounds)
        NC.check_pairs(c.csr, uniq, unique=True)
        assert short == int((uniq[0] < 0).sum())
        keep = uniq[0] >= 0
        if rounds == 1:                                                  # one draw: the winners of the plain call
            assert np.array_equal(uniq[:, keep], plain[:, keep])
    if name == "S" and m == 1000:
        # 1,000 distinct pairs out of about 2,200 free ones: one round leaves losers, eight resolve more of them
        s1, s8 = NC.ref_pairs(name, m, True, 1)[1], NC.ref_pairs(name, m, True, 8)[1]
        assert s1 > 50 and s8 < s1
    if name == "H":
        assert NC.ref_pairs(name, m, True, 8)[1] == 0


def test_pairs_slots_and_exclude():
    c = NC.case("S")
    plain, _ = NC.ref_pairs("S", 1000, False)
    part = N.negatives_reference(c.csr, num=300, seed=NC.SEED, unique=False, slot_base=700)
    assert np.array_equal(part.numpy(), plain[:, 700:])                 # a slot depends on its index only
    ex, _ = NC.ref_pairs("S", 1000, True, 8, exclude=True)
    NC.check_pairs(c.csr, ex, unique=True, extra=c.held)
    # max_draws = 1: the slots whose first pair is rejected hold (-1, -1)
    one, lost = N.negatives_reference(c.csr, num=1000, seed=NC.SEED, unique=False, max_draws=1, return_short=True)
    one = one.numpy()
    assert 0 < lost == int((one[0] < 0).sum()) < 400
    assert np.array_equal(one[:, one[0] >= 0], plain[:, one[0] >= 0])


def test_complete_graph_and_check():
    c = NC.case("C")
    rows, short = N.negatives_reference(c.csr, c.sources, 4, seed=1, return_short=True)
    assert (rows == -1).all() and short == c.sources.size
    pairs, lost = N.negatives_reference(c.csr, num=64, seed=1, return_short=True)
    assert (pairs == -1).all() and lost == 64
    if not torch.cuda.is_available():                                    # (the public entry points on a host CSR)
        with pytest.raises(ValueError, match="7 of 7 rows"):
            lpformer_amd.negative_rows(c.csr, c.sources, 4, seed=1)
        with pytest.raises(ValueError, match="64 of 64 pairs"):
            lpformer_amd.negative_pairs(c.csr, 64, seed=1)
        assert (lpformer_amd.negative_pairs(c.csr, 64, seed=1, check=False) == -1).all()
        s = NC.case("S")
        got = lpformer_amd.negative_rows(s.csr, s.sources, 63, seed=NC.SEED, check=False, as_pairs=True)
        assert got.shape == (s.sources.size, 63, 2) and np.array_equal(got[..., 1].numpy(), NC.ref_rows("S", 63)[0])
        assert (got[..., 0] == torch.from_numpy(s.sources.copy())[:, None]).all()


def test_bad_arguments():
    c = NC.case("S")
    for bad in (0, 1025, 2.0, True):
        with pytest.raises(ValueError):
            N.negatives_reference(c.csr, c.sources, bad, seed=0)
    with pytest.raises(ValueError):
        N.negatives_reference(c.csr, c.sources, 4, seed=0.5)
    with pytest.raises(ValueError):
        N.negatives_reference(c.csr, c.sources, 4, num=3, seed=0)
    with pytest.raises(ValueError):
        N.negatives_reference(c.csr, num=3, seed=0, rounds=0)
    with pytest.raises(ValueError):
        N.UniformNegatives(c.csr, seed=0, mode="head")


# ------------------------------------------------------------------------------------------------------ link_split
@pytest.fixture(scope="module")
def split_graph():
    n = 300
    ei, _ = D.chung_lu_graph(n, 1200)
    x = np.random.default_rng(0).standard_normal((n, 8)).astype(np.float32)
    return n, ei, x


def _keys(pairs, n):
    p = np.asarray(pairs).reshape(-1, 2)
    return np.minimum(p[:, 0], p[:, 1]) * n + np.maximum(p[:, 0], p[:, 1])


@pytest.mark.parametrize("layout", ["shared", "rows"])
def test_link_split(split_graph, layout):
    n, ei, x = split_graph
    kw = dict(eps=1e-3, seed=4, negatives=layout, num_neg=None if layout == "shared" else 20)
    data = D.link_split(ei, x, n, **kw)
    canon = np.unique(_keys(ei[:, ei[0] != ei[1]].T, n))
    E = canon.size
    tr, va, te = (_keys(data[k].numpy(), n) for k in ("train_pos", "valid_pos", "test_pos"))
    # a partition of the canonical edges, sized by the fractions
    assert va.size == int(0.05 * E) and te.size == int(0.10 * E) and tr.size == E - va.size - te.size
    assert np.array_equal(np.sort(np.concatenate([tr, va, te])), canon)
    for k in ("train_pos", "valid_pos", "test_pos", "train_pos_val"):
        assert data[k].dtype == torch.int64 and data[k].dim() == 2 and data[k].shape[1] == 2
    assert data["train_pos_val"].shape == data["valid_pos"].shape and np.isin(_keys(data["train_pos_val"], n), tr).all()
    # the training adjacency holds the training edges only
    adj = data["adj_mask"]
    akeys = np.unique(_keys(np.stack([np.repeat(np.arange(n), np.diff(adj.rowptr)), adj.col], axis=1), n))
    assert np.array_equal(akeys, np.sort(tr)) and data["full_adj_mask"] is data["adj_mask"]
    assert data["edge_index"].shape == (2, 2 * tr.size)
    # the negatives avoid EVERY edge, and the two sets differ
    vn, tn = data["valid_neg"], data["test_neg"]
    if layout == "shared":
        assert vn.shape == (va.size, 2) and tn.shape == (te.size, 2)
        assert not np.isin(_keys(tn, n), _keys(vn, n)).any()                    # disjoint as unordered pairs
        assert np.unique(_keys(vn, n)).size == va.size and np.unique(_keys(tn, n)).size == te.size
    else:
        assert vn.shape == (va.size, 20, 2) and tn.shape == (te.size, 20, 2)
        assert (vn[..., 0] == data["valid_pos"][:, :1]).all() and (tn[..., 0] == data["test_pos"][:, :1]).all()
        assert all(np.unique(r).size == 20 for r in vn[..., 1].numpy())
        assert not np.array_equal(vn[:20, :, 1].numpy(), tn[:20, :, 1].numpy())
    for neg in (vn, tn):
        assert neg.dtype == torch.int64 and int(neg.min()) >= 0 and int(neg.max()) < n
        assert not np.isin(_keys(neg, n), canon).any() and (neg[..., 0] != neg[..., 1]).all()
    for k in ("x", "num_nodes", "adj_t", "full_adj_t", "adj_mask", "full_adj_mask", "ppr", "ppr_test"):
        assert k in data
    # the same arguments, the same dict
    again = D.link_split(ei, x, n, **kw)
    assert set(again) == set(data)
    for k, v in data.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, again[k]), k
        elif isinstance(v, graph.CSR):
            assert np.array_equal(v.rowptr, again[k].rowptr) and np.array_equal(v.col, again[k].col), k
    other = D.link_split(ei, x, n, **dict(kw, seed=5))
    assert not torch.equal(other["valid_pos"], data["valid_pos"]) and not torch.equal(other["valid_neg"], vn)


def test_link_split_options(split_graph):
    n, ei, x = split_graph
    data = D.link_split(torch.from_numpy(ei.T.copy()), x, n, eps=1e-3, use_val_in_test=True, num_neg=77,
                        val_frac=0.1, test_frac=0.2)
    assert data["valid_neg"].shape == (77, 2) and data["test_neg"].shape == (77, 2)
    va = _keys(data["valid_pos"], n)
    full = data["full_adj_mask"]
    fkeys = np.unique(_keys(np.stack([np.repeat(np.arange(n), np.diff(full.rowptr)), full.col], axis=1), n))
    assert np.isin(va, fkeys).all() and not np.isin(_keys(data["test_pos"], n), fkeys).any()
    assert data["full_adj_mask"] is not data["adj_mask"] and data["ppr_test"] is not data["ppr"]
    with pytest.raises(ValueError):
        D.link_split(ei, x, n, negatives="both")
    with pytest.raises(ValueError):
        D.link_split(ei, x, n, val_frac=0.6, test_frac=0.5)
    with pytest.raises(TypeError):
        D.link_split(ei, x, n, edge_weight=np.ones(ei.shape[1], np.float32))
    # a graph too dense to supply the negatives says so
    a, b = np.triu_indices(12, 1)
    with pytest.raises(ValueError, match="came up short"):
        D.link_split(np.stack([a, b]), np.zeros((12, 4), np.float32), 12, eps=1e-2)
