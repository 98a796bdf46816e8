"""Graph edits with the exact incremental PPR refresh, host path (lpf_ppr_push_cpu_sources + numpy):
``update_ppr`` / ``update_data`` against the full producers on the edited edge list, array by array and bit by bit."""
import os

import numpy as np
import pytest

import lpformer_amd
from lpformer_amd import _lib, graph
from lpformer_amd import data as D
from lpformer_amd import graph_update as U
from lpformer_amd import readers as R
from lpformer_amd.ppr import calc_ppr
from tests.golden_util import GOLDEN_DIR

ALPHA, EPS, N = 0.15, 1e-3, 3000


def assert_same_csr(a, b, what=""):
    np.testing.assert_array_equal(a.rowptr, b.rowptr, err_msg=f"rowptr {what}")
    np.testing.assert_array_equal(a.col, b.col, err_msg=f"col {what}")
    if a.val is None or b.val is None:
        assert a.val is None and b.val is None, what
    else:
        np.testing.assert_array_equal(a.val.view(np.uint32), b.val.view(np.uint32), err_msg=f"val {what}")


def edited_edge_list(ei, n, add=None, remove=None):
    """Restatement of the edit: both directions of every pair, (old | add) - remove, sorted."""
    keys = set((ei[0].astype(np.int64) * n + ei[1]).tolist())
    for pairs, op in ((add, keys.add), (remove, keys.discard)):
        if pairs is not None:
            for a, b in np.asarray(pairs, np.int64).T.tolist():
                op(a * n + b)
                op(b * n + a)
    k = np.array(sorted(keys), np.int64)
    return np.stack([k // n, k % n])


@pytest.fixture(scope="module")
def base():
    ei, _ = D.chung_lu_graph(N, 12000, seed=1)
    return ei, calc_ppr(ei, N, ALPHA, EPS)


def random_pairs(k, seed=0):
    """k random non-loop pairs."""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, N, size=(2, 2 * k))
    return p[:, p[0] != p[1]][:, :k]


def edit_cases(ei):
    """name -> (add, remove): the case list of the issue (shared with tests/test_gpu_graph_update.py)."""
    rng = np.random.default_rng(7)
    deg = np.bincount(ei[0], minlength=N)
    hub, isolated = int(np.argmax(deg)), int(np.flatnonzero(deg == 0)[0])
    add = random_pairs(20)
    present = ei[:, rng.choice(ei.shape[1], 10, replace=False)]
    absent = random_pairs(5, seed=11)
    others = rng.choice(np.flatnonzero((deg > 0) & (np.arange(N) != hub)), 3, replace=False)
    return {
        "add": (add, None),
        "remove": (None, present),
        "mixed": (add[:, :8], present[:, :4]),
        "noop": (present[:, :3], absent),                       # additions that exist + removals that do not
        "noop_plus_real": (np.concatenate([present[:, :3], add[:, :2]], axis=1),
                           np.concatenate([absent, present[:, 5:6]], axis=1)),
        "hub": (np.stack([np.full(3, hub), others]), None),
        "isolated": (np.array([[isolated], [int(others[0])]]), None),
        "twin_reversed": (np.concatenate([add[:, :4], add[::-1, :4]], axis=1), None),
    }


def test_push_sources_equals_rows_of_the_full_push(base):
    ei, full = base
    g = graph.csr_from_coo(ei[0], ei[1], None, N)
    src = np.unique(np.random.default_rng(1).integers(0, N, 200)).astype(np.int32)
    for threads in (1, 3):
        rp, c, v = U._push_sources_host(g.rowptr, g.col, N, src, ALPHA, EPS, threads)
        for i, s in enumerate(src):
            a0, a1 = full.rowptr[s], full.rowptr[s + 1]
            np.testing.assert_array_equal(c[rp[i]:rp[i + 1]], full.col[a0:a1])
            np.testing.assert_array_equal(v[rp[i]:rp[i + 1]].view(np.uint32), full.val[a0:a1].view(np.uint32))
    rp, c, v = U._push_sources_host(g.rowptr, g.col, N, src[:0], ALPHA, EPS)
    assert rp.tolist() == [0] and c.size == 0
    bad = np.array([5, 5], np.int32)                                   # not strictly ascending
    with pytest.raises(_lib.LpfError):
        U._push_sources_host(g.rowptr, g.col, N, bad, ALPHA, EPS)


@pytest.mark.parametrize("case", ["add", "remove", "mixed", "noop", "noop_plus_real", "hub", "isolated",
                                  "twin_reversed"])
def test_update_ppr_equals_full_push_on_edited_graph(base, case):
    ei, old = base
    add, remove = edit_cases(ei)[case]
    new, stats = lpformer_amd.update_ppr(old, ei, add=add, remove=remove, alpha=ALPHA, eps=EPS, full_above=1.0)
    assert stats["path"] == "incremental"
    assert_same_csr(new, calc_ppr(edited_edge_list(ei, N, add, remove), N, ALPHA, EPS), case)
    if case == "noop":
        assert stats["n_add_noop"] == 3 and stats["n_remove_noop"] == 5
        assert stats["n_keys"] == 0 and stats["n_affected"] == 0
        assert_same_csr(new, old)
    if case == "noop_plus_real":
        assert stats["n_add_noop"] == 3 and stats["n_remove_noop"] == 5 and stats["n_keys"] > 0


def test_incremental_path_does_not_repush_everything(base):
    ei, old = base
    add = random_pairs(20)
    sources, s0 = lpformer_amd.ppr_affected_sources(old, ei, add=add)
    new, stats = lpformer_amd.update_ppr(old, ei, add=add, alpha=ALPHA, eps=EPS, full_above=1.0)
    print(f"keys {stats['n_keys']}, flagged {stats['n_affected']} of {N} ({stats['fraction']:.3f})")
    assert stats["n_affected"] == sources.size == s0["n_affected"] and stats["n_affected"] < 0.5 * N
    assert np.all(np.diff(sources) > 0)
    ref = calc_ppr(edited_edge_list(ei, N, add), N, ALPHA, EPS)
    flagged = np.zeros(N, bool)
    flagged[sources] = True
    for s in range(N):
        a, b, c = (slice(m.rowptr[s], m.rowptr[s + 1]) for m in (old, new, ref))
        same_as_old = (np.array_equal(old.col[a], ref.col[c]) and
                       np.array_equal(old.val[a].view(np.uint32), ref.val[c].view(np.uint32)))
        if not flagged[s]:      # untouched by the update, and rightly so
            assert np.array_equal(new.col[b], old.col[a]) and np.array_equal(new.val[b].view(np.uint32),
                                                                              old.val[a].view(np.uint32))
            assert same_as_old, f"row {s} changed but was not flagged"
    # (ppr_affected_sources also takes the adjacency as a CSR)
    s2, _ = lpformer_amd.ppr_affected_sources(old, graph.csr_from_coo(ei[0], ei[1], None, N), add=add)
    np.testing.assert_array_equal(s2, sources)


@pytest.mark.parametrize("with_val", [False, True])
def test_update_data_equals_build_data(with_val):
    n = 800
    ei, w = D.chung_lu_graph(n, 3000, seed=3, max_weight=4)
    x = np.random.default_rng(0).standard_normal((n, 8)).astype(np.float32)
    rng = np.random.default_rng(5)
    val = rng.integers(0, n, size=(2, 150))
    val = val[:, val[0] != val[1]]
    val = np.concatenate([val, ei[:, :5]], axis=1) if with_val else None     # (five validation edges are training edges too)
    data = D.build_data(ei, x, n, edge_weight=w, eps=EPS, val_edge_index=val)
    before = {k: (v.rowptr.copy(), v.col.copy(), None if v.val is None else v.val.copy())
              for k, v in data.items() if isinstance(v, graph.CSR)}
    add = rng.integers(0, n, size=(2, 12))
    add = add[:, add[0] != add[1]]
    if with_val:
        add = np.concatenate([add, val[:, :2]], axis=1)          # accept two validation edges into the training graph
    remove = ei[:, rng.choice(ei.shape[1], 4, replace=False)]
    if with_val:
        remove = np.concatenate([remove, ei[:, :1]], axis=1)     # a training edge that is ALSO a validation edge
    stats = {}
    new = lpformer_amd.update_data(data, add=add, remove=remove, alpha=ALPHA, eps=EPS, edge_weight=2.0,
                                   full_above=1.0, stats=stats)
    # the edited training edge list with weights: old weights kept, new edges get 2.0
    ei2 = edited_edge_list(ei, n, add, remove)
    old_w = dict(zip((ei[0] * n + ei[1]).tolist(), w.tolist()))
    w2 = np.array([old_w.get(k, 2.0) for k in (ei2[0] * n + ei2[1]).tolist()], np.float32)
    want = D.build_data(ei2, x, n, edge_weight=w2, eps=EPS, val_edge_index=val)
    for k in ("adj_t", "adj_mask", "full_adj_t", "full_adj_mask", "ppr", "ppr_test"):
        assert_same_csr(new[k], want[k], k)
    assert new["x"] is data["x"] and new is not data
    assert (new["ppr_test"] is new["ppr"]) == (not with_val) == (data["ppr_test"] is data["ppr"])
    assert (new["full_adj_t"] is new["adj_t"]) == (not with_val)
    assert stats["ppr"]["path"] == "incremental" and ("ppr_test" in stats) == with_val
    for k, (rp, c, v) in before.items():      # the input dict and its arrays are untouched
        np.testing.assert_array_equal(data[k].rowptr, rp)
        np.testing.assert_array_equal(data[k].col, c)
        if v is not None:
            np.testing.assert_array_equal(data[k].val, v)


def _pairs_missing(full_keys_of, train_keys_of, n):
    k = np.setdiff1d(full_keys_of, train_keys_of)
    return np.stack([k // n, k % n])


def test_ppr_test_from_ppr_on_golden_fixture():
    """data["ppr_test"] is an edge insertion applied to data["ppr"]: the validation edges."""
    z = np.load(os.path.join(GOLDEN_DIR, "lp_all_d64_residual_valtest.npz"))
    n, eps = 360, 1e-3
    ei, full = z["edge_index"].astype(np.int64), z["full_edge_index"].astype(np.int64)
    val_pairs = _pairs_missing(full[0] * n + full[1], ei[0] * n + ei[1], n)
    assert val_pairs.shape[1] > 0
    ppr = graph.csr_from_coo(z["ppr_row"], z["ppr_col"], z["ppr_val"], n)           # recorded from the reference
    want = graph.csr_from_coo(z["ppr_test_row"], z["ppr_test_col"], z["ppr_test_val"], n)
    got, stats = lpformer_amd.update_ppr(ppr, ei, add=val_pairs, alpha=ALPHA, eps=eps, full_above=1.0, verify=8)
    assert stats["path"] == "incremental"
    assert_same_csr(got, want)
    assert_same_csr(got, calc_ppr(full, n, ALPHA, eps))


def test_ppr_test_from_ppr_on_ogb_tiny_collab():
    import torch
    torch.manual_seed(5)
    d = R.read_data_ogb(os.path.join(GOLDEN_DIR, "ogb_tiny"), "ogbl-collab", eps=1e-3, dim=16, use_val_in_test=True)
    n = d["num_nodes"]
    assert d["ppr_test"] is not d["ppr"]

    def keys(c):
        return np.repeat(np.arange(n, dtype=np.int64), np.diff(c.rowptr)) * n + c.col

    tk = keys(d["adj_t"])
    val_pairs = _pairs_missing(keys(d["full_adj_t"]), tk, n)
    got, stats = lpformer_amd.update_ppr(d["ppr"], np.stack([tk // n, tk % n]), add=val_pairs, alpha=ALPHA, eps=1e-3,
                                         full_above=1.0)
    assert stats["path"] == "incremental" and stats["n_affected"] > 0
    assert_same_csr(got, d["ppr_test"])


def test_full_path_verify_and_argument_checks(base):
    ei, old = base
    add = random_pairs(20)
    inc, _ = lpformer_amd.update_ppr(old, ei, add=add, alpha=ALPHA, eps=EPS, full_above=1.0)
    full, stats = lpformer_amd.update_ppr(old, ei, add=add, alpha=ALPHA, eps=EPS, full_above=0.0)
    assert stats["path"] == "full"
    assert_same_csr(full, inc)
    _, stats = lpformer_amd.update_ppr(old, ei, add=add, alpha=ALPHA, eps=EPS, full_above=1.0, verify=8)
    assert stats["n_verified"] == 8
    # a matrix that does not meet the preconditions: one value of every UNFLAGGED row changed
    sources, _ = lpformer_amd.ppr_affected_sources(old, ei, add=add)
    bad = graph.CSR(old.rowptr, old.col, old.val.copy(), N)
    unflagged = np.setdiff1d(np.arange(N), sources)
    bad.val[old.rowptr[unflagged]] += np.float32(1e-3)
    with pytest.raises(_lib.LpfError, match="verify"):
        lpformer_amd.update_ppr(bad, ei, add=add, alpha=ALPHA, eps=EPS, full_above=1.0, verify=8)
    for kw in (dict(add=np.array([[3], [3]])), dict(remove=np.array([[4], [4]])), dict(add=np.array([[0], [N]])),
               dict(remove=np.array([[-1], [2]])), dict(add=np.zeros((3, 2), np.int64))):
        with pytest.raises(ValueError):
            lpformer_amd.update_ppr(old, ei, alpha=ALPHA, eps=EPS, **kw)
    with pytest.raises(ValueError):
        lpformer_amd.update_data({"adj_t": graph.csr_from_coo(ei[0], ei[1], None, N), "ppr": old}, add=[[1], [1]])
