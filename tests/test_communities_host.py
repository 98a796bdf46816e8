"""communities without a GPU: the numpy restatement (communities_reference, what the entry point runs for a host
graph.CSR when no GPU is present) against networkx's modularity, the hand cases, the planted partitions and a per-node
loop of the move rule; the quality bound against networkx's Louvain; the helpers, argument validation and the C ABI
registration."""
from functools import lru_cache

import networkx as nx
import numpy as np
import pytest
import torch

import lpformer_amd
from lpformer_amd import _lib, community, graph
from lpformer_amd.community import (COMMUNITY_BINS, Communities, communities, communities_reference,
                                    move_round_reference, partition_quality, quality_reference, same_community)
from lpformer_amd.structure import pair_node_values
from tests import communities_cases as CC
from tests import node_structure_cases as NC

SYMBOLS = {"lpf_community_workspace_bytes": 3, "lpf_community_move": 21, "lpf_community_quality": 8}


@lru_cache(maxsize=None)
def _nx_graph(name):
    A = CC.CASES[name]().A.copy()
    A.setdiag(0)
    A.eliminate_zeros()
    return nx.from_scipy_sparse_array(A)


@lru_cache(maxsize=None)
def _nx_louvain_modularity(name) -> float:
    G = _nx_graph(name)
    return nx.community.modularity(G, nx.community.louvain_communities(G, seed=0))


def _parts(label: np.ndarray):
    order = np.argsort(label, kind="stable")
    return [set(p.tolist()) for p in np.split(order, np.nonzero(np.diff(label[order]))[0] + 1)] if label.size else []


def _check_valid(name, c: Communities):
    case = CC.CASES[name]()
    G = _nx_graph(name)
    label = c.label.numpy()
    n = case.n
    assert c.n == n and c.label.dtype == torch.int32 and label.shape == (n,)
    # every community is named by its smallest member
    assert (label <= np.arange(n)).all() and (label[label] == label).all()
    assert c.count == np.unique(label).size
    degree = np.asarray([G.degree(v) for v in range(n)], np.int64)
    assert c.two_m == int(degree.sum())
    # the exact numerator against networkx's modularity of the same partition
    want = nx.community.modularity(G, _parts(label)) * c.two_m ** 2
    assert abs(c.quality_num - want) <= 1e-9 * max(abs(c.quality_num), 1), (c.quality_num, want)
    assert isinstance(c.quality_num, int) and c.modularity == c.quality_num / c.two_m ** 2
    # no community spans two components; isolated nodes are singletons
    component = CC.component(name)
    assert (component[label] == component).all()
    isolated = np.nonzero(degree == 0)[0]
    assert (label[isolated] == isolated).all() and (np.bincount(label, minlength=n)[isolated] == 1).all()
    # Qnum rises strictly over the kept levels, from at least the singletons' value
    q = [-int((degree * degree).sum())] + [lv["quality_num"] for lv in c.levels]
    assert all(b > a for a, b in zip(q[1:], q[2:])) and (len(q) == 1 or q[1] > q[0])
    assert c.quality_num == q[-1] and len(c.hierarchy) == len(c.levels)
    nodes = [lv["nodes"] for lv in c.levels]
    assert nodes[:1] in ([], [n]) and all(b < a for a, b in zip(nodes, nodes[1:]))
    for lv, h in zip(c.levels, c.hierarchy):
        assert 1 <= lv["accepted"] <= lv["rounds"] <= 64 and set(lv) == {"nodes", "rounds", "accepted", "quality_num"}
        hl = h.numpy()
        assert h.dtype == torch.int32 and (hl[hl] == hl).all() and (hl <= np.arange(n)).all()
        assert quality_reference(case.A.indptr, case.A.indices, None, None, degree, hl) == lv["quality_num"]
    # each level merges communities of the level before
    for fine, coarse in zip(c.hierarchy, c.hierarchy[1:]):
        assert torch.equal(coarse[fine.long()], coarse)
    if c.hierarchy:
        assert torch.equal(c.hierarchy[-1], c.label)


@pytest.mark.parametrize("hand", CC.hand_cases(), ids=lambda h: h.what)
def test_restatement_matches_the_hand_cases(hand):
    for seed in (0, 1, 2, 3):
        c = communities_reference(hand.csr, seed=seed)
        assert c.label.tolist() == hand.label and c.count == hand.count, seed
    assert c.n == hand.csr.n and not c.label.is_cuda


@pytest.mark.parametrize("name", CC.NAMES)
def test_restatement_gives_a_valid_partition_of_exact_quality(name):
    c = CC.reference(name)
    print(name, "communities", c.count, "modularity", c.modularity, "levels", c.levels)
    _check_valid(name, c)


@pytest.mark.parametrize("name", ("K", "S", "B"))
def test_two_seeds_are_valid_and_a_seed_is_reproducible(name):
    csr = CC.CASES[name]().csr
    a, b, other = communities_reference(csr, seed=1), communities_reference(csr, seed=1), CC.reference(name)
    _check_valid(name, a)
    assert torch.equal(a.label, b.label) and a.levels == b.levels and a.quality_num == b.quality_num
    assert all(torch.equal(x, y) for x, y in zip(a.hierarchy, b.hierarchy))
    assert a.levels != other.levels or not torch.equal(a.label, other.label)      # the seed is used


def test_stored_self_loops_change_nothing():
    plain, loops = CC.reference("K"), CC.reference("Kloops")
    assert torch.equal(plain.label, loops.label) and plain.levels == loops.levels and plain.two_m == loops.two_m


@pytest.mark.parametrize("seed", (0, 1, 2, 3))
def test_planted_cliques_come_out_one_community_each(seed):
    d, r = CC.reference("D", seed), CC.reference("R", seed)
    np.testing.assert_array_equal(d.label.numpy(), CC.d_planted())
    np.testing.assert_array_equal(r.label.numpy(), CC.r_planted())
    assert d.count == len(CC.D_CLIQUES) + 5 and r.count == CC.R_CLIQUES


@pytest.mark.parametrize("name", CC.QUALITY_GRAPHS)
def test_quality_against_networkx_louvain(name):
    """modularity >= (1 - margin) * modularity of networkx.community.louvain_communities(seed=0), seeds 0 - 3; the
    margin and the shortfalls it was set from: tests/communities_cases.py."""
    want = _nx_louvain_modularity(name)
    got = [CC.reference(name, seed).modularity for seed in CC.QUALITY_SEEDS]
    print(name, "networkx", want, "shortfalls", [round(1 - q / want, 4) for q in got], "margin", CC.QUALITY_MARGIN)
    assert CC.QUALITY_MARGIN >= 0.01
    for q in got:
        assert q >= (1 - CC.QUALITY_MARGIN) * want


def _move_round_by_loops(lv, seed, level, rnd):
    """The round of the module docstring, one node at a time in Python integers."""
    n = lv["k"].size
    act = community.active_nodes(seed, level, rnd, n)
    comm, tot, cnt, k = (lv[x].tolist() for x in ("comm", "tot", "cnt", "k"))
    new = list(comm)
    for v in range(n):
        if not act[v]:
            continue
        w_c = {}
        for e in range(lv["indptr"][v], lv["indptr"][v + 1]):
            u = int(lv["indices"][e])
            if u != v:
                w_c[comm[u]] = w_c.get(comm[u], 0) + int(lv["weight"][e])
        cur = comm[v]
        stay = lv["two_m"] * w_c.get(cur, 0) - k[v] * (tot[cur] - k[v])
        best = None
        for c, w in w_c.items():
            gain = lv["two_m"] * w - k[v] * tot[c]
            if c == cur or gain <= stay or (cnt[cur] == 1 and cnt[c] == 1 and c > cur):
                continue
            if best is None or (-gain, c) < best:
                best = (-gain, c)
        if best is not None:
            new[v] = best[1]
    return np.asarray(new, np.int64)


def test_move_round_against_a_per_node_loop():
    lv = CC.weighted_level(NC.graph_k())
    assert (lv["cnt"] == 1).any() and (lv["cnt"] > 1).any() and lv["two_m"] < 1 << 31
    for seed, level, rnd in ((0, 0, 0), (5, 1, 3), (0, 2, 63)):
        got = move_round_reference(lv["indptr"], lv["indices"], lv["weight"], lv["k"], lv["comm"], lv["tot"], lv["cnt"],
                                   lv["two_m"], seed, level, rnd)
        want = _move_round_by_loops(lv, seed, level, rnd)
        np.testing.assert_array_equal(got, want)
        act = community.active_nodes(seed, level, rnd, lv["k"].size)
        assert (got[~act] == lv["comm"][~act]).all() and (got != lv["comm"]).sum() > 100
        assert 0.4 < act.mean() < 0.6
    # the activation bit is the draw of negatives.py on Python integers
    from lpformer_amd.negatives import G, mix64
    key = mix64(5 + G * (((1 << 32) + 3) + 1))
    assert [mix64(key + G * (v + 1)) >> 63 for v in range(64)] == community.active_nodes(5, 1, 3, 64).astype(int).tolist()


def test_size_summary_same_community_and_bins():
    case, c = CC.graph_d(), CC.reference("D")
    label = CC.d_planted()
    sizes = np.bincount(label, minlength=case.n)
    assert c.size.dtype == torch.int64 and np.array_equal(c.size.numpy(), sizes[label])
    s = c.summary()
    assert s == {"communities": 11, "largest_share": 130 / case.n, "median_size": 3.0, "modularity": c.modularity,
                 "levels": len(c.levels)}
    assert all(type(v) in (int, float) for v in s.values())
    a, b = case.pairs
    ok = (a >= 0) & (a < case.n) & (b >= 0) & (b < case.n)
    assert int((~ok).sum()) == 4
    want = ok & (label[np.where(ok, a, 0)] == label[np.where(ok, b, 0)])
    for edges in (torch.from_numpy(case.pairs.copy()), torch.from_numpy(case.pairs.T.copy()), case.pairs.copy()):
        same = same_community(c, edges)
        assert same.dtype == torch.bool and np.array_equal(same.numpy(), want)
    assert want.any() and not want.all()
    assert same_community(c, torch.zeros(2, 0, dtype=torch.int64)).shape == (0,)
    assert COMMUNITY_BINS == ((0, 1), (1, 2))
    pos, neg = torch.arange(same.numel(), dtype=torch.float32), torch.zeros(16)
    rows = lpformer_amd.evaluate.metrics_by_bin(pos, neg, same.to(torch.int64), bins=COMMUNITY_BINS)
    assert len(rows) == 2
    size_axis = pair_node_values(c.size, torch.from_numpy(case.pairs.copy()))
    assert np.array_equal(size_axis.numpy(), np.where(ok, np.minimum(sizes[label][np.where(ok, a, 0)],
                                                                     sizes[label][np.where(ok, b, 0)]), -1))
    empty = communities_reference(graph.CSR(np.zeros(1, np.int64), np.zeros(0, np.int32), None, 0))
    assert empty.count == 0 and empty.label.shape == (0,) and empty.modularity == 0.0 and empty.levels == []
    assert empty.summary()["communities"] == 0 and empty.size.shape == (0,)


def test_argument_errors_come_before_any_device_use():
    csr = CC.graph_r().csr
    for fn in (communities, communities_reference):
        for bad in ({"seed": 1.5}, {"seed": True}, {"max_levels": 0}, {"max_levels": 2.0}, {"max_rounds": 0},
                    {"max_rounds": None}, {"patience": 0}, {"patience": "3"}, {"tolerance": -1e-3}, {"tolerance": 1.0},
                    {"tolerance": "1e-6"}):
            with pytest.raises(ValueError):
                fn(csr, **bad)
    for bad in (63, 100, 32, 16384, 64.0, True):
        with pytest.raises(ValueError):
            communities(csr, lds_slots=bad)
    with pytest.raises(TypeError):
        communities("not a graph")
    with pytest.raises(TypeError):
        communities((csr, None))
    with pytest.raises(TypeError):
        partition_quality("not a graph", np.zeros(3, np.int64))
    for bad in (np.zeros(csr.n - 1, np.int64), np.zeros((csr.n, 1), np.int64), np.zeros(csr.n, np.float32)):
        with pytest.raises(ValueError):
            partition_quality(csr, bad)


def test_host_csr_without_a_gpu():
    """Through the public functions where they take the host path (no GPU present), else the restatement itself."""
    case, ref = CC.graph_b(), CC.reference("B")
    c = (communities_reference if torch.cuda.is_available() else communities)(case.csr)
    assert not c.label.is_cuda and torch.equal(c.label, ref.label) and c.levels == ref.levels
    if not torch.cuda.is_available():
        assert partition_quality(case.csr, ref.label) == (ref.quality_num, ref.two_m)
        assert partition_quality(case.csr, ref.hierarchy[0].numpy()) == (ref.levels[0]["quality_num"], ref.two_m)
        one = partition_quality(case.csr, np.zeros(case.n, np.int64))
        assert one == (0, ref.two_m)                               # one part: 2m * 2m - (2m)^2


def test_abi_registration_and_exports():
    assert _lib.ABI_VERSION == 16
    for name, n_args in SYMBOLS.items():
        assert len(_lib.HIP_PROTOTYPES[name]) == n_args and _lib.PROTOTYPES[name][0] is not None
    assert (_lib.CONST["LPF_COMM_LONG_ROW"], _lib.CONST["LPF_COMM_LDS_SLOTS"], _lib.CONST["LPF_COMM_LDS_SLOTS_MAX"]) == \
        (64, 4096, 8192)
    hip = _lib.hip()                                                          # loads without a GPU
    # bad arguments are refused before anything touches a device
    assert hip.lpf_community_move(-1, 0, None, None, None, None, None, None, None, 0, 0, 0, 0, None, 0, 64, None, 0,
                                  None, None, None) == -1
    assert hip.lpf_community_move(5, 0, None, None, None, None, None, None, None, 0, 0, 0, 0, None, 0, 64, None, 0,
                                  None, None, None) == -1
    assert hip.lpf_community_quality(3, -1, None, None, None, None, None, None) == -1
    assert hip.lpf_community_quality(3, 0, None, None, None, None, None, None) == -1
    # the workspace: none while every listed row's table fits the LDS slots, else one table per persistent workgroup
    assert hip.lpf_community_workspace_bytes(0, 0, 4096) == 0
    assert hip.lpf_community_workspace_bytes(10, 2048, 4096) == 0
    assert hip.lpf_community_workspace_bytes(10, 2049, 4096) == 10 * 8192 * 12
    assert hip.lpf_community_workspace_bytes(3, 129, 64) == 3 * 512 * 12
    assert hip.lpf_community_workspace_bytes(100000, 129, 64) == 512 * 512 * 12
    for bad in (63, 96, 16384, 0, -64):
        assert hip.lpf_community_workspace_bytes(3, 129, bad) == -1
    assert hip.lpf_community_workspace_bytes(-1, 129, 64) == -1
    for name in ("communities", "Communities", "communities_reference", "partition_quality", "same_community",
                 "COMMUNITY_BINS"):
        assert getattr(lpformer_amd, name) is getattr(community, name) and name in lpformer_amd.__all__
    assert "communities" in lpformer_amd.__doc__
