"""The training epoch on the host: TrainEdges.covered against a brute force of the reference's rule
(src/train/train_model.py:40-45: rows outside the batch -> undirected pairs -> complement), check_against, the
bookkeeping of train_epoch and fit with stub modules, the exports."""
import numpy as np
import pytest
import torch

import lpformer_amd
from lpformer_amd import _lib, epoch, graph
from tests import epoch_cases as EC


# ------------------------------------------------------------------------------------------------------- 1. covered
def test_hand_made_rows_hold_the_cases_they_claim():
    tp = EC.hand_train_pos()
    assert tp.shape == (30, 2) and int(tp.max()) < EC.HAND_N
    te = lpformer_amd.TrainEdges(tp, EC.HAND_N)
    assert te.num_rows == 30 and te.num_groups == 30 - 1 - 1 - 2 - 2
    assert te.gid.dtype == torch.int32 and te.mult.dtype == torch.int32 and te.gkey.dtype == torch.int64
    mult = te.mult[te.gid.long()].tolist()
    assert mult[:11] == [2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 1] and set(mult[11:]) == {1}
    assert int(te.mult.sum()) == 30 and bool((te.gkey[1:] > te.gkey[:-1]).all())
    lo, hi = tp.min(1).values, tp.max(1).values
    assert torch.equal(te.gkey[te.gid.long()], lo * EC.HAND_N + hi)
    mixed = set(EC.HAND_MIXED)
    assert len(mixed) == len(EC.HAND_MIXED)
    assert len(mixed & {0, 1}) == 1 and {2, 3} <= mixed and len(mixed & {4, 5, 6}) == 2 and {7, 8, 9} <= mixed and 10 in mixed


@pytest.mark.parametrize("name", list(EC.HAND_BATCHES))
def test_covered_is_the_reference_rule(name):
    tp = EC.hand_train_pos()
    perm = torch.tensor(EC.HAND_BATCHES[name], dtype=torch.int64)
    te = lpformer_amd.TrainEdges(tp, EC.HAND_N)
    out = te.covered(perm)
    assert out.shape == (2, perm.numel()) and out.dtype == torch.int64
    want = EC.brute_force_covered(tp.numpy(), perm.numpy())
    assert np.array_equal(out.numpy(), want)                                   # the (-1, -1) positions included
    emitted = {(int(a), int(b)) for a, b in out.t().tolist() if a >= 0}
    assert emitted == EC.brute_force_removed(tp.numpy(), perm.numpy())          # as sets: the reference's removed pairs
    n_emit = int((want[0] >= 0).sum())
    assert te.stats() == [n_emit, perm.numel() - n_emit, 0, 0]
    assert not bool(te.cnt.any())
    expect = {"empty": (0, 0), "one_row": (1, 0), "one_of_two": (0, 1), "all_rows": (30, 0), "mixed": (10, 3)}[name]
    assert tuple(te.stats()[:2]) == expect
    # what RemovedEdges(edges) would remove instead: every named pair, whatever the rows outside the batch hold
    named = {tuple(sorted(r)) for r in tp[perm].tolist()}
    assert emitted <= named and (emitted != named) == (name in ("one_of_two", "mixed"))


def test_covered_accumulates_stats_counts_bad_ids_and_resets_its_counters():
    tp = EC.hand_train_pos()
    te = lpformer_amd.TrainEdges(tp, EC.HAND_N)
    a = te.covered(torch.tensor(EC.HAND_MIXED))
    b = te.covered(torch.tensor(EC.HAND_MIXED))                                # the counters were reset: same answer
    assert torch.equal(a, b) and te.stats() == [20, 6, 0, 0]
    perm = torch.tensor([30, 2, -1, 3])
    out = te.covered(perm)
    assert out.t().tolist() == [[-1, -1], [2, 3], [-1, -1], [2, 3]]
    assert te.stats(check_range=False) == [22, 6, 2, 0] and not bool(te.cnt.any())
    with pytest.raises(IndexError):
        te.stats()
    te.reset_stats()
    assert te.stats() == [0, 0, 0, 0]
    m = te.mask(torch.tensor([2, 3]))
    assert isinstance(m, graph.RemovedEdges) and m.edges.t().tolist() == [[2, 3], [2, 3]]
    with pytest.raises(ValueError):
        lpformer_amd.TrainEdges(tp.t(), EC.HAND_N)
    with pytest.raises(IndexError):
        lpformer_amd.TrainEdges(tp, EC.HAND_N - 1)


def test_mask_goes_through_the_removed_edges_path_with_its_padding():
    """(-1, -1) is padding the consumer ignores: the sorted removed keys of a mask are those of its emitted pairs."""
    from lpformer_amd import mask_delta
    tp = EC.hand_train_pos()
    te = lpformer_amd.TrainEdges(tp, EC.HAND_N)
    own = EC.symmetric_keys(tp.numpy(), EC.HAND_N)
    rk = mask_delta.removed_from_edges(own, te.mask(torch.tensor(EC.HAND_MIXED)).edges, EC.HAND_N)
    pairs = EC.brute_force_removed(tp.numpy(), EC.HAND_MIXED)
    want = sorted({a * EC.HAND_N + b for a, b in pairs} | {b * EC.HAND_N + a for a, b in pairs})
    assert rk.tolist() == want


# ------------------------------------------------------------------------------------------------- 2. check_against
def test_check_against_raises_for_an_extra_or_a_missing_edge():
    tp = EC.hand_train_pos()
    n = EC.HAND_N
    te = lpformer_amd.TrainEdges(tp, n)
    keys = EC.symmetric_keys(tp.numpy(), n)
    assert torch.equal(te.directed_keys(), keys) and (8 * n + 8) in keys.tolist()
    te.check_against(EC.AdjacencyStandIn(keys, n))
    extra = torch.unique(torch.cat([keys, torch.tensor([1 * n + 11, 11 * n + 1])]))
    missing = keys[(keys != 0 * n + 2) & (keys != 2 * n + 0)]
    swapped = torch.unique(torch.cat([missing, torch.tensor([1 * n + 11, 11 * n + 1])]))      # same size, other edge
    assert swapped.numel() == keys.numel()
    for bad in (extra, missing, swapped):
        with pytest.raises(ValueError):
            lpformer_amd.TrainEdges(tp, n).check_against(EC.AdjacencyStandIn(bad, n))
    with pytest.raises(ValueError):
        lpformer_amd.TrainEdges(tp, n + 1).check_against(EC.AdjacencyStandIn(keys, n))


# --------------------------------------------------------------------------------------------------- 3. train_epoch
class _StubModel(torch.nn.Module):
    def __init__(self, keys, n):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor([0.3, -0.2]))
        self.keys, self.num_nodes, self.calls, self.key_reads = keys, n, [], 0

    def _own_mask_keys(self, test_set):
        self.key_reads += 1
        return self.keys

    def forward(self, edges, adj_prop=None, adj_mask=None):
        self.calls.append((edges, adj_prop, adj_mask, self.training))
        x = torch.stack([edges[0], edges[1]], dim=1).double() / self.num_nodes
        return (x * self.w.double()).float()


class _StubScore(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.b = torch.nn.Parameter(torch.tensor(0.1))

    def forward(self, h):
        return torch.sigmoid(h.sum(dim=1) + self.b)


def _stub_setup(E=300, n=500, weights=None):
    rng = np.random.default_rng(5)
    key = rng.choice(n * (n - 1) // 2, E, replace=False)          # E distinct pairs u < v
    u = (np.floor((1 + np.sqrt(1 + 8 * key)) / 2)).astype(np.int64)
    v = key - u * (u - 1) // 2
    tp = torch.from_numpy(np.stack([v, u], axis=1))
    keys = EC.symmetric_keys(tp.numpy(), n)
    both = np.concatenate([tp.numpy(), tp.numpy()[:, ::-1]]).T
    val = np.ones(both.shape[1], np.float32) if weights is None else weights(both.shape[1])
    data = {"train_pos": tp, "num_nodes": n, "adj_t": graph.csr_from_coo(both[0], both[1], val, n)}
    model, score = _StubModel(keys, n), _StubScore()
    opt = torch.optim.SGD(list(model.parameters()) + list(score.parameters()), lr=0.1)
    return data, model, score, opt


def test_train_epoch_bookkeeping():
    data, model, score, opt = _stub_setup()
    steps = []
    w0 = model.w.detach().clone()
    loss = lpformer_amd.train_epoch(model, score, data, opt, batch_size=128, num_negative=2,
                                    generator=torch.Generator().manual_seed(3),
                                    on_step=lambda i, l: steps.append((i, l)))
    assert [i for i, _ in steps] == [0, 1, 2] and all(isinstance(l, torch.Tensor) and not l.requires_grad for _, l in steps)
    pos_calls, neg_calls = model.calls[0::2], model.calls[1::2]
    assert [c[0].shape[1] for c in pos_calls] == [128, 128, 44] and [c[0].shape[1] for c in neg_calls] == [256, 256, 88]
    assert all(c[3] for c in model.calls) and score.training
    want = sum(float(l) * b for (_, l), b in zip(steps, (128, 128, 44))) / 300
    assert loss == want
    # every row once; the mask of a batch of unique rows names exactly its edges; no propagation override
    seen = torch.cat([c[0] for c in pos_calls], dim=1).t()
    assert sorted(map(tuple, seen.tolist())) == sorted(map(tuple, data["train_pos"].tolist()))
    for c in pos_calls:
        assert c[1] is None and isinstance(c[2], graph.RemovedEdges) and torch.equal(c[2].edges, c[0])
    assert all(c[1] is None and c[2] is None for c in neg_calls)
    assert all(int(c[0].min()) >= 0 and int(c[0].max()) < 500 for c in neg_calls)
    assert not torch.equal(model.w.detach(), w0)                      # the optimiser stepped
    assert all(p.grad is None or not bool(p.grad.any()) for p in list(model.parameters()) + list(score.parameters()))
    # the index is built once and kept with the data; the adjacency check ran once per (index, adjacency)
    te = data[epoch._CACHE_KEY][1]
    lpformer_amd.train_epoch(model, score, data, opt, batch_size=128)
    assert data[epoch._CACHE_KEY][1] is te and te.stats() == [600, 0, 0, 0]
    assert model.key_reads == 2                                        # (read per epoch, compared once)
    assert len(te._checked) == 1


def test_train_epoch_honours_batches_negatives_clip_and_mask_input():
    data, model, score, opt = _stub_setup()
    batches = [torch.arange(0, 7), torch.arange(100, 103), torch.tensor([299])]
    negs = [torch.randint(0, 500, (2, 5)) for _ in batches]
    asked = []

    def negatives(step, edges):
        asked.append((step, edges.shape[1]))
        return negs[step]
    steps = []
    te = lpformer_amd.TrainEdges(data["train_pos"], 500)
    loss = lpformer_amd.train_epoch(model, score, data, opt, batches=batches, negatives=negatives, train_edges=te,
                                    clip=None, mask_input=True, on_step=lambda i, l: steps.append(float(l)))
    assert epoch._CACHE_KEY not in data and te.stats() == [11, 0, 0, 0]
    assert asked == [(0, 7), (1, 3), (2, 1)]
    for k, b in enumerate(batches):
        pos, neg = model.calls[2 * k], model.calls[2 * k + 1]
        assert torch.equal(pos[0], data["train_pos"][b].t()) and neg[0] is negs[k]
        assert pos[1] is pos[2] and isinstance(pos[1], graph.RemovedEdges)        # --mask-input: the same difference
    assert loss == (steps[0] * 7 + steps[1] * 3 + steps[2] * 1) / 11
    # a weighted propagation matrix: the reference's masked matrix is unweighted -- refuse, do not guess
    data_w, model_w, score_w, opt_w = _stub_setup(weights=lambda m: np.linspace(1.0, 2.0, m).astype(np.float32))
    with pytest.raises(ValueError, match="adj_prop"):
        lpformer_amd.train_epoch(model_w, score_w, data_w, opt_w, batch_size=128, mask_input=True)
    assert model_w.calls == []
    lpformer_amd.train_epoch(model_w, score_w, data_w, opt_w, batch_size=128)      # without mask_input: fine
    # row ids outside [0, E) surface at the end of the epoch
    with pytest.raises(IndexError):
        lpformer_amd.train_epoch(model, score, data, opt, batches=[torch.tensor([0, 300])])
    # the adjacency must be the training edges'
    model.keys = model.keys[1:]
    with pytest.raises(ValueError):
        lpformer_amd.train_epoch(model, score, data, opt, batch_size=128)


# ------------------------------------------------------------------------------------------------------------ 4. fit
def _scripted(monkeypatch, model, valid_scores):
    seen = []

    def fake_evaluate(m, s, d, batch_size=32768, k_list=(100,), heart=False):
        i = len(seen)
        seen.append({"w": m.w.detach().clone(), "k_list": k_list, "heart": heart})
        v = valid_scores[i]
        return {"Hits@100": (0.9, v, v / 2), "Hits@20": (0.5, 1.0 - v, 0.0), "MRR": (0.1, 0.2, 0.3)}
    monkeypatch.setattr(lpformer_amd.evaluate, "evaluate_model", fake_evaluate)
    return seen


def test_fit_early_stops_as_the_reference_counts(monkeypatch):
    data, model, score, opt = _stub_setup()
    #        improves  improves  stale 1  stale 2 (a tie is no improvement)  stale 3 > kill_cnt = 2: stop
    script = [0.10, 0.30, 0.20, 0.30, 0.25, 0.99, 0.99]
    seen = _scripted(monkeypatch, model, script)
    out = lpformer_amd.fit(model, score, data, opt, epochs=20, eval_steps=1, kill_cnt=2, decay=0.5, batch_size=128)
    assert len(seen) == 5 and len(out["history"]) == 5 and out["stopped_early"]
    assert out["best_epoch"] == 2 and out["best_valid"] == 0.30
    assert torch.equal(out["model_state"]["w"], seen[1]["w"]) and not torch.equal(seen[1]["w"], model.w.detach())
    assert set(out["score_state"]) == {"b"}
    assert [h["lr"] for h in out["history"]] == [0.1 * 0.5 ** e for e in range(5)]
    assert all(np.isfinite(h["loss"]) and h["results"]["Hits@100"][1] == script[i] for i, h in enumerate(out["history"]))
    assert seen[0]["k_list"] == (20, 50, 100) and seen[0]["heart"] is False


def test_fit_evaluates_every_eval_steps_and_runs_out_of_epochs(monkeypatch):
    data, model, score, opt = _stub_setup()
    seen = _scripted(monkeypatch, model, [0.5, 0.4, 0.3, 0.2])
    out = lpformer_amd.fit(model, score, data, opt, epochs=7, eval_steps=2, kill_cnt=100, metric="Hits@20",
                           k_list=(20, 100), heart=True, batch_size=300)
    assert len(seen) == 3 and [("results" in h) for h in out["history"]] == [False, True, False, True, False, True, False]
    assert not out["stopped_early"] and out["best_epoch"] == 6 and out["best_valid"] == 0.7     # Hits@20 = 1 - script
    assert seen[0]["k_list"] == (20, 100) and seen[0]["heart"] is True
    assert [h["lr"] for h in out["history"]] == [0.1] * 7
    with pytest.raises(KeyError):
        lpformer_amd.fit(model, score, data, opt, epochs=1, eval_steps=1, metric="Hits@7", batch_size=300)


# ------------------------------------------------------------------------------------------------ 5. ABI and exports
def test_exports_and_abi():
    assert {"TrainEdges", "train_epoch", "fit"} <= set(lpformer_amd.__all__)
    assert callable(lpformer_amd.train_epoch) and callable(lpformer_amd.fit)
    assert "lpf_batch_cover" in _lib.HIP_PROTOTYPES and len(_lib.HIP_PROTOTYPES["lpf_batch_cover"]) == 11
    assert _lib.ABI_VERSION == 16
