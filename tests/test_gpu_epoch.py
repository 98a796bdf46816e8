"""The training epoch on the GPU: lpf_batch_cover against the CPU restatement position by position, the mask of
TrainEdges against the reference's masked tensor (bitwise) where RemovedEdges(edges) differs, train_epoch against the
hand-written reference-shaped loop (bitwise), and a seeded run with the dropouts on.  python -m pytest tests -m gpu."""
import numpy as np
import pytest
import torch

import lpformer_amd
from oracle.ref_shims import SparseTensor
from tests import epoch_cases as EC
from tests.test_gpu_train import _build, _load

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E6, N6 = 301, 40


# ------------------------------------------------------------------------------------------------------ 6. the kernel
@pytest.fixture(scope="module")
def rows6():
    tp = EC.random_rows_with_duplicates(E6, N6, seed=11)
    te = lpformer_amd.TrainEdges(tp, N6)
    assert tp.shape == (E6, 2) and int((te.mult >= 2).sum()) >= 40 and int((te.mult == 1).sum()) >= 100
    lo = tp.min(1).values * N6 + tp.max(1).values
    fwd = tp[:, 0] * N6 + tp[:, 1]
    # pairs held in both directions exist
    both = set(fwd[tp[:, 0] < tp[:, 1]].tolist()) & set((tp[:, 1] * N6 + tp[:, 0])[tp[:, 0] > tp[:, 1]].tolist())
    assert len(both) >= 10 and lo.numel() == E6
    return tp


def _both(tp, perm):
    """(device result, stats, cnt clean) and the CPU restatement's of one call on fresh objects."""
    dev, cpu = lpformer_amd.TrainEdges(tp, N6, device=DEV), lpformer_amd.TrainEdges(tp, N6)
    out = dev.covered(perm.to(DEV))
    want = cpu.covered(perm)
    return out, dev.stats(check_range=False), bool(dev.cnt.any()), want, cpu.stats(check_range=False)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 257, 301])
def test_batch_cover_matches_the_restatement_position_by_position(rows6, B):
    perm = torch.randperm(E6, generator=torch.Generator().manual_seed(B))[:B]
    out, stats, dirty, want, want_stats = _both(rows6, perm)
    assert out.dtype == torch.int64 and out.shape == (2, B) and out.device.type == "cuda"
    assert torch.equal(out.cpu(), want) and stats == want_stats and not dirty
    assert stats[0] + stats[1] == B and stats[2] == 0
    assert np.array_equal(want.numpy(), EC.brute_force_covered(rows6.numpy(), perm.numpy()))
    if B == E6:
        assert stats[0] == E6                      # every row in the batch: every edge removed
    elif B >= 63:
        assert stats[0] > 0 and stats[1] > 0       # both outcomes occur


def test_batch_cover_counts_across_workgroups(rows6):
    """The two rows of a pair at batch positions 0 and B - 1, B = 257: counted and emitted by different workgroups."""
    te = lpformer_amd.TrainEdges(rows6, N6)
    g = int(torch.nonzero(te.mult == 2)[0])
    r0, r1 = torch.nonzero(te.gid == g).flatten().tolist()
    rest = torch.tensor([r for r in torch.randperm(E6, generator=torch.Generator().manual_seed(7)).tolist()
                         if r not in (r0, r1)][:255])
    perm = torch.cat([torch.tensor([r0]), rest, torch.tensor([r1])])
    assert perm.numel() == 257
    out, stats, dirty, want, want_stats = _both(rows6, perm)
    assert torch.equal(out.cpu(), want) and stats == want_stats and not dirty
    pair = sorted(rows6[r0].tolist())
    assert out[:, 0].tolist() == pair and out[:, 256].tolist() == pair
    # with the twin left out the first position is held back
    out2, _, _, want2, _ = _both(rows6, perm[:256])
    assert torch.equal(out2.cpu(), want2) and out2[:, 0].tolist() == [-1, -1]


def test_batch_cover_skips_and_counts_row_ids_out_of_range(rows6):
    perm = torch.randperm(E6, generator=torch.Generator().manual_seed(3))[:130].clone()
    bad = perm.clone()
    bad[5], bad[70] = E6, -1
    te = lpformer_amd.TrainEdges(rows6, N6, device=DEV)
    out = te.covered(bad.to(DEV))
    stats = te.stats(check_range=False)
    assert stats[2] == 2 and stats[0] + stats[1] == 128 and not bool(te.cnt.any())
    assert out[:, 5].tolist() == [-1, -1] and out[:, 70].tolist() == [-1, -1]
    cpu = lpformer_amd.TrainEdges(rows6, N6)
    assert torch.equal(out.cpu(), cpu.covered(bad)) and cpu.stats(check_range=False) == stats
    # every other position is what the batch without the two rows gives
    keep = torch.ones(130, dtype=torch.bool)
    keep[5] = keep[70] = False
    want = EC.brute_force_covered(rows6.numpy(), perm[keep].numpy())
    assert np.array_equal(out.cpu().numpy()[:, keep.numpy()], want)
    with pytest.raises(IndexError):
        te.stats()


def test_two_calls_in_a_row_on_one_stream(rows6):
    g = torch.Generator().manual_seed(21)
    p1, p2 = torch.randperm(E6, generator=g)[:200], torch.randperm(E6, generator=g)[:77]
    te = lpformer_amd.TrainEdges(rows6, N6, device=DEV)
    o1 = te.covered(p1.to(DEV))
    o2 = te.covered(p2.to(DEV))                     # (no synchronisation in between: the reset is in stream order)
    o3 = te.covered(p1.to(DEV))
    w1, w2 = lpformer_amd.TrainEdges(rows6, N6).covered(p1), lpformer_amd.TrainEdges(rows6, N6).covered(p2)
    assert torch.equal(o1.cpu(), w1) and torch.equal(o2.cpu(), w2) and torch.equal(o3.cpu(), w1)
    e1, e2 = int((w1[0] >= 0).sum()), int((w2[0] >= 0).sum())
    assert te.stats() == [2 * e1 + e2, 2 * (200 - e1) + 77 - e2, 0, 0] and not bool(te.cnt.any())


# ------------------------------------------------------------------------------------- 7. / 8. / 9. the model's mask
class _Case:
    pass


@pytest.fixture(scope="module")
def dup_case():
    """The train_step_d64 graph; train_pos = its 900 undirected edges plus 20 duplicate rows (10 of them reversed), so the
    typing adjacency is unchanged.  ``batch``: 64 rows with one row of 6 duplicated pairs (twin outside), both rows of 3
    others, and 52 unique rows."""
    c = _Case()
    c.z, c.cfg = _load("train_step_d64")
    n = c.n = c.cfg["n"]
    ei = c.z["edge_index"].astype(np.int64)
    base = ei[:, ei[0] < ei[1]].T.copy()
    rng = np.random.default_rng(17)
    d = rng.choice(base.shape[0], 20, replace=False)
    dup = base[d].copy()
    dup[:10] = dup[:10, ::-1]
    c.train_pos = torch.from_numpy(np.concatenate([base, dup]))
    nb = base.shape[0]
    unique_rows = np.setdiff1d(np.arange(nb), d)
    held = d[[0, 1, 2, 10, 11, 12]]                                    # base rows whose twins (nb + k) stay outside
    full = np.concatenate([d[[3, 4, 13]], nb + np.array([3, 4, 13])])  # both rows of three pairs
    batch = np.concatenate([held, full, rng.choice(unique_rows, 64 - held.size - full.size, replace=False)])
    c.batch = torch.from_numpy(batch[rng.permutation(64)])
    c.held_pairs = {tuple(sorted(r)) for r in base[held].tolist()}
    c.full_pairs = {tuple(sorted(r)) for r in base[d[[3, 4, 13]]].tolist()}
    removed = EC.brute_force_removed(c.train_pos.numpy(), c.batch.numpy())
    assert len(c.held_pairs) == 6 and not (c.held_pairs & removed) and c.full_pairs <= removed and len(removed) == 55
    return c


def _masked_adj(train_pos, perm, n):
    """The reference's per-batch typing adjacency (src/train/train_model.py:40-44), as tests/test_gpu_train.py builds it."""
    adjmask = torch.ones(train_pos.shape[0], dtype=torch.bool)
    adjmask[perm] = False
    keep = train_pos[adjmask].t()
    masked = SparseTensor.from_edge_index(keep, sparse_sizes=(n, n)).to_symmetric()
    return masked.to_torch_sparse_coo_tensor().coalesce().bool().int()


def test_mask_is_the_reference_tensor_where_removed_edges_is_not(dup_case):
    c = dup_case
    model, score = _build(c.z, c.cfg)
    te = lpformer_amd.TrainEdges(c.train_pos, c.n, device=DEV)
    te.check_against(model)
    perm = c.batch.to(DEV)
    edges = te.train_pos[perm].t()
    masked_adj = _masked_adj(c.train_pos, c.batch, c.n)
    got_pairs = {(int(a), int(b)) for a, b in te.covered(perm).t().tolist() if a >= 0}
    assert got_pairs == EC.brute_force_removed(c.train_pos.numpy(), c.batch.numpy())
    assert te.stats()[:2] == [58, 6]
    model.train()
    score.train()
    h_mask = model(edges, adj_mask=te.mask(perm)).detach()
    h_ref = model(edges, adj_mask=masked_adj).detach()
    h_named = model(edges, adj_mask=lpformer_amd.RemovedEdges(edges)).detach()
    h_plain = model(edges).detach()
    assert torch.isfinite(h_ref).all() and h_ref.shape == (64, model.out_dim)
    assert torch.equal(h_mask, h_ref)
    # RemovedEdges(edges) also removes the six pairs whose twin rows stay in the adjacency: another selection
    assert not torch.equal(h_named, h_ref) and not torch.equal(h_plain, h_ref)
    held_pos = [i for i, r in enumerate(edges.t().tolist()) if tuple(sorted(r)) in c.held_pairs]
    assert len(held_pos) == 6
    differs = (h_named != h_ref).any(dim=1).nonzero().flatten().tolist()
    assert set(differs) & set(held_pos)
    # the same in eval() through the inference kernels
    model.eval()
    with torch.no_grad():
        x = model.propagate()
        p_mask, _ = model.calc_pairwise(edges, x, adj_mask=te.mask(perm))
        p_ref, _ = model.calc_pairwise(edges, x, adj_mask=masked_adj)
        p_named, _ = model.calc_pairwise(edges, x, adj_mask=lpformer_amd.RemovedEdges(edges))
    assert torch.equal(p_mask, p_ref) and not torch.equal(p_named, p_ref)


def test_train_epoch_equals_the_hand_written_loop(dup_case):
    c = dup_case
    n = c.n
    rng = torch.Generator().manual_seed(5)
    others = torch.tensor(np.setdiff1d(np.arange(c.train_pos.shape[0]), c.batch.numpy()))
    others = others[torch.randperm(others.numel(), generator=rng)]
    batches = [c.batch, others[:64], others[64:101]]                    # 64 / 64 / 37 rows
    negs = [torch.randint(0, n, (2, b.numel()), generator=rng).to(DEV) for b in batches]

    def fresh():
        model, score = _build(c.z, c.cfg)
        opt = torch.optim.Adam(list(model.parameters()) + list(score.parameters()), lr=5e-3)
        return model, score, opt
    # the epoch driver
    model, score, opt = fresh()
    data = {"train_pos": c.train_pos, "num_nodes": n}
    steps = []
    loss = lpformer_amd.train_epoch(model, score, data, opt, batches=batches, negatives=lambda i, e: negs[i],
                                    on_step=lambda i, l: steps.append(l.clone()))
    # the reference-shaped loop with masked tensors (tests/test_gpu_train.py::test_train_epoch_shaped_loop_runs_and_learns)
    model2, score2, opt2 = fresh()
    train_pos = c.train_pos.to(DEV)
    steps2 = []
    model2.train()
    score2.train()
    for perm, neg_edges in zip(batches, negs):
        masked_adj = _masked_adj(c.train_pos, perm, n)
        edges = train_pos[perm.to(DEV)].t()
        h = model2(edges, adj_prop=None, adj_mask=masked_adj)
        pos_loss = -torch.log(score2(h) + 1e-6).mean()
        neg_loss = -torch.log(1 - score2(model2(neg_edges)) + 1e-6).mean()
        l2 = pos_loss + neg_loss
        l2.backward()
        torch.nn.utils.clip_grad_norm_(model2.parameters(), 1.0)
        torch.nn.utils.clip_grad_norm_(score2.parameters(), 1.0)
        opt2.step()
        opt2.zero_grad()
        steps2.append(l2.detach().clone())
    assert len(steps) == 3 and all(torch.equal(a, b) for a, b in zip(steps, steps2))
    for (k, p), (k2, p2) in zip(list(model.named_parameters()) + list(score.named_parameters()),
                                list(model2.named_parameters()) + list(score2.named_parameters())):
        assert k == k2 and torch.equal(p, p2), k
    sizes = [b.numel() for b in batches]
    assert loss == sum(float(l) * b for l, b in zip(steps, sizes)) / sum(sizes)
    assert float(steps[0]) != float(steps[2])
    te = data[lpformer_amd.epoch._CACHE_KEY][1]
    assert te.device.type == "cuda" and te.stats()[2] == 0 and not bool(te.cnt.any())


def test_train_epoch_with_dropouts_learns_and_repeats_under_a_seed(dup_case):
    c = dup_case
    cfg = dict(c.cfg, att_drop=0.1, dropout=0.1, gnn_drop=0.1, feat_drop=0.1)

    def run():
        model, score = _build(c.z, cfg)
        score.dropout = 0.1
        opt = torch.optim.Adam(list(model.parameters()) + list(score.parameters()), lr=5e-3)
        data = {"train_pos": c.train_pos, "num_nodes": c.n}
        torch.manual_seed(0)
        losses = [lpformer_amd.train_epoch(model, score, data, opt, batch_size=128) for _ in range(6)]
        return model, score, losses
    model, score, losses = run()
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    model.eval()
    score.eval()
    with torch.no_grad():
        p = score(model(c.train_pos[:64].t().to(DEV)))
    assert torch.isfinite(p).all() and p.shape == (64,)
    _, _, again = run()
    assert again == losses
