"""lpformer_amd.skipgram on the host: ``skipgram_reference`` (fp64, written out from the contract, no autograd) against
torch autograd of ``_skipgram_loss`` with ``torch.optim.SparseAdam`` on an fp64 ``nn.Embedding(sparse=True)``; the
bad-id rule; that the error bounds the device is held to (tests/skipgram_cases.py) reject wrong results; the
``trainer`` argument of ``node2vec_embeddings`` without a GPU."""
import pytest
import torch

from lpformer_amd import skipgram
from lpformer_amd.random_walks import _skipgram_loss, _windows, node2vec_embeddings
from tests import random_walks_cases as RC
from tests import skipgram_cases as SC

# Both sides are fp64 and differ in summation order only.  Worst absolute differences over the two steps of every case,
# as measured on the CPU: loss 4.4e-16 (= 2^-51), table 2.60e-14, exp_avg 3.9e-17, exp_avg_sq 1.04e-20.  The tolerances
# are the next powers of two above them.  The table's is the widest because the first Adam step is
# lr g / (|g| + eps / sqrt(1 - beta2)): its slope near g = 0 is lr / 3e-7, and a gradient that differs by 1e-19 moves
# the row by 1e-14.
TOL = {"loss": 2.0 ** -50, "table": 2.0 ** -45, "exp_avg": 2.0 ** -54, "exp_avg_sq": 2.0 ** -66}


def _autograd_steps(c, steps):
    emb = torch.nn.Embedding(c.n, c.spec.dim, sparse=True, _weight=c.table.to(torch.float64))
    opt = torch.optim.SparseAdam(list(emb.parameters()), lr=SC.LR)
    ctx = c.spec.context
    pos = _windows(c.pos.t().to(torch.int64), ctx).reshape(-1, ctx)
    neg = _windows(c.neg.t().to(torch.int64), ctx).reshape(-1, ctx)
    for _ in range(steps):
        opt.zero_grad()
        loss = _skipgram_loss(emb, pos, neg)
        loss.backward()
        opt.step()
        st = opt.state[emb.weight]
        yield loss.detach(), emb.weight.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()


@pytest.mark.parametrize("name", SC.GOOD)
def test_reference_equals_autograd_and_sparse_adam_over_two_steps(name):
    c = SC.case(name)
    table, state = c.table.to(torch.float64), skipgram.skipgram_state(c.table.to(torch.float64))
    for step, (loss, weight, m, v) in enumerate(_autograd_steps(c, 2), 1):
        ref = skipgram.skipgram_reference(table, state, c.pos, c.neg, c.spec.context, lr=SC.LR)
        diff = {"loss": abs(float(loss - ref.loss)), "table": float((weight - ref.table).abs().max()),
                "exp_avg": float((m - ref.exp_avg).abs().max()), "exp_avg_sq": float((v - ref.exp_avg_sq).abs().max())}
        print(name, "step", step, diff)
        for k, d in diff.items():
            assert d <= TOL[k], (k, d)
        assert ref.step == step and ref.loss.dtype == torch.float64 and ref.loss.dim() == 0
        # only touched rows moved
        untouched = torch.ones(c.n, dtype=torch.bool)
        untouched[ref.rows] = False
        assert torch.equal(ref.table[untouched], table[untouched]) and not ref.exp_avg[untouched].any()
        table, state = ref.table, skipgram.SkipGramState(ref.exp_avg, ref.exp_avg_sq, ref.step)


def test_cases_cover_what_they_claim():
    for name in SC.NAMES:
        c, ref = SC.case(name), SC.reference(name)
        assert c.pos.shape[1] % 64 and c.pos.stride(0) == c.pos.shape[1] + c.spec.pad
        logit = (c.table.double()[ref.centre.clamp(min=0)] * c.table.double()[ref.other.clamp(min=0)]).sum(1)
        same = ref.centre == ref.other
        assert float(logit[~same].abs().max()) < 8.0, name
        # a pair with c == x has the logit |E[c]|^2, about 0.8 sqrt(dim); none lies where (1 - s) + 1e-15 has lost
        # its digits (tests/skipgram_cases.py)
        assert float(logit.max()) < 25.0, name
    assert {SC.SPECS[k].dim for k in SC.NAMES} >= {4, 36, 128, 512}
    assert any(s.context == 2 for s in SC.SPECS.values()) and any(s.context == s.length + 1 for s in SC.SPECS.values())
    for name in ("star_d128", "iso_d512"):                         # pairs with c == x exist
        ref = SC.reference(name)
        assert ((ref.centre == ref.other) & (ref.centre >= 0)).any(), name
    star = SC.reference("star_d128")
    row, _, _ = SC.occurrences(star)
    assert int((row == 0).sum()) > 8 * SC.CHUNK                    # the hub's segment crosses many chunks


def test_a_bad_id_gives_coefficient_zero_and_indexes_nothing():
    c, ref = SC.case("bad_d36"), SC.reference("bad_d36")
    nwin, per = c.spec.length + 2 - c.spec.context, c.spec.context - 1
    Mp = c.pos.shape[1] * nwin * per
    bad_pos = torch.arange(5 * nwin * per, 6 * nwin * per)         # every pair of positive walk 5 (a row of -1)
    bad_neg = Mp + torch.arange(5 * nwin * per, 5 * nwin * per + per)     # its negative walk: the window of the start
    bad = torch.cat([bad_pos, bad_neg])
    assert (ref.coef[bad] == 0).all() and (ref.centre[bad] == -1).all() and (ref.other[bad] == -1).all()
    good = torch.ones(ref.coef.numel(), dtype=torch.bool)
    good[bad] = False
    assert (ref.coef[good] != 0).all() and (ref.centre[good] >= 0).all()
    assert (ref.rows >= 0).all() and (ref.rows < c.n).all()
    # the bad pairs still count in Mp and Mn: the same walks without walk 5 have a loss larger by the factor W / (W - 1)
    # on the positive side, which is all that is checked here: the mean is over ALL pairs
    keep = torch.arange(c.pos.shape[1]) != 5
    sub = skipgram.skipgram_reference(c.table, skipgram.skipgram_state(c.table), c.pos[:, keep].contiguous(),
                                      c.neg[:, :0].contiguous(), c.spec.context, lr=SC.LR)
    only_pos = skipgram.skipgram_reference(c.table, skipgram.skipgram_state(c.table), c.pos,
                                           c.neg[:, :0].contiguous(), c.spec.context, lr=SC.LR)
    W = c.pos.shape[1]
    assert abs(float(only_pos.loss) * W / (W - 1) - float(sub.loss)) < 1e-12
    # an id far outside the table in the padding of the buffers is never read (a view of a wider buffer)
    assert int(c.pos.untyped_storage().nbytes()) > c.pos.numel() * 4


def test_the_gradient_bound_rejects_wrong_sums():
    """The bound a device gradient row is held to must be tight enough to see one lost occurrence, one coefficient of
    the wrong sign and one skipped chunk.  Case star_d128, hub row 0 (thousands of occurrences, dozens of chunks) --
    the row where the bound is widest relative to a single term.  The damaged occurrence is the one of MEDIAN
    coefficient magnitude in the hub's first chunk.  Not every occurrence would do: a walk that starts at the hub
    comes back to it, its positive pair (hub, hub) has the logit |E[hub]|^2 = 9 and a coefficient of 1e-4 / Mp, and
    losing that occurrence moves the row by less than fp32 resolves (the smallest ratio is printed as well)."""
    c, ref = SC.case("star_d128"), SC.reference("star_d128")
    _, b_g = SC.coef_bound(c, c.table, ref)
    bound = SC.grad_bound(c.table, ref, b_g)[0]                    # rows[0] == 0: the hub
    assert int(ref.rows[0]) == 0
    row, other, pair = SC.occurrences(ref)
    hub = torch.nonzero(row == 0).reshape(-1)
    E = c.table.to(torch.float64)
    terms = ref.coef[pair[hub], None] * E[other[hub]]              # [occurrences of the hub, dim]
    assert float((terms.sum(0) - ref.grad[0]).abs().max()) < 1e-12
    first = terms[:SC.CHUNK]
    print("smallest |term| / bound among the hub's first chunk:", float((first.abs() / bound).max(dim=1).values.min()))
    weakest = int(ref.coef[pair[hub[:SC.CHUNK]]].abs().argsort()[SC.CHUNK // 2])
    for what, damage in (("one occurrence dropped", first[weakest]), ("one coefficient's sign flipped", 2 * first[weakest]),
                         ("one chunk skipped", terms[SC.CHUNK:2 * SC.CHUNK].sum(0))):
        worst = float((damage.abs() / bound).max())
        print(what, "largest |damage| / bound over the row's elements:", worst)
        assert worst > 1.0, what
    # ... and the correct fp32 evaluation in another order sits inside it
    f32 = (ref.coef.to(torch.float32)[pair[hub], None] * c.table[other[hub]]).flip(0).cumsum(0)[-1].to(torch.float64)
    assert ((f32 - ref.grad[0]).abs() <= bound).all()


def test_integer_lists_are_exact_in_fp32():
    p = SC.integer_lists()
    assert tuple(int(b - a) for a, b in zip(p["seg"][:-1], p["seg"][1:])) == SC.EDGE_LENGTHS
    assert float(p["want"].abs().max()) < 2 ** 24 and torch.equal(p["want"], p["want"].round())


def test_device_trainer_needs_a_gpu_source_and_a_supported_dim():
    csr = RC.case("C").csr
    if not torch.cuda.is_available():
        with pytest.raises(ValueError, match="GPU"):
            node2vec_embeddings(csr, 16, walk_length=4, context=3, walks_per_node=1, trainer="device")
    with pytest.raises(ValueError, match="dim"):
        node2vec_embeddings(csr, 6, walk_length=4, context=3, trainer="device")
    with pytest.raises(ValueError, match="dim"):
        node2vec_embeddings(csr, 516, walk_length=4, context=3, trainer="device")
    with pytest.raises(ValueError, match="trainer"):
        node2vec_embeddings(csr, 16, walk_length=4, context=3, trainer="hip")


def test_torch_trainer_stops_after_max_steps():
    csr = RC.case("C").csr
    emb, losses = node2vec_embeddings(csr, 4, walk_length=3, context=2, walks_per_node=1, batch_walks=8, max_steps=2)
    assert emb.shape == (csr.n, 4) and len(losses) == 1 and torch.isfinite(emb).all()
    with pytest.raises(ValueError, match="max_steps"):
        node2vec_embeddings(csr, 4, walk_length=3, context=2, max_steps=0)
