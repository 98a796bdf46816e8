"""Stage E's gather of ``tail_chain_kernel`` (GPU box): ``lpf_tail_chain_rows_perm_ew_f32`` driven directly, bitwise
against the two launches it replaces -- ``lpf_dense_chain_f32`` (in_mode 1: r_e = ReLU(LayerNorm(W_e0 (x_a * x_b) + b_e0)))
followed by ``lpf_tail_chain_rows_perm_f32`` reading that r_e.

Stage E gathers whole rows (8 adjacent lanes per 128-byte line, a wavefront taking 8 of its group's 16 pairs) and hands the
products to its k-loop through LDS, so which lane fetches which pair's ids is no longer the lane that computes on them.
What can go wrong is therefore an id or a piece that lands in another pair's slot, at the ends of a ragged workgroup above
all.  D = 128, the weights of tests/scoring_harness.py, and

* M in {1, 15, 16, 17, 63, 64, 65, 130}: less than a wavefront's share, a group more or less, a workgroup more or less,
  three workgroups with a ragged last one;
* a node table of 7 rows, so ids repeat, a == b occurs, with row strides 128 and 132;
* ids below 0 and >= 7 (they read row 0);
* the order as identity and reversed;
* ``*n_full`` in {0, 1, 63, 64, 65, M}: workgroups without selected nodes, mixed ones taking ``row_empty``, none;
* logit and prob, written by the same launch.
"""
import numpy as np
import pytest
import torch

from lpformer_amd import _lib
from lpformer_amd._lib import check, ptr
from lpformer_amd.ops import raw_stream
from tests import scoring_harness as H

pytestmark = pytest.mark.gpu
DEV = H.DEV
D = 128
N_ROWS = 7
SIZES = (1, 15, 16, 17, 63, 64, 65, 130)


class Tail:
    """The tables of both forms of the tail, built once from the harness' model and left unchanged."""

    def __init__(self):
        model, score, _, _ = H._setup(D, "all", seed=3, bs=128)
        self.model, self.ew = model, model.elementwise_lin
        a, c, self.kpad = model._score_fold(score)
        self.tt = model._tail_tables(score, a, c)
        ew = self.ew
        self.te = ew._chain1.tables(ew.linears[0].weight, ew.linears[0].bias, ew.norm.weight, ew.norm.bias)
        self.ctl = torch.zeros(16, dtype=torch.int64, device=DEV)

    def inputs(self, m, ldx, seed):
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(N_ROWS, ldx, generator=g).to(DEV)[:, :D]
        batch = torch.randint(0, N_ROWS, (2, m), generator=g)
        batch[1, ::5] = batch[0, ::5]                               # a == b
        batch[0, 1::7] = -1 - torch.arange(len(batch[0, 1::7]))     # below 0 -> row 0
        batch[1, 2::7] = N_ROWS + torch.arange(len(batch[1, 2::7])) # >= n_rows -> row 0
        batch[0, m - 1] = N_ROWS - 1                                # (the last pair, the one dead lanes compute on, is no row 0)
        rows = torch.zeros(m, D + 4)
        rows[:, :D + self.model.count_dim] = torch.randn(m, D + self.model.count_dim, generator=g)
        return x, batch.to(DEV), rows.to(DEV)

    def _call(self, name, m, rows, r, perm, n_full, extra):
        tt, out = self.tt, torch.full((2, m), float("nan"), device=DEV)
        check(getattr(_lib.hip(), name)(
            m, D, self.model.count_dim, ptr(rows), rows.stride(0), ptr(tt["wB"]), ptr(tt["bB"]), ptr(tt["lnB_g"]),
            ptr(tt["lnB_b"]), ptr(r), 0 if r is None else r.stride(0), ptr(tt["wC"]), ptr(tt["bC"]), ptr(tt["w_dot"]),
            ptr(tt["b_dot"]), ptr(self.ctl), ptr(perm), ptr(n_full), ptr(tt["bC_empty"]), ptr(tt["row_empty"]), *extra,
            ptr(out[0]), ptr(out[1]), raw_stream(torch.device(DEV))), name)
        return out

    def stage_e(self, m, x, batch, rows, perm, n_full):
        te = self.te
        return self._call("lpf_tail_chain_rows_perm_ew_f32", m, rows, None, perm, n_full,
                          (ptr(x), x.stride(0), ptr(batch), batch.stride(0), x.shape[0], ptr(te["w1p"]), ptr(te["b1"]),
                           ptr(te["ln_g"]), ptr(te["ln_b"])))

    def r_e(self, m, x, batch):
        r = torch.zeros(m, self.kpad, dtype=torch.float32, device=DEV)
        assert self.ew._chain1.run(self.te, x, relu=True, batch=batch, in_mode=1, out=r[:, :D]) is not None
        return r

    def two_launches(self, m, r, rows, perm, n_full):
        return self._call("lpf_tail_chain_rows_perm_f32", m, rows, r, perm, n_full, ())


@pytest.fixture(scope="module")
def tail():
    return Tail()


@pytest.mark.parametrize("m", SIZES)
def test_stage_e_is_bitwise_the_dense_chain_launch(tail, m):
    combos = 0
    for ldx in (128, 132):
        x, batch, rows = tail.inputs(m, ldx, seed=100 * m + ldx)
        assert x.stride(0) == ldx
        r = tail.r_e(m, x, batch)                                   # (one reference r_e per table, shared below)
        for rev in (False, True):
            order = torch.arange(m, dtype=torch.int32)
            perm = (order.flip(0) if rev else order).contiguous().to(DEV)
            for nf in sorted({min(v, m) for v in (0, 1, 63, 64, 65, m)}):
                n_full = torch.tensor([nf], dtype=torch.int64, device=DEV)
                want = tail.two_launches(m, r, rows, perm, n_full)
                got = tail.stage_e(m, x, batch, rows, perm, n_full)
                torch.cuda.synchronize()
                assert torch.isfinite(want).all(), (m, ldx, rev, nf)
                bad = (got.view(torch.int32) != want.view(torch.int32)).nonzero()
                assert bad.numel() == 0, (f"M {m} ldx {ldx} reversed {rev} n_full {nf}: (logit | prob, pair) {bad[:8].tolist()} "
                                          f"differ, by up to {(got - want).abs().max().item():.3e}")
                combos += 1
    assert combos >= 2 * 2 * 2


def test_scores_depend_on_every_gathered_piece(tail):
    """The comparison above would pass if both sides ignored part of a row: changing one float of one table row -- each
    of the 32 pieces in turn -- changes the score of a pair that reads it, and of no pair that does not."""
    m = 65
    x, batch, rows = tail.inputs(m, 132, seed=7)
    perm = torch.arange(m, dtype=torch.int32, device=DEV)
    n_full = torch.tensor([m], dtype=torch.int64, device=DEV)
    base = tail.stage_e(m, x, batch, rows, perm, n_full)[0].clone()
    ids = batch.clone()
    ids[(ids < 0) | (ids >= N_ROWS)] = 0
    reads = ((ids[0] == N_ROWS - 1) | (ids[1] == N_ROWS - 1))
    assert reads.any() and (~reads).any() and bool(reads[m - 1])
    for piece in range(D // 4):
        x2 = x.clone()
        x2[N_ROWS - 1, 4 * piece + piece % 4] += 1.0
        got = tail.stage_e(m, x2, batch, rows, perm, n_full)[0]
        changed = got != base
        assert torch.equal(changed | reads, reads), f"piece {piece}: a pair that does not read the row changed"
        assert changed[reads].any(), f"piece {piece}: no pair that reads the row changed"
