"""The stage boundaries of ``tail_chain_kernel`` (GPU box): the LayerNorm exchanges with a slot and a single barrier each,
the boundary vectors (biases, LayerNorm weights, ``w_dot``) staged in LDS, stage A's rows requested ahead of their use.

D = 128, fp32, side stream off, on the two-hub graph of tests/scoring_harness.py with the batches of
test_gpu_three_launch.py's ``Case``: 1, 63, 65, 129 and 200 pairs, of which none, all, or a number that is no multiple of
the tail's 64-pair workgroup select a node -- the last gives a mixed workgroup (lanes that take the constant row) with
workgroups of pairs without selected nodes behind it.

* Logits of the three-launch step against the fp64 restatement within the per-row bound of tests/f32_error_model.py, with
  the constants test_gpu_f32_reference.py holds the tails to.  This is the anchor outside the kernel family: the bitwise
  comparison of three launches against four shares the kernel template on both sides.
* The same batch scored five times, alternating over two streams with a different batch in flight on the other stream:
  bitwise equal every time.  A LayerNorm exchange read before its barrier, or a slot written twice, shows here.
* One case through ``lpf_tail_chain_rows_perm_f32`` (``fuse_step = False``) and one at D = 256, whose instantiations
  took the same changes.
"""
import numpy as np
import pytest
import torch

from tests import scoring_harness as H
from tests import test_gpu_f32_reference as F
from tests.test_gpu_three_launch import Case

pytestmark = pytest.mark.gpu
DEV = H.DEV
SIZES = (1, 63, 65, 129, 200)
CASES = [(bs, comp) for bs in SIZES for comp in ("none", "all", "mixed") if not (bs == 1 and comp == "mixed")]
EW = "lpf_tail_chain_rows_perm_ew_f32"
PERM = "lpf_tail_chain_rows_perm_f32"


class Boundaries(Case):
    """``Case`` with the fp64 reference of every batch it hands out, computed once and left unchanged."""

    def __init__(self):
        super().__init__()
        self._refs = {}

    def reference(self, bs, comp):
        key = (bs, comp)
        if key not in self._refs:
            batch, n_full = self.batch(bs, comp)
            ref = F._reference(self.model, self.score, batch, self.h)
            assert int((ref["ref"]["counts"].sum(axis=1) > 0).sum()) == n_full     # (the batch is what it was built to be)
            self._refs[key] = (batch, ref)
        return self._refs[key]


@pytest.fixture(scope="module")
def case():
    c = Boundaries()
    yield c
    c.model.fuse_step = "auto"


def _within_bound(tag, got, ref, dim):
    err = np.abs(H._np(got).astype(np.float64) - ref["logit"])
    bound = F._logit_bound(ref, "rows", dim, F.C_TAIL[dim])
    worst = float((err / bound).max())
    print(f"{tag}: max |got - ref| {err.max():.3e}, worst err / bound {worst:.3f}")
    assert np.isfinite(H._np(got)).all() and worst <= 1.0, f"{tag}: {err.max():.3e} beyond the bound ({worst:.2f})"


@pytest.mark.parametrize("bs, comp", CASES)
def test_three_launch_logits_within_the_fp64_bound(case, monkeypatch, bs, comp):
    batch, ref = case.reference(bs, comp)
    reach = H.Reach(monkeypatch, (EW, PERM))
    case.scores(batch, "auto", True)                        # (sizes the workspaces)
    got, ran = reach.ran(lambda: case.scores(batch, "auto", True))
    assert ran == {EW}, ran
    _within_bound(f"[{bs} {comp}] three launches", got, ref, 128)


@pytest.mark.parametrize("bs, comp", [(1, "all"), (63, "mixed"), (65, "mixed"), (129, "mixed"), (200, "mixed"), (200, "all"),
                                      (129, "none")])
def test_repeats_over_two_streams_are_bitwise_equal(case, bs, comp):
    m = case.model
    other = {"none": "all", "all": "none" if bs == 1 else "mixed", "mixed": "all"}[comp]
    b0, _ = case.batch(bs, comp)
    b1, _ = case.batch(bs, other, shift=17)
    want = case.scores(b0, "auto", True)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)]
    for s in streams:                                       # (every stream has workspaces of its own: size them)
        with torch.cuda.stream(s):
            case.scores(b0, "auto", True)
            case.scores(b1, "auto", True)
    torch.cuda.synchronize()
    m.fuse_step = "auto"
    outs = []
    for i in range(5):
        with torch.cuda.stream(streams[(i + 1) % 2]):
            m.score_pairs(b1, case.h, case.score, logits=True)        # in flight next to ...
        with torch.cuda.stream(streams[i % 2]):
            outs.append(m.score_pairs(b0, case.h, case.score, logits=True).clone())
    torch.cuda.synchronize()
    assert m.check_selection()
    for i, out in enumerate(outs):
        assert torch.equal(out, want), f"run {i}: differs by {(out - want).abs().max().item():.3e}"


def test_four_launch_tail_within_the_fp64_bound(case, monkeypatch):
    """``fuse_step = False``: the same template without stage E (r_e read from memory, rows requested in stage A)."""
    batch, ref = case.reference(200, "mixed")
    reach = H.Reach(monkeypatch, (EW, PERM))
    case.scores(batch, False, True)
    got, ran = reach.ran(lambda: case.scores(batch, False, True))
    assert ran == {PERM}, ran
    _within_bound("[200 mixed] four launches", got, ref, 128)
    batch, ref = case.reference(129, "none")
    _within_bound("[129 none] four launches", case.scores(batch, False, True), ref, 128)


def test_d256_tail_within_the_fp64_bound(monkeypatch):
    """D = 256 (one workgroup per CU, two pieces of the boundary vectors per thread): full, mixed and short workgroups."""
    model, score, _, tb = H._setup(256, "all", seed=5, bs=200)
    model.attention_impl = "flip"
    model.use_side_stream = False
    h = model.propagate()
    ref = F._reference(model, score, tb, h)
    cnt = ref["ref"]["counts"].sum(axis=1)
    assert (cnt == 0).sum() > 64 and (cnt > 0).sum() > 64 and (cnt > 0).sum() % 64
    reach = H.Reach(monkeypatch, (EW, PERM))
    model.score_pairs(tb, h, score, logits=True)
    assert model.check_selection()
    got, ran = reach.ran(lambda: model.score_pairs(tb, h, score, logits=True))
    assert ran == {PERM} and model.check_selection(), ran
    _within_bound("[D = 256] rows + perm tail", got, ref, 256)
