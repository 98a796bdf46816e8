"""The k-loops of ``tail_chain_kernel`` with the weight stream's store, wait and request among a k-group's MFMAs and the
stream running across the stage boundaries (GPU box).

``lpf_tail_chain_rows_perm_ew_f32`` (``fuse_step = "auto"``) and ``lpf_tail_chain_rows_perm_f32`` (``fuse_step = False``)
at D = 128, fp32, on the two-hub graph and ``Case`` of test_gpu_three_launch.py: 1, 63, 64, 65, 128 and 129 pairs of which
0, 1, 64, 65 or all select a node -- an all-short launch, a mixed workgroup, the boundary on a workgroup's edge, and every
stage's first and last k-group with a single live lane.

(a) logits within the fp64 bound test_gpu_tail_boundaries.py applies;
(b) logits BITWISE what the parent commit's library computed for exactly these batches (tests/golden/tail_kloop_parent.npz,
    written once by tools/tail_kloop_record.py with the parent's build; the fixture names the commit): the order of the
    MFMAs into every accumulator did not change;
(c) two launches on two streams bitwise equal.
One D = 64 and one D = 256 batch through ``score_pairs`` against the fp64 restatement: every instantiation's loops changed.
"""
import os

import numpy as np
import pytest
import torch

from tests import scoring_harness as H
from tests import test_gpu_f32_reference as F
from tests.test_gpu_tail_boundaries import EW, PERM, _within_bound
from tests.test_gpu_three_launch import Case

pytestmark = pytest.mark.gpu
DEV = H.DEV
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tail_kloop_parent.npz")
SIZES = (1, 63, 64, 65, 128, 129)
CASES = [(bs, nf) for bs in SIZES for nf in sorted({0, 1, 64, 65, bs}) if nf <= bs]
FORMS = (("auto", EW), (False, PERM))
TAILS = (EW, PERM, "lpf_tail_chain_rows_f32", "lpf_tail_chain_merge_f32", "lpf_tail_chain_f32")


def key(form, bs, n_full):
    return f"{'ew' if form == 'auto' else 'perm'}_{bs}_{n_full}"


class KLoop(Case):
    """``Case`` handing out batches with a given number of pairs that select a node, and their fp64 reference -- computed
    once and left unchanged."""

    def __init__(self):
        super().__init__()
        self._refs = {}

    def batch_of(self, bs, n_full):
        rng = np.random.default_rng(1000 * bs + n_full)
        where = np.zeros(bs, bool)
        where[rng.choice(bs, n_full, replace=False)] = True
        out = torch.empty(2, bs, dtype=torch.int64, device=DEV)
        fi = np.arange(n_full) % self.full.shape[1]                 # (the a == b and repeated pairs first)
        ei = rng.choice(self.empty.shape[1], bs - n_full, replace=True)
        out[:, torch.from_numpy(np.flatnonzero(where)).to(DEV)] = self.full[:, torch.from_numpy(fi).to(DEV)]
        out[:, torch.from_numpy(np.flatnonzero(~where)).to(DEV)] = self.empty[:, torch.from_numpy(ei).to(DEV)]
        return out.contiguous()

    def reference(self, bs, n_full):
        if (bs, n_full) not in self._refs:
            batch = self.batch_of(bs, n_full)
            ref = F._reference(self.model, self.score, batch, self.h)
            assert int((ref["ref"]["counts"].sum(axis=1) > 0).sum()) == n_full     # (the batch is what it was built to be)
            self._refs[(bs, n_full)] = (batch, ref)
        return self._refs[(bs, n_full)]


@pytest.fixture(scope="module")
def case():
    c = KLoop()
    yield c
    c.model.fuse_step = "auto"


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    assert len(str(g["parent_commit"])) >= 7
    return g


@pytest.mark.parametrize("form, kernel", FORMS)
@pytest.mark.parametrize("bs, n_full", CASES)
def test_logits_within_the_fp64_bound_and_bitwise_the_parents(case, golden, monkeypatch, bs, n_full, form, kernel):
    batch, ref = case.reference(bs, n_full)
    reach = H.Reach(monkeypatch, (EW, PERM))
    case.scores(batch, form, True)                          # (sizes the workspaces)
    got, ran = reach.ran(lambda: case.scores(batch, form, True))
    assert ran == {kernel}, ran
    _within_bound(f"[{bs} pairs, {n_full} full] {kernel}", got, ref, 128)
    want = golden[key(form, bs, n_full)]
    got = H._np(got)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
        f"differs from commit {golden['parent_commit']} by {np.abs(got - want).max():.3e}"


@pytest.mark.parametrize("form, kernel", FORMS)
@pytest.mark.parametrize("bs, n_full", CASES)
def test_two_launches_on_two_streams_are_bitwise_equal(case, bs, n_full, form, kernel):
    m = case.model
    batch, _ = case.reference(bs, n_full)
    streams = [torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)]
    for s in streams:                                       # (every stream has workspaces of its own: size them)
        with torch.cuda.stream(s):
            case.scores(batch, form, True)
    torch.cuda.synchronize()
    m.fuse_step = form
    outs = []
    for s in streams:
        with torch.cuda.stream(s):
            outs.append(m.score_pairs(batch, case.h, case.score, logits=True).clone())
    torch.cuda.synchronize()
    assert m.check_selection()
    assert torch.equal(outs[0], outs[1]), f"differ by {(outs[0] - outs[1]).abs().max().item():.3e}"


@pytest.mark.parametrize("dim, seed", [(64, 3), (256, 5)])
def test_other_widths_within_the_fp64_bound(monkeypatch, dim, seed):
    """D = 64 (three workgroups per CU, one weight element per thread and stage) and D = 256 (the r_e loop stays rolled,
    k-groups in pairs): full, mixed and short workgroups through ``lpf_tail_chain_rows_perm_f32``."""
    model, score, _, tb = H._setup(dim, "all", seed=seed, bs=200)
    model.attention_impl = "flip"
    model.use_side_stream = False
    h = model.propagate()
    ref = F._reference(model, score, tb, h)
    cnt = ref["ref"]["counts"].sum(axis=1)
    assert (cnt == 0).sum() > 0 and (cnt > 0).sum() > 64 and (cnt > 0).sum() % 64      # (a mixed workgroup at least)
    reach = H.Reach(monkeypatch, TAILS)
    model.score_pairs(tb, h, score, logits=True)
    assert model.check_selection()
    got, ran = reach.ran(lambda: model.score_pairs(tb, h, score, logits=True))
    assert ran == {PERM} and model.check_selection(), ran
    _within_bound(f"[D = {dim}] rows + perm tail", got, ref, dim)
