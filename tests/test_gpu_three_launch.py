"""The three-launch step of the fp32, D = 128 hot path (GPU box): ``lpf_select4_q`` -> ``lpf_pair_attention_rows4_f32`` ->
``lpf_tail_chain_rows_perm_ew_f32`` against the four-launch step it replaces (``fuse_step = False``: the elementwise
layer and the query gather in ``lpf_dense_chain_side_f32``, r_e and q through memory).  The model runs without its side
stream, as under ``bench.py``'s rotation over streams: that is where ``fuse_step = "auto"`` takes the new step.

Stage E of the tail restates dense_chain.hip's layer 1 operation for operation and stage C keeps its summation order, so
logits and probabilities are compared BITWISE; so are the query rows the selection writes (``Y[a] + Y[b]``, for the pairs
that kept an entry -- the others' rows must stay untouched) and everything else the selection leaves.  Batches of 1, 63,
64, 65 and 200 pairs on the small two-hub graph of tests/scoring_harness.py, composed so that the pairs with selected
nodes are none, all, or a number that is no multiple of the tail's 64-pair workgroup (a mixed workgroup with lanes that
take the constant row, and workgroups of pairs without selected nodes behind it), with a == b and repeated pairs."""
import numpy as np
import pytest
import torch

import lpformer_amd
from lpformer_amd import _lib
from lpformer_amd.profile import KernelTimer
from tests import scoring_harness as H

pytestmark = pytest.mark.gpu
DEV = H.DEV
SIZES = (1, 63, 64, 65, 200)
CASES = [(bs, comp) for bs in SIZES for comp in ("none", "all", "mixed") if not (bs == 1 and comp == "mixed")]
NEW = ("lpf_select4_q", "lpf_tail_chain_rows_perm_ew_f32")
OLD = ("lpf_select4", "lpf_dense_chain_side_f32", "lpf_tail_chain_rows_perm_f32")


class Case:
    """One model (D = 128, fp32, thresholds of mask mode "all"), its encoder output and a pool of pairs sorted by whether
    they select a node -- decided by the selection itself, once."""

    def __init__(self):
        self.model, self.score, self.data, pool = H._setup(128, "all", seed=3, bs=700)
        m = self.model
        m.attention_impl = "flip"
        m.PT_EXACT_MAX = float("inf")
        m.use_side_stream = False     # (one stream per step, as under the bench's rotation: what "auto" fuses)
        self.h = m.propagate()
        assert m._uses_select4() and m._uses_rows()
        pool = pool.clone()
        pool[:, :4] = torch.tensor([[0, 5, 0, 0], [0, 5, 1, 1]], device=DEV)      # a == b (hub, plain node), a repeated pair
        ws = m._select4_device(pool, False)
        assert m.check_selection()
        has = (ws.pair_tab.view(-1, 4)[:pool.shape[1], 1:].sum(1) > 0).cpu().numpy()
        assert has[:4].all() and has.sum() >= 200 and (~has).sum() >= 50
        self.full, self.empty = pool[:, torch.from_numpy(np.flatnonzero(has)).to(DEV)], \
            pool[:, torch.from_numpy(np.flatnonzero(~has)).to(DEV)]

    def batch(self, bs, comp, shift=0):
        """[2, bs] ids with ``n_full`` pairs that select a node (first the a == b and repeated ones), spread over the batch;
        returns (batch, n_full)."""
        n_full = {"none": 0, "all": bs, "mixed": 70 if bs == 200 else bs // 2 + 1}[comp]
        assert comp != "mixed" or (0 < n_full < bs and n_full % 64)
        rng = np.random.default_rng(100 * bs + len(comp) + shift)
        where = np.zeros(bs, bool)
        where[rng.choice(bs, n_full, replace=False)] = True
        out = torch.empty(2, bs, dtype=torch.int64, device=DEV)
        fi = (np.arange(n_full) + shift) % self.full.shape[1]
        fi[:min(4, n_full)] = np.arange(min(4, n_full))
        ei = rng.choice(self.empty.shape[1], bs - n_full, replace=True)            # (repeats among these too)
        out[:, torch.from_numpy(np.flatnonzero(where)).to(DEV)] = self.full[:, torch.from_numpy(fi).to(DEV)]
        out[:, torch.from_numpy(np.flatnonzero(~where)).to(DEV)] = self.empty[:, torch.from_numpy(ei).to(DEV)]
        return out.contiguous(), n_full

    def scores(self, batch, form, logits):
        m = self.model
        m.fuse_step = form
        for _attempt in range(3):
            out = m.score_pairs(batch, self.h, self.score, logits=logits).clone()
            if m.check_selection():
                return out
        raise AssertionError("the selection workspace could not be sized")


@pytest.fixture(scope="module")
def case():
    c = Case()
    yield c
    c.model.fuse_step = "auto"


@pytest.mark.parametrize("bs, comp", CASES)
def test_three_launches_score_bitwise_what_four_do(case, monkeypatch, bs, comp):
    batch, _ = case.batch(bs, comp)
    reach = H.Reach(monkeypatch, NEW + OLD)
    case.scores(batch, "auto", True)                        # (sizes the workspaces: not counted below)
    new_l, ran_new = reach.ran(lambda: case.scores(batch, "auto", True))
    new_p = case.scores(batch, "auto", False)
    old_l, ran_old = reach.ran(lambda: case.scores(batch, False, True))
    old_p = case.scores(batch, False, False)
    assert ran_new == set(NEW), ran_new
    assert ran_old == set(OLD), ran_old
    assert torch.isfinite(new_l).all()
    assert torch.equal(new_l, old_l), f"logits differ by {(new_l - old_l).abs().max().item():.3e}"
    assert torch.equal(new_p, old_p), f"probabilities differ by {(new_p - old_p).abs().max().item():.3e}"


@pytest.mark.parametrize("bs, comp", CASES)
def test_selection_writes_the_query_of_pairs_with_entries_only(case, bs, comp):
    m = case.model
    batch, n_full = case.batch(bs, comp)
    y = m._node_y(case.h, m._fold())
    m._select4_device(batch, False)                          # (sizes the workspace)
    assert m.check_selection()
    ws = m._select4_device(batch, False)
    torch.cuda.synchronize()
    tab0, cnt0, ent0 = ws.pair_tab.view(-1, 4)[:bs].clone(), ws.blk_cnt.clone(), ws.entries.view(-1, 4).clone()
    mark = float(np.float32(-12345.0))
    q = torch.full((bs, 128), mark, dtype=torch.float32, device=DEV)
    ws = m._select4_device(batch, False, q=(y, q))
    assert m.check_selection()
    tab1, cnt1, ent1 = ws.pair_tab.view(-1, 4)[:bs], ws.blk_cnt, ws.entries.view(-1, 4)
    has = tab0[:, 1:].sum(1) > 0
    assert int(has.sum()) == n_full                          # (the batch is what it was built to be)
    assert torch.equal(tab0[:, 1:], tab1[:, 1:]) and torch.equal(cnt0, cnt1)
    assert torch.equal(has, tab1[:, 1:].sum(1) > 0)
    # entries: a pair's run starts where its table entry says (where a block lands is the allocation's business)
    for p in torch.nonzero(has).flatten().tolist():
        s0, s1, k = int(tab0[p, 0]), int(tab1[p, 0]), int(tab0[p, 1:].sum())
        assert torch.equal(ent0[s0:s0 + k], ent1[s1:s1 + k]), p
    want = y[batch[0]] + y[batch[1]]
    assert torch.equal(q[has], want[has])
    assert (q[~has] == mark).all(), "a pair without entries got a query row"


@pytest.mark.parametrize("bs, comp", CASES)
def test_recorded_plan_and_captured_graph_replay_the_new_step(case, monkeypatch, bs, comp):
    other = {"none": "all", "all": "none" if bs == 1 else "mixed", "mixed": "none"}[comp]
    b0, _ = case.batch(bs, comp)
    b1, _ = case.batch(bs, other, shift=17)
    eager = [case.scores(b, "auto", True) for b in (b0, b1)]
    case.model.fuse_step = "auto"
    reach = H.Reach(monkeypatch, NEW + OLD)
    plan = lpformer_amd.PlannedScorer(case.model, case.score, case.h, b0, logits=True)
    graph = lpformer_amd.GraphedScorer(case.model, case.score, case.h, b0, logits=True)
    assert reach.calls[NEW[1]] > 0 and reach.calls[OLD[2]] == 0 and reach.calls[OLD[1]] == 0
    for b, want in zip((b0, b1, b0), (eager[0], eager[1], eager[0])):
        out_p, out_g = plan(b).clone(), graph(b).clone()
        torch.cuda.synchronize()
        assert plan.check() and graph.check()
        assert torch.equal(out_p, want), "recorded plan != eager"
        assert torch.equal(out_g, want), "captured graph != eager"


@pytest.mark.parametrize("bs", (65, 200))
def test_overflow_is_nan_in_both_forms(case, bs):
    """The existing, handled overflow -- an entry buffer too small for the batch: sticky bit, NaN scores,
    ``check_selection()`` false -- looks the same from both forms; the next call sizes the buffer again."""
    m = case.model
    batch, _ = case.batch(bs, "mixed")
    good = case.scores(batch, "auto", True)
    for form in ("auto", False):
        m.fuse_step = form
        ws = m._ws[("sel4", torch.cuda.current_stream().cuda_stream, bs)]
        ws.ensure(ent_cap=8, shrink=True)
        out = m.score_pairs(batch, case.h, case.score, logits=True)
        assert torch.isnan(out).all(), form
        assert not m.check_selection(), form
        again = m.score_pairs(batch, case.h, case.score, logits=True)
        assert m.check_selection() and torch.equal(again, good), form


def _spans(model, score, h, batch):
    model.score_pairs(batch, h, score)
    assert model.check_selection()
    KernelTimer.reset()
    KernelTimer.enabled = True
    try:
        model.score_pairs(batch, h, score)
        return set(KernelTimer.summary())
    finally:
        KernelTimer.enabled = False
        KernelTimer.reset()


def test_other_configurations_keep_their_launches(case):
    """D = 64 and the bf16 precision mode still run the elementwise branch's own launch; the fp32 D = 128 step has none,
    unless ``fuse_step`` is off."""
    m = case.model
    batch, _ = case.batch(200, "mixed")
    m.fuse_step = "auto"
    assert "dense_chain_mlp_hidden" not in _spans(m, case.score, case.h, batch)
    m.fuse_step = False
    assert "dense_chain_mlp_hidden" in _spans(m, case.score, case.h, batch)
    m.fuse_step = "auto"
    m.precision = m.tail_precision = "bf16"
    try:
        assert "dense_chain_mlp_hidden" in _spans(m, case.score, case.h, batch)
    finally:
        m.precision = m.tail_precision = "f32"
    # ... and with the side stream on "auto" keeps the step with the elementwise launch on it
    m.use_side_stream = True
    try:
        assert m.fuse_step == "auto" and not m._three_launches(case.h, None)
        m.fuse_step = True
        assert m._three_launches(case.h, None)
    finally:
        m.use_side_stream, m.fuse_step = False, "auto"
    m64, s64, _, b64 = H._setup(64, "all", seed=3, bs=200)
    m64.use_side_stream = False
    assert m64.fuse_step == "auto"
    assert "dense_chain_mlp_hidden" in _spans(m64, s64, m64.propagate(), b64)


def test_unsupported_width_is_reported_not_run():
    """A shape without an instantiation of stage E returns LPF_ERR_UNSUPPORTED before anything is launched (the caller
    then takes the four-launch path)."""
    lib = _lib.hip()
    t = torch.zeros(64, dtype=torch.float32, device=DEV)
    i = torch.zeros(64, dtype=torch.int64, device=DEV)
    p = t.data_ptr()
    rc = lib.lpf_tail_chain_rows_perm_ew_f32(1, 64, 4, p, 68, p, p, p, p, None, 0, p, p, p, p, None, i.data_ptr(),
                                             i.data_ptr(), p, p, p, 64, i.data_ptr(), 1, 1, p, p, p, p, p, None, None)
    assert rc == _lib.CONST["LPF_ERR_UNSUPPORTED"]
