"""The host's launch order around the selection workspaces (GPU box): which ``lpf_*`` entry points a FIRST call of a
(stream, batch size) issues -- workspace construction, the first-batch sizing with its token launches, then the step --
and which a third call issues, for every selection form (pair-major ``lpf_select4``; ``lpf_select4`` +
``lpf_select4_regions``; ``lpf_select3_plan / _run``; the general ``lpf_select_plan / _run``, with and without an
adjacency override).  The lists below were recorded from the code as it was BEFORE the workspaces, their sizing and their
status protocol moved into ``lpformer_amd/selection.py``; that module reproduces them entry for entry.

130 pairs of tests/scoring_harness.py's two-hub graph: three blocks of 64 pairs, the last one ragged, with the hub pair
(> 512 selected nodes) and 102 pairs that select nothing.  The same runs also pin that sizing leaves no trace in the
results: a model whose workspaces were dropped and sized again scores bit for bit what it scored before."""
import pytest
import torch

from lpformer_amd import _lib
from lpformer_amd.graphed import PlannedScorer
from tests import scoring_harness as H

pytestmark = pytest.mark.gpu
BS = 130
WATCHED = tuple(n for n in _lib.HIP_PROTOTYPES if n not in PlannedScorer._SKIP)   # (every launch; not the pure queries)


def _score_pairs(model, score, data, batch):
    h = model.propagate()
    torch.cuda.synchronize()

    def call():
        out = model.score_pairs(batch, h, score, logits=True)
        assert model.check_selection()
        return (out,)
    return call


def _node_mask(model, score, data, batch):
    model.use_mask_delta = False                      # (the override is a graph of its own: general path)
    adj = data["adj_mask"].to_torch_sparse_coo()

    def call():
        return tuple(t for info in model.compute_node_mask(batch, adj=adj) if info is not None for t in info)
    return call


def _calc_pairwise(model, score, data, batch):
    h = model.propagate()
    torch.cuda.synchronize()

    def call():
        out = model.calc_pairwise(batch, h)[0]
        assert model.check_selection()
        return (out,)
    return call


# name -> (D, model settings, the call under test)
CONFIGS = {
    "score_pairs_d128": (128, {}, _score_pairs),
    "score_pairs_d64": (64, {}, _score_pairs),
    "score_pairs_select3": (64, dict(select4_regions=False), _score_pairs),
    "score_pairs_general": (128, dict(use_select_index=False), _score_pairs),
    "node_mask_override": (128, {}, _node_mask),
    "calc_pairwise_d128": (128, {}, _calc_pairwise),
}


def trace(name, monkeypatch):
    """(launches of the first call, launches of the third call, results of the third call, results of a call after the
    workspaces were dropped) of a fresh model in configuration ``name``."""
    dim, settings, make = CONFIGS[name]
    model, score, data, batch = H._setup(dim, "all", seed=3, bs=BS)
    for k, v in settings.items():
        setattr(model, k, v)
    call = make(model, score, data, batch)
    reach = H.Reach(monkeypatch, WATCHED)
    call()
    first = list(reach.log)
    call()
    del reach.log[:]
    kept = tuple(t.clone() for t in call())
    third = list(reach.log)
    model._ws.clear()                                 # fresh workspaces: sized again by the next call
    again = call()
    torch.cuda.synchronize()
    return first, third, kept, again


_S4_SIZING = ["lpf_select4", "lpf_select4"]                                         # token buffer, sized buffer
_REGIONS_SIZING = ["lpf_select4", "lpf_select4", "lpf_select4_regions"]             # select4 alone, then both on token regions
_REGIONS = ["lpf_select4", "lpf_select4_regions"]
_SELECT3 = ["lpf_select3_plan", "lpf_select3_run"]
_GENERAL = ["lpf_select_plan", "lpf_select_run"]
_T0_INDEX = ["lpf_ppr_filter_count", "lpf_ppr_filter_fill"]                         # the general path's >1-hop index
# what `_patterns_pay` looks at once per parameter version at D = 128: a type-major selection of a sample (sized like
# any first batch), exported
_PATTERN_SAMPLE = _REGIONS_SIZING + _REGIONS + ["lpf_select_export"]
_PATTERN_SAMPLE_GENERAL = _T0_INDEX + _GENERAL + _GENERAL + ["lpf_select_export"]

# name -> (launches of the first call, launches of the third call), recorded before lpformer_amd/selection.py existed
EXPECTED = {
    "score_pairs_d128": (
        ["lpf_gemm_f32"] + _PATTERN_SAMPLE + ["lpf_dense_chain_side_f32", "lpf_gemm_f32"] + _S4_SIZING
        + ["lpf_select4", "lpf_pair_attention_rows4_f32", "lpf_tail_chain_rows_perm_f32"],
        ["lpf_dense_chain_side_f32", "lpf_select4", "lpf_pair_attention_rows4_f32", "lpf_tail_chain_rows_perm_f32"]),
    "score_pairs_d64": (
        ["lpf_gemm_f32", "lpf_dense_chain_side_f32", "lpf_gemm_f32"] + _REGIONS_SIZING + _REGIONS
        + ["lpf_pair_attention_fused_f32", "lpf_tail_chain_merge_f32"],
        ["lpf_dense_chain_side_f32"] + _REGIONS + ["lpf_pair_attention_fused_f32", "lpf_tail_chain_merge_f32"]),
    "score_pairs_select3": (
        ["lpf_gemm_f32", "lpf_dense_chain_side_f32", "lpf_gemm_f32"] + _SELECT3 + _SELECT3
        + ["lpf_pair_attention_fused_f32", "lpf_tail_chain_merge_f32"],
        ["lpf_dense_chain_side_f32"] + _SELECT3 + ["lpf_pair_attention_fused_f32", "lpf_tail_chain_merge_f32"]),
    "score_pairs_general": (
        ["lpf_gemm_f32"] + _PATTERN_SAMPLE_GENERAL + ["lpf_dense_chain_side_f32", "lpf_gemm_f32"] + _GENERAL + _GENERAL
        + ["lpf_pair_attention_rows_perm_f32", "lpf_tail_chain_rows_perm_f32"],
        ["lpf_dense_chain_side_f32"] + _GENERAL + ["lpf_pair_attention_rows_perm_f32", "lpf_tail_chain_rows_perm_f32"]),
    "node_mask_override": (
        _T0_INDEX + _GENERAL + _GENERAL + ["lpf_select_export"],
        _GENERAL + ["lpf_select_export"]),
    "calc_pairwise_d128": (
        _PATTERN_SAMPLE + ["lpf_gemm_f32", "lpf_pair_gather_f32"] + _S4_SIZING
        + ["lpf_select4", "lpf_pair_attention_rows4_f32", "lpf_dense_chain_f32"],
        ["lpf_pair_gather_f32", "lpf_select4", "lpf_pair_attention_rows4_f32", "lpf_dense_chain_f32"]),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_launch_order_of_the_first_and_of_a_later_call(name, monkeypatch):
    first, third, kept, again = trace(name, monkeypatch)
    want_first, want_third = EXPECTED[name]
    assert first == want_first
    assert third == want_third
    assert len(kept) == len(again) and len(kept) > 0
    for a, b in zip(kept, again):
        assert a.shape == b.shape and torch.equal(a, b), "sizing the workspaces again changed a result"
