"""What the host hands the C ABI per scoring step, across the switches (GPU box): for the THIRD call of every case below
the entry points in issue order, each with its scalar arguments (exact values; a pointer only as ``P`` or None), the
stream it goes to ("main" = the caller's current stream, "side" = the model's side stream of it) and the stream
hand-overs ``("wait", waiter, waited)`` between them; for the first call the entry points' names.  A case the model
refuses is pinned as the exception's type.

tests/test_gpu_selection_order.py pins the names for six configurations; this module pins what a rearrangement of the
host code could change without changing a name: the stream of a launch, a hand-over, a stride, a capacity, a flag.
EXPECTED was printed by ``python -m tests.test_gpu_step_launches`` from the code as it was BEFORE the attention front end
and the tail launch were written once each (commit 4cc733f); the module also prints the SHA-256 of every case's scores.

130 pairs of tests/scoring_harness.py's two-hub graph: three blocks of 64 pairs, the last one ragged, with the hub pair
(> 512 selected nodes) and 102 pairs that select nothing."""
import ctypes
import hashlib

import pytest
import torch

import lpformer_amd
from lpformer_amd import _lib
from lpformer_amd.graphed import GraphedScorer, PlannedScorer
from tests import scoring_harness as H

pytestmark = pytest.mark.gpu
BS = 130
P = "P"        # a pointer argument that is set
_SCALAR_TYPES = tuple(_lib._SCALARS.values())


class _Recorder:
    """The hooks of ``_lib.recording`` (as ``lpformer_amd.graphed._StepRecorder``): launches and hand-overs in issue
    order; nothing is replayed, so no tensor is kept."""

    def __init__(self):
        self.calls = []

    def launch(self, name, fn):
        if name in PlannedScorer._SKIP:   # (pure queries)
            return fn

        def call(*args):
            self.calls.append((name, args))
            return fn(*args)
        return call

    def keep(self, t):
        pass

    def wait(self, waiter, waited):
        self.calls.append((None, (waiter, waited)))


def _entries(calls, main, side):
    """``calls`` of a recorder in the frozen form: ("wait", waiter role, waited role) or (name, stream role, arguments
    but the stream: scalars as they are, pointers as P / None)."""
    def role(raw):
        if raw == main.cuda_stream:
            return "main"
        return "side" if side is not None and raw == side.cuda_stream else "other"

    out = []
    for name, args in calls:
        if name is None:
            out.append(("wait", role(args[0].cuda_stream), role(args[1].cuda_stream)))
            continue
        types = _lib.HIP_PROTOTYPES[name]
        assert len(types) == len(args) and types[-1] is ctypes.c_void_p, name
        vals = tuple((a.item() if hasattr(a, "item") else a) if t in _SCALAR_TYPES else (None if not a else P)
                     for t, a in zip(types[:-1], args[:-1]))
        out.append((name, role(args[-1] or 0), vals))
    return out


def _score_pairs(logits=True, adj=False, head_layers=2):
    def make(model, score, data, batch):
        if head_layers != 2:
            torch.manual_seed(11)
            score = lpformer_amd.mlp_score(2 * model.dim, 2 * model.dim, 1, head_layers).to(H.DEV).eval()
        adj_mask = data["adj_mask"].to_torch_sparse_coo() if adj else None
        h = model.propagate()
        torch.cuda.synchronize()
        return lambda: model.score_pairs(batch, h, score, adj_mask=adj_mask, logits=logits)
    return make


def _calc_pairwise(return_weights=False):
    def make(model, score, data, batch):
        h = model.propagate()
        torch.cuda.synchronize()

        def call():
            out, weights = model.calc_pairwise(batch, h, return_weights=return_weights)
            return out if weights is None else torch.cat([out.reshape(-1), weights.reshape(-1)])
        return call
    return make


def _pair_features(model, score, data, batch):
    h = model.propagate()
    torch.cuda.synchronize()
    return lambda: model.pair_features(batch, h)


# name -> (D, model settings, what makes the call under test); a scorer class instead: see ``_scorer``
CASES = {
    "d128": (128, {}, _score_pairs()),
    "d128_no_side": (128, dict(use_side_stream=False), _score_pairs()),
    "d128_fuse_step": (128, dict(fuse_step=True), _score_pairs()),
    "d128_four_no_side": (128, dict(fuse_step=False, use_side_stream=False), _score_pairs()),
    "d128_no_skip_empty": (128, dict(tail_skip_empty=False), _score_pairs()),
    "d128_general": (128, dict(use_select_index=False), _score_pairs()),
    "d128_general_no_skip_empty": (128, dict(use_select_index=False, tail_skip_empty=False), _score_pairs()),
    "d128_flip_units": (128, dict(attention_impl="flip", attention_rows=False), _score_pairs()),
    "d128_mfma": (128, dict(attention_impl="mfma"), _score_pairs()),
    "d128_bf16": (128, dict(precision="bf16"), _score_pairs()),
    "d128_tail_bf16": (128, dict(tail_precision="bf16"), _score_pairs()),
    "d128_query_gemm": (128, dict(query_from="gemm"), _score_pairs()),
    "d128_no_tail_chain": (128, dict(use_tail_chain=False), _score_pairs()),
    "d128_no_fused_attention": (128, dict(use_fused_attention=False), _score_pairs()),
    "d128_no_fused_no_tail_chain": (128, dict(use_fused_attention=False, use_tail_chain=False), _score_pairs()),
    "d128_prob": (128, {}, _score_pairs(logits=False)),
    "d128_adj_override": (128, dict(use_mask_delta=False), _score_pairs(adj=True)),
    "d128_three_layer_head": (128, {}, _score_pairs(head_layers=3)),
    "d64": (64, {}, _score_pairs()),
    "d64_select3": (64, dict(select4_regions=False), _score_pairs()),
    "d64_bf16": (64, dict(precision="bf16"), _score_pairs()),
    "d256_flip": (256, dict(attention_impl="flip"), _score_pairs()),
    "d256_mfma": (256, dict(attention_impl="mfma"), _score_pairs()),
    "calc_pairwise_d128": (128, {}, _calc_pairwise()),
    "calc_pairwise_d64": (64, {}, _calc_pairwise()),
    "calc_pairwise_weights_d128": (128, {}, _calc_pairwise(return_weights=True)),
    "pair_features_d128": (128, {}, _pair_features),
    "planned_d128": (128, {}, PlannedScorer),
    "graphed_d128": (128, {}, GraphedScorer),
}


def _scorer(cls, model, score, data, batch):
    """A scorer recorded at the defaults and replayed once: (names of the eager step, what the scorer holds -- the plan
    in the frozen form, roles relative to the scorer's stream; a captured graph shows nothing --, its scores)."""
    h = model.propagate()
    torch.cuda.synchronize()
    eager = model.score_pairs(batch, h, score, logits=True).clone()
    assert model.check_selection()
    scorer = cls(model, score, h, batch, logits=True)
    out = scorer(batch)
    assert scorer.check() is True
    assert torch.equal(out, eager)
    plan = []
    if cls is PlannedScorer:
        side = model._side.get(scorer.stream.cuda_stream) if model._side else None
        plan = _entries([(name, args) for name, _, args, _ in scorer._plan], scorer.stream, side)
    return [cls.__name__, scorer.captures], plan, out


def trace(name):
    """(names of the first call's launches, entries of the third call, scores of the third call) of a fresh model in
    configuration ``name``; ("raises", exception type) for a case the model refuses."""
    dim, settings, make = CASES[name]
    model, score, data, batch = H._setup(dim, "all", seed=3, bs=BS)
    for k, v in settings.items():
        setattr(model, k, v)
    if isinstance(make, type):
        return _scorer(make, model, score, data, batch)
    try:
        call = make(model, score, data, batch)
        with _lib.recording(_Recorder()) as rec:
            call()
        first = [n for n, _ in rec.calls if n is not None]
        assert model.check_selection()
        call()
        assert model.check_selection()
        main = torch.cuda.current_stream(model.device)
        with _lib.recording(_Recorder()) as rec:
            out = call()
        assert model.check_selection()
    except (NotImplementedError, ValueError, TypeError) as e:    # (a refusal; a failed launch is no case)
        return "raises", type(e).__name__, None
    side = model._side.get(main.cuda_stream) if model._side else None
    return first, _entries(rec.calls, main, side), out


def digest(t) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


# recorded at the parent of the refactor, see above
EXPECTED = {
    "d128": (
        ["lpf_gemm_f32", "lpf_select4", "lpf_select4", "lpf_select4_regions", "lpf_select4", "lpf_select4_regions",
         "lpf_select_export", "lpf_dense_chain_side_f32", "lpf_gemm_f32", "lpf_select4", "lpf_select4",
         "lpf_select4", "lpf_pair_attention_rows4_f32", "lpf_tail_chain_rows_perm_f32"],
        [
            ("wait", "side", "main"),
            ("lpf_dense_chain_side_f32", "side", (130, 1, "P", 128, "P", 130, 2000, 128, "P", 128, "P", None, 0, "P", "P", 1, None, 0, None, "P", 260, None, "P", 256, 128, "P", 128)),
            ("lpf_select4", "main", (130, "P", 130, 2000, "P", "P", "P", "P", "P", "P", "P", 0, 0, 0.0, 0.0, 0.001, "P", "P", "P", None, "P", 184960, 0)),
            ("wait", "main", "side"),
            ("lpf_pair_attention_rows4_f32", "main", (128, 130, "P", "P", "P", 184960, "P", 256, "P", 128, "P", "P", "P", "P", "P", 770, 17, 7360, 0.000244140625, "P", "P", "P", "P", "P", 4, "P", "P", 4925, "P", 132, "P", "P")),
            ("lpf_tail_chain_rows_perm_f32", "main", (130, 128, 4, "P", 132, "P", "P", "P", "P", "P", 260, "P", "P", "P", "P", "P", "P", "P", "P", "P", "P", None)),
        ]),
    "d128_no_side": (
        ["lpf_select4", "lpf_select4", "lpf_select4_regions", "lpf_select4", "lpf_select4_regions",
         "lpf_select_export", "lpf_gemm_f32", "lpf_gemm_f32", "lpf_select4", "lpf_select4", "lpf_select4_q",
         "lpf_pair_attention_rows4_f32", "lpf_tail_chain_rows_perm_ew_f32"],
        [
            ("lpf_select4_q", "main", (130, "P", 130, 2000, "P", "P", "P", "P", "P", "P", "P", 0, 0, 0.0, 0.0, 0.001, "P", "P", "P", None, "P", 184960, 0, "P", 256, "P", 128, 128)),
            ("lpf_pair_attention_rows4_f32", "main", (128, 130, "P", "P", "P", 184960, "P", 256, "P", 128, "P", "P", "P", "P", "P", 770, 17, 7360, 0.000244140625, "P", "P", "P", "P", "P", 4, "P", "P", 4925, "P", 132, "P", "P")),
            ("lpf_tail_chain_rows_perm_ew_f32", "main", (130, 128, 4, "P", 132, "P", "P", "P", "P", None, 0, "P", "P", "P", "P", "P", "P", "P", "P", "P", "P", 128, "P", 130, 2000, "P", "P", "P", "P", "P", None)),
        ]),
    "d128_fuse_step": (
        ["lpf_select4", "lpf_select4", "lpf_select4_regions", "lpf_select4", "lpf_select4_regions",
         "lpf_select_export", "lpf_gemm_f32", "lpf_gemm_f32", "lpf_select4", "lpf_select4", "lpf_select4_q",
         "lpf_pair_attention_rows4_f32", "lpf_tail_chain_rows_perm_ew_f32"],
        [
            ("lpf_select4_q", "main", (130, "P", 130, 2000, "P", "P", "P", "P", "P", "P", "P", 0, 0, 0.0, 0.0, 0.001, "P", "P", "P", None, "P", 184960, 0, "P", 256, "P", 128, 128)),
            ("lpf_pair_attention_rows4_f32", "main", (128, 130, "P", "P", "P", 184960, "P", 256, "P", 128, "P", "P", "P", "P", "P", 770, 17, 7360, 0.000244140625, "P", "P", "P", "P", "P", 4, "P", "P", 4925, "P", 132, "P", "P")),
            ("lpf_tail_chain_rows_perm_ew_f32", "main", (130, 128, 4, "P", 132, "P", "P", "P", "P", None, 0, "P", "P", "P", "P", "P", "P", "P", "P", "P", "P", 128, "P", 130, 2000, "P", "P", "P", "P", "P", None)),
        ]),
    "d128_four_no_side": (
        ["lpf_gemm_f32", "lpf_select4", "lpf_select4", "lpf_select4_regions", "lpf_select4", "lpf_select4_regions",
         "lpf_select_export", "lpf_dense_chain_side_f32", "lpf_gemm_f32", "lpf_select4", "lpf_select4",
         "lpf_select4", "lpf_pair_attention_rows4_f32", "lpf_tail_chain_rows_perm_f32"],
        [
            ("lpf_dense_chain_side_f32", "main", (130, 1, "P", 128, "P", 130, 2000, 128, "P", 128, "P", None, 0, "P", "P", 1, None, 0, None, "P", 260, None, "P", 256, 128, "P", 128)),
            ("lpf_select4", "main", (130, "P", 130, 2000, "P", "P", "P", "P", "P", "P", "P", 0, 0, 0.0, 0.0, 0.001, "P", "P", "P", None, "P", 184960, 0)),
            ("lpf_pair_attention_rows4_f32", "main", (128, 130, "P", "P", "P", 184960, "P", 256, "P", 128, "P", "P", "P", "P", "P", 770, 17, 7360, 0.000244140625, "P", "P", "P", "P", "P", 4, "P", "P", 4925, "P", 132, "P", "P")),
            ("lpf_tail_chain_rows_perm_f32", "main", (130, 128, 4, "P", 132, "P", "P", "P", "P", "P", 260, "P", "P", "P", "P", "P", "P", "P", "P", "P", "P", None)),
        ]),
    "d128_no_skip_empty": (
        ["lpf_gemm_f32", "lpf_select4", "lpf_select4", "lpf_select4_regions", "lpf_select4", "lpf_select4_regions",
         "lpf_select_export", "lpf_dense_chain_side_f32", "lpf_gemm_f32", "lpf_select4", "lpf_select4",
         "lpf_select4", "lpf_pair_attention_rows4_f32", "lpf_tail_chain_rows_f32"],
        [
            ("wait", "side", "main"),
            ("lpf_dense_chain_side_f32", "side", (130, 1, "P", 128, "P", 130, 2000, 128, "P", 128, "P", None, 0, "P", "P", 1, None, 0, None, "P", 260, None, "P", 256, 128, "P", 128)),
            ("lpf_select4", "main", (130, "P", 130, 2000, "P", "P", "P", "P", "P", "P", "P", 0, 0, 0.0, 0.0, 0.001, "P", "P", "P", None, "P", 184960, 0)),
            ("wait", "main", "side"),
            ("lpf_pair_attention_rows4_f32", "main", (128, 130, "P", "P", "P", 184960, "P", 256, "P", 128, "P", "P", "P", "P", "P", 770, 17, 7360, 0.000244140625, "P", "P", "P", "P", "P", 4, "P", "P", 4925, "P", 132, None, None)),
            ("lpf_tail_chain_rows_f32", "main", (130, 128, 4, "P", 132, "P", "P", "P", "P", "P", 260, "P", "P", "P", "P", "P", "P", None)),
        ]),
    "d128_general": (
        ["lpf_gemm_f32", "lpf_ppr_filter_count", "lpf_ppr_filter_fill", "lpf_select_plan", "lpf_select_run",
         "lpf_select_plan", "lpf_select_run", "lpf_select_export", "lpf_dense_chain_side_f32", "lpf_gemm_f32",
         "lpf_select_plan", "lpf_select_run", "lpf_select_plan", "lpf_select_run",
         "lpf_pair_attention_rows_perm_f32", "lpf_tail_chain_rows_perm_f32"],
        [
            ("wait", "side", "main"),
            ("lpf_dense_chain_side_f32", "side", (130, 1, "P", 128, "P", 130, 2000, 128, "P", 128, "P", None, 0, "P", "P", 1, None, 0, None, "P", 260, None, "P", 256, 128, "P", 128)),
            ("lpf_select_plan", "main", (130, "P", 130, 2000, "P", "P", "P", None, None, "P", "P", "P", "P", 4112, "P", "P")),
            ("lpf_select_run", "main", (130, "P", "P", "P", 4112, "P", "P", "P", None, None, "P", "P", None, "P", "P", 0.0, 0.0, 0.001, 0, "P", "P", 14866, 0)),
            ("wait", "main", "side"),
            ("lpf_pair_attention_rows_perm_f32", "main", (128, 130, "P", "P", 14866, "P", 256, "P", 128, "P", "P", "P", "P", "P", "P", "P", "P", 4, "P", "P", 2789, "P", 132, "P", "P", "P")),
            ("lpf_tail_chain_rows_perm_f32", "main", (130, 128, 4, "P", 132, "P", "P", "P", "P", "P", 260, "P", "P", "P", "P", "P", "P", "P", "P", None, "P", None)),
        ]),
    "d128_general_no_skip_empty": (
        ["lpf_gemm_f32", "lpf_ppr_filter_count", "lpf_ppr_filter_fill", "lpf_select_plan", "lpf_select_run",
         "lpf_select_plan", "lpf_select_run", "lpf_select_export", "lpf_dense_chain_side_f32", "lpf_gemm_f32",
         "lpf_select_plan", "lpf_select_run", "lpf_select_plan", "lpf_select_run", "lpf_pair_attention_rows_f32",
         "lpf_tail_chain_rows_f32"],
        [
            ("wait", "side", "main"),
            ("lpf_dense_chain_side_f32", "side", (130, 1, "P", 128, "P", 130, 2000, 128, "P", 128, "P", None, 0, "P", "P", 1, None, 0, None, "P", 260, None, "P", 256, 128, "P", 128)),
            ("lpf_select_plan", "main", (130, "P", 130, 2000, "P", "P", "P", None, None, "P", "P", "P", "P", 4112, "P", "P")),
            ("lpf_select_run", "main", (130, "P", "P", "P", 4112, "P", "P", "P", None, None, "P", "P", None, "P", "P", 0.0, 0.0, 0.001, 0, "P", "P", 14866, 0)),
            ("wait", "main", "side"),
            ("lpf_pair_attention_rows_f32", "main", (128, 130, "P", "P", 14866, "P", 256, "P", 128, "P", "P", "P", "P", "P", "P", "P", "P", 4, "P", "P", 2789, "P", 132)),
            ("lpf_tail_chain_rows_f32", "main", (130, 128, 4, "P", 132, "P", "P", "P", "P", "P", 260, "P", "P", "P", "P", "P", "P", None)),
        ]),
    "d128_flip_units": (
        ["lpf_gemm_f32", "lpf_dense_chain_side_f32", "lpf_gemm_f32", "lpf_select4", "lpf_select4",
         "lpf_select4_regions", "lpf_select4", "lpf_select4_regions", "lpf_pair_attention_flip_f32",
         "lpf_tail_chain_merge_f32"],
        [
            ("wait", "side", "main"),
            ("lpf_dense_chain_side_f32", "side", (130, 1, "P", 128, "P", 130, 2000, 128, "P", 128, "P", None, 0, "P", "P", 1, None, 0, None, "P", 260, None, "P", 256, 128, "P", 128)),
            ("lpf_select4", "main", (130, "P", 130, 2000, "P", "P", "P", "P", "P", "P", "P", 0, 0, 0.0, 0.0, 0.001, "P", "P", "P", "P", "P", 184960, 0)),
            ("lpf_select4_regions", "main", (130, "P", "P", "P", 184960, "P", "P", 14866, "P")),
            ("wait", "main", "side"),
            ("lpf_pair_attention_flip_f32", "main", (128, 130, "P", "P", 14866, "P", 256, "P", 128, "P", "P", "P", "P", "P", "P", "P", 931)),
            ("lpf_tail_chain_merge_f32", "main", (130, 128, 4, "P", "P", 931, "P", "P", "P", "P", "P", "P", "P", "P", "P", 260, "P", "P", "P", "P", "P", "P", None)),
        ]),
    "d128_mfma": (
        ["lpf_gemm_f32", "lpf_dense_chain_side_f32", "lpf_gemm_f32", "lpf_select4", "lpf_select4",
         "lpf_select4_regions", "lpf_select4", "lpf_select4_regions", "lpf_pair_attention_fused_f32",
         "lpf_tail_chain_merge_f32"],
        [
            ("wait", "side", "main"),
            ("lpf_dense_chain_side_f32", "side", (130, 1, "P", 128, "P", 130, 2000, 128, "P", 128, "P", None, 0, "P", "P", 1, None, 0, None, "P", 260, None, "P", 256, 128, "P", 128)),
            ("lpf_select4", "main", (130, "P", 130, 2000, "P", "P", "P", "P", "P", "P", "P", 0, 0, 0.0, 0.0, 0.001, "P", "P", "P", "P", "P", 184960, 0)),
            ("lpf_select4_regions", "main", (130, "P", "P", "P", 184960, "P", "P", 14866, "P")),
            ("wait", "main", "side"),
            ("lpf_pair_attention_fused_f32", "main", (128, 130, "P", "P", 14866, "P", 256, "P", 128, "P", "P", "P", "P", "P", "P", "P", 931)),
            ("lpf_tail_chain_merge_f32", "main", (130, 128, 4, "P", "P", 931, "P", "P", "P", "P", "P", "P", "P", "P", "P", 260, "P", "P", "P", "P", "P", "P", None)),
        ]),
    "d128_bf16": (
        ["lpf_gemm_f32", "lpf_select4", "lpf_select4", "lpf_select4_regions", "lpf_select4", "lpf_select4_regions",
         "lpf_select_export", "lpf_dense_chain_side_f32", "lpf_gemm_f32", "lpf_select4", "lpf_select4",
         "lpf_select4", "lpf_pair_attention_rows4_zbf16", "lpf_tail_chain_rows_perm_f32"],
        [
            ("wait", "side", "main"),
            ("lpf_dense_chain_side_f32", "side", (130, 1, "P", 128, "P", 130, 2000, 128, "P", 128, "P", None, 0, "P", "P", 1, None, 0, None, "P", 260, None, "P", 256, 128, "P", 128)),
            ("lpf_select4", "main", (130, "P", 130, 2000, "P", "P", "P", "P", "P", "P", "P", 0, 0, 0.0, 0.0, 0.001, "P", "P", "P", None, "P", 184960, 0)),
            ("wait", "main", "side"),
            ("lpf_pair_attention_rows4_zbf16", "main", (128, 130, "P", "P", "P", 184960, "P", 128, "P", 128, "P", "P", "P", "P", "P", 770, 17, 7360, 0.000244140625, "P", "P", "P", "P", "P", 4, "P", "P", 4925, "P", 132, "P", "P")),
            ("lpf_tail_chain_rows_perm_f32", "main", (130, 128, 4, "P", 132, "P", "P", "P", "P", "P", 260, "P", "P", "P", "P", "P", "P", "P", "P", "P", "P", None)),
        ]),
    "d128_tail_bf16": (
        ["lpf_gemm_f32", "lpf_select4", "lpf_select4", "lpf_select4_regions", "lpf_select4", "lpf_select4_regions",
         "lpf_select_export", "lpf_dense_chain_side_f32", "lpf_gemm_f32", "lpf_select4", "lpf_select4",
         "lpf_select4", "lpf_pair_attention_rows4_f32", "lpf_tail_chain_rows_perm_bf16"],
        [
            ("wait", "side", "main"),
            ("lpf_dense_chain_side_f32", "side", (130, 1, "P", 128, "P", 130, 2000, 128, "P", 128, "P", None, 0, "P", "P", 1, None, 0, None, "P", 260, None, "P", 256, 128, "P", 128)),
            ("lpf_select4", "main", (130, "P", 130, 2000, "P", "P", "P", "P", "P", "P", "P", 0, 0, 0.0, 0.0, 0.001, "P", "P", "P", None, "P", 184960, 0)),
            ("wait", "main", "side"),
            ("lpf_pair_attention_rows4_f32", "main", (128, 130, "P", "P", "P", 184960, "P", 256, "P", 128, "P", "P", "P", "P", "P", 770, 17, 7360, 0.000244140625, "P", "P", "P", "P", "P", 4, "P", "P", 4925, "P", 132, "P", "P")),
            ("lpf_tail_chain_rows_perm_bf16", "main", (130, 128, 4, "P", 132, "P", "P", "P", "P", "P", 260, "P", "P", "P", "P", "P", "P", "P", "P", "P", "P", None)),
        ]),
    "d128_query_gemm": (
        ["lpf_select4", "lpf_select4", "lpf_select4_regions", "lpf_select4", "lpf_select4_regions",
         "lpf_select_export", "lpf_dense_chain_f32", "lpf_gemm_f32", "lpf_dense_chain_f32", "lpf_select4",
         "lpf_select4", "lpf_select4", "lpf_pair_attention_rows4_f32", "lpf_tail_chain_rows_perm_f32"],
        [
            ("wait", "side", "main"),
            ("lpf_dense_chain_f32", "side", (130, 1, "P", 128, "P", 130, 2000, 128, "P", 128, "P", None, 0, "P", "P", 1, None, 0, None, "P", 260, None)),
            ("lpf_dense_chain_f32", "side", (130, 2, "P", 128, "P", 130, 2000, 128, "P", 128, "P", None, 0, None, None, 0, None, 0, None, "P", 128, None)),
            ("lpf_select4", "main", (130, "P", 130, 2000, "P", "P", "P", "P", "P", "P", "P", 0, 0, 0.0, 0.0, 0.001, "P", "P", "P", None, "P", 184960, 0)),
            ("wait", "main", "side"),
            ("lpf_pair_attention_rows4_f32", "main", (128, 130, "P", "P", "P", 184960, "P", 128, "P", 128, "P", "P", "P", "P", "P", 770, 17, 7360, 0.000244140625, "P", "P", "P", "P", "P", 4, "P", "P", 4925, "P", 132, "P", "P")),
            ("lpf_tail_chain_rows_perm_f32", "main", (130, 128, 4, "P", 132, "P", "P", "P", "P", "P", 260, "P", "P", "P", "P", "P", "P", "P", "P", "P", "P", None)),
        ]),
    "d128_no_tail_chain": (
        ["lpf_dense_chain_f32", "lpf_select4", "lpf_select4", "lpf_select4_regions", "lpf_select4",
         "lpf_select4_regions", "lpf_select_export", "lpf_gemm_f32", "lpf_pair_gather_f32", "lpf_select4",
         "lpf_select4", "lpf_select4", "lpf_pair_attention_rows4_f32", "lpf_dense_chain_f32", "lpf_dense_chain_f32"],
        [
            ("wait", "side", "main"),
            ("lpf_dense_chain_f32", "side", (130, 1, "P", 128, "P", 130, 2000, 128, "P", 128, "P", None, 0, "P", "P", 1, None, 0, None, "P", 260, None)),
            ("wait", "side", "main"),
            ("lpf_pair_gather_f32", "side", (130, 128, "P", 130, 2000, "P", 256, None, 0, "P", 128)),
            ("lpf_select4", "main", (130, "P", 130, 2000, "P", "P", "P", "P", "P", "P", "P", 0, 0, 0.0, 0.0, 0.001, "P", "P", "P", None, "P", 184960, 0)),
            ("wait", "main", "side"),
            ("lpf_pair_attention_rows4_f32", "main", (128, 130, "P", "P", "P", 184960, "P", 256, "P", 128, "P", "P", "P", "P", "P", 770, 17, 7360, 0.000244140625, "P", "P", "P", "P", "P", 4, "P", "P", 4925, "P", 132, None, None)),
            ("lpf_dense_chain_f32", "main", (130, 0, "P", 132, None, 0, 0, 132, "P", 132, "P", None, 0, "P", "P", 1, None, 0, None, "P", 260, None)),
            ("lpf_dense_chain_f32", "main", (130, 0, "P", 260, None, 0, 0, 260, "P", 256, "P", None, 0, None, None, 1, "P", 1, "P", "P", 0, None)),
        ]),
    "d128_no_fused_attention": (
        ["lpf_dense_chain_f32", "lpf_gemm_f32", "lpf_pair_gather_f32", "lpf_select4", "lpf_select4",
         "lpf_select4_regions", "lpf_select4", "lpf_select4_regions", "lpf_select_export", "lpf_pair_scores_f32",
         "lpf_pair_softmax_gather_f32", "lpf_tail_chain_f32"],
        [
            ("wait", "side", "main"),
            ("lpf_dense_chain_f32", "side", (130, 1, "P", 128, "P", 130, 2000, 128, "P", 128, "P", None, 0, "P", "P", 1, None, 0, None, "P", 260, None)),
            ("wait", "side", "main"),
            ("lpf_pair_gather_f32", "side", (130, 128, "P", 130, 2000, "P", 256, None, 0, "P", 128)),
            ("lpf_select4", "main", (130, "P", 130, 2000, "P", "P", "P", "P", "P", "P", "P", 0, 0, 0.0, 0.0, 0.001, "P", "P", "P", "P", "P", 184960, 0)),
            ("lpf_select4_regions", "main", (130, "P", "P", "P", 184960, "P", "P", 14866, "P")),
            ("lpf_select_export", "main", (130, "P", "P", 14866, "P", "P", 132, 4, "P", "P", "P", "P")),
            ("wait", "main", "side"),
            ("lpf_pair_scores_f32", "main", (128, "P", 130, "P", "P", "P", "P", "P", 256, "P", 128, "P", "P", "P", "P", "P", "P", 6621)),
            ("lpf_pair_softmax_gather_f32", "main", (128, 130, "P", "P", "P", "P", "P", "P", 256, "P", "P", "P", 516, None, "P")),
            ("lpf_tail_chain_f32", "main", (130, 128, 4, "P", 516, "P", "P", "P", "P", 132, "P", "P", "P", "P", "P", 260, "P", "P", "P", "P", "P", None)),
        ]),
    "d128_no_fused_no_tail_chain": (
        ["lpf_dense_chain_f32", "lpf_gemm_f32", "lpf_pair_gather_f32", "lpf_select4", "lpf_select4",
         "lpf_select4_regions", "lpf_select4", "lpf_select4_regions", "lpf_select_export", "lpf_pair_scores_f32",
         "lpf_pair_softmax_gather_f32", "lpf_dense_chain_f32", "lpf_dense_chain_f32", "lpf_dense_chain_f32"],
        [
            ("wait", "side", "main"),
            ("lpf_dense_chain_f32", "side", (130, 1, "P", 128, "P", 130, 2000, 128, "P", 128, "P", None, 0, "P", "P", 1, None, 0, None, "P", 260, None)),
            ("wait", "side", "main"),
            ("lpf_pair_gather_f32", "side", (130, 128, "P", 130, 2000, "P", 256, None, 0, "P", 128)),
            ("lpf_select4", "main", (130, "P", 130, 2000, "P", "P", "P", "P", "P", "P", "P", 0, 0, 0.0, 0.0, 0.001, "P", "P", "P", "P", "P", 184960, 0)),
            ("lpf_select4_regions", "main", (130, "P", "P", "P", 184960, "P", "P", 14866, "P")),
            ("lpf_select_export", "main", (130, "P", "P", 14866, "P", "P", 132, 4, "P", "P", "P", "P")),
            ("wait", "main", "side"),
            ("lpf_pair_scores_f32", "main", (128, "P", 130, "P", "P", "P", "P", "P", 256, "P", 128, "P", "P", "P", "P", "P", "P", 6621)),
            ("lpf_pair_softmax_gather_f32", "main", (128, 130, "P", "P", "P", "P", "P", "P", 256, "P", "P", "P", 516, None, "P")),
            ("lpf_dense_chain_f32", "main", (130, 0, "P", 516, None, 0, 0, 388, "P", 128, "P", "P", 516, "P", "P", 0, None, 0, None, "P", 132, None)),
            ("lpf_dense_chain_f32", "main", (130, 0, "P", 132, None, 0, 0, 132, "P", 132, "P", None, 0, "P", "P", 1, None, 0, None, "P", 260, None)),
            ("lpf_dense_chain_f32", "main", (130, 0, "P", 260, None, 0, 0, 260, "P", 256, "P", None, 0, None, None, 1, "P", 1, "P", "P", 0, None)),
        ]),
    "d128_prob": (
        ["lpf_gemm_f32", "lpf_select4", "lpf_select4", "lpf_select4_regions", "lpf_select4", "lpf_select4_regions",
         "lpf_select_export", "lpf_dense_chain_side_f32", "lpf_gemm_f32", "lpf_select4", "lpf_select4",
         "lpf_select4", "lpf_pair_attention_rows4_f32", "lpf_tail_chain_rows_perm_f32"],
        [
            ("wait", "side", "main"),
            ("lpf_dense_chain_side_f32", "side", (130, 1, "P", 128, "P", 130, 2000, 128, "P", 128, "P", None, 0, "P", "P", 1, None, 0, None, "P", 260, None, "P", 256, 128, "P", 128)),
            ("lpf_select4", "main", (130, "P", 130, 2000, "P", "P", "P", "P", "P", "P", "P", 0, 0, 0.0, 0.0, 0.001, "P", "P", "P", None, "P", 184960, 0)),
            ("wait", "main", "side"),
            ("lpf_pair_attention_rows4_f32", "main", (128, 130, "P", "P", "P", 184960, "P", 256, "P", 128, "P", "P", "P", "P", "P", 770, 17, 7360, 0.000244140625, "P", "P", "P", "P", "P", 4, "P", "P", 4925, "P", 132, "P", "P")),
            ("lpf_tail_chain_rows_perm_f32", "main", (130, 128, 4, "P", 132, "P", "P", "P", "P", "P", 260, "P", "P", "P", "P", "P", "P", "P", "P", "P", None, "P")),
        ]),
    "d128_adj_override": (
        ["lpf_gemm_f32", "lpf_select4", "lpf_select4", "lpf_select4_regions", "lpf_select4", "lpf_select4_regions",
         "lpf_select_export", "lpf_dense_chain_side_f32", "lpf_gemm_f32", "lpf_ppr_filter_count",
         "lpf_ppr_filter_fill", "lpf_select_plan", "lpf_select_run", "lpf_select_plan", "lpf_select_run",
         "lpf_pair_attention_rows_perm_f32", "lpf_tail_chain_rows_perm_f32"],
        [
            ("wait", "side", "main"),
            ("lpf_dense_chain_side_f32", "side", (130, 1, "P", 128, "P", 130, 2000, 128, "P", 128, "P", None, 0, "P", "P", 1, None, 0, None, "P", 260, None, "P", 256, 128, "P", 128)),
            ("lpf_select_plan", "main", (130, "P", 130, 2000, "P", "P", "P", "P", None, "P", "P", "P", "P", 4112, "P", "P")),
            ("lpf_select_run", "main", (130, "P", "P", "P", 4112, "P", "P", "P", None, "P", "P", "P", None, "P", "P", 0.0, 0.0, 0.001, 0, "P", "P", 14866, 0)),
            ("wait", "main", "side"),
            ("lpf_pair_attention_rows_perm_f32", "main", (128, 130, "P", "P", 14866, "P", 256, "P", 128, "P", "P", "P", "P", "P", "P", "P", "P", 4, "P", "P", 2789, "P", 132, "P", "P", "P")),
            ("lpf_tail_chain_rows_perm_f32", "main", (130, 128, 4, "P", 132, "P", "P", "P", "P", "P", 260, "P", "P", "P", "P", "P", "P", "P", "P", None, "P", None)),
        ]),
    "d128_three_layer_head": (
        ["lpf_dense_chain_f32", "lpf_select4", "lpf_select4", "lpf_select4_regions", "lpf_select4",
         "lpf_select4_regions", "lpf_select_export", "lpf_gemm_f32", "lpf_pair_gather_f32", "lpf_select4",
         "lpf_select4", "lpf_select4", "lpf_pair_attention_rows4_f32", "lpf_dense_chain_f32", "lpf_gemm_f32",
         "lpf_gemm_f32", "lpf_rowdot_sigmoid_f32"],
        [
            ("wait", "side", "main"),
            ("lpf_dense_chain_f32", "side", (130, 1, "P", 128, "P", 130, 2000, 128, "P", 128, "P", None, 0, "P", "P", 1, "P", 128, "P", "P", 256, None)),
            ("wait", "side", "main"),
            ("lpf_pair_gather_f32", "side", (130, 128, "P", 130, 2000, "P", 256, None, 0, "P", 128)),
            ("lpf_select4", "main", (130, "P", 130, 2000, "P", "P", "P", "P", "P", "P", "P", 0, 0, 0.0, 0.0, 0.001, "P", "P", "P", None, "P", 184960, 0)),
            ("wait", "main", "side"),
            ("lpf_pair_attention_rows4_f32", "main", (128, 130, "P", "P", "P", 184960, "P", 256, "P", 128, "P", "P", "P", "P", "P", 770, 17, 7360, 0.000244140625, "P", "P", "P", "P", "P", 4, "P", "P", 4925, "P", 132, None, None)),
            ("lpf_dense_chain_f32", "main", (130, 0, "P", 132, None, 0, 0, 132, "P", 132, "P", None, 0, "P", "P", 1, "P", 128, "P", "P", 256, None)),
            ("lpf_gemm_f32", "main", (130, 256, 256, "P", 256, "P", 256, "P", None, 0, "P", 256, 1)),
            ("lpf_gemm_f32", "main", (130, 256, 256, "P", 256, "P", 256, "P", None, 0, "P", 256, 1)),
            ("lpf_rowdot_sigmoid_f32", "main", (130, 256, "P", 256, "P", 0.05874919891357422, "P", None)),
        ]),
    "d64": (
        ["lpf_gemm_f32", "lpf_dense_chain_side_f32", "lpf_gemm_f32", "lpf_select4", "lpf_select4",
         "lpf_select4_regions", "lpf_select4", "lpf_select4_regions", "lpf_pair_attention_fused_f32",
         "lpf_tail_chain_merge_f32"],
        [
            ("wait", "side", "main"),
            ("lpf_dense_chain_side_f32", "side", (130, 1, "P", 64, "P", 130, 2000, 64, "P", 64, "P", None, 0, "P", "P", 1, None, 0, None, "P", 132, None, "P", 128, 64, "P", 64)),
            ("lpf_select4", "main", (130, "P", 130, 2000, "P", "P", "P", "P", "P", "P", "P", 0, 0, 0.0, 0.0, 0.001, "P", "P", "P", "P", "P", 184960, 0)),
            ("lpf_select4_regions", "main", (130, "P", "P", "P", 184960, "P", "P", 14866, "P")),
            ("wait", "main", "side"),
            ("lpf_pair_attention_fused_f32", "main", (64, 130, "P", "P", 14866, "P", 128, "P", 64, "P", "P", "P", "P", "P", "P", "P", 931)),
            ("lpf_tail_chain_merge_f32", "main", (130, 64, 4, "P", "P", 931, "P", "P", "P", "P", "P", "P", "P", "P", "P", 132, "P", "P", "P", "P", "P", "P", None)),
        ]),
    "d64_select3": (
        ["lpf_gemm_f32", "lpf_dense_chain_side_f32", "lpf_gemm_f32", "lpf_select3_plan", "lpf_select3_run",
         "lpf_select3_plan", "lpf_select3_run", "lpf_pair_attention_fused_f32", "lpf_tail_chain_merge_f32"],
        [
            ("wait", "side", "main"),
            ("lpf_dense_chain_side_f32", "side", (130, 1, "P", 64, "P", 130, 2000, 64, "P", 64, "P", None, 0, "P", "P", 1, None, 0, None, "P", 132, None, "P", 128, 64, "P", 64)),
            ("lpf_select3_plan", "main", (130, "P", 130, 2000, "P", "P", "P", "P", "P", 0, 0, "P", "P", "P", 4112, "P", "P")),
            ("lpf_select3_run", "main", (130, "P", "P", "P", 4112, "P", "P", "P", "P", 0.0, 0.0, 0.001, 0, "P", "P", 14866, 0)),
            ("wait", "main", "side"),
            ("lpf_pair_attention_fused_f32", "main", (64, 130, "P", "P", 14866, "P", 128, "P", 64, "P", "P", "P", "P", "P", "P", "P", 931)),
            ("lpf_tail_chain_merge_f32", "main", (130, 64, 4, "P", "P", 931, "P", "P", "P", "P", "P", "P", "P", "P", "P", 132, "P", "P", "P", "P", "P", "P", None)),
        ]),
    "d64_bf16": (
        ["lpf_gemm_f32", "lpf_dense_chain_side_f32", "lpf_gemm_f32", "lpf_select4", "lpf_select4",
         "lpf_select4_regions", "lpf_select4", "lpf_select4_regions", "lpf_pair_attention_fused_bf16",
         "lpf_tail_chain_merge_f32"],
        [
            ("wait", "side", "main"),
            ("lpf_dense_chain_side_f32", "side", (130, 1, "P", 64, "P", 130, 2000, 64, "P", 64, "P", None, 0, "P", "P", 1, None, 0, None, "P", 132, None, "P", 128, 64, "P", 64)),
            ("lpf_select4", "main", (130, "P", 130, 2000, "P", "P", "P", "P", "P", "P", "P", 0, 0, 0.0, 0.0, 0.001, "P", "P", "P", "P", "P", 184960, 0)),
            ("lpf_select4_regions", "main", (130, "P", "P", "P", 184960, "P", "P", 14866, "P")),
            ("wait", "main", "side"),
            ("lpf_pair_attention_fused_bf16", "main", (64, 130, "P", "P", 14866, "P", 64, "P", 64, "P", "P", "P", "P", "P", "P", "P", 931)),
            ("lpf_tail_chain_merge_f32", "main", (130, 64, 4, "P", "P", 931, "P", "P", "P", "P", "P", "P", "P", "P", "P", 132, "P", "P", "P", "P", "P", "P", None)),
        ]),
    "d256_flip": (
        ["lpf_gemm_f32", "lpf_select4", "lpf_select4", "lpf_select4_regions", "lpf_select4", "lpf_select4_regions",
         "lpf_select_export", "lpf_dense_chain_side_f32", "lpf_gemm_f32", "lpf_select4", "lpf_select4",
         "lpf_select4", "lpf_pair_attention_rows4_f32", "lpf_tail_chain_rows_perm_f32"],
        [
            ("wait", "side", "main"),
            ("lpf_dense_chain_side_f32", "side", (130, 1, "P", 256, "P", 130, 2000, 256, "P", 256, "P", None, 0, "P", "P", 1, None, 0, None, "P", 516, None, "P", 256, 256, "P", 256)),
            ("lpf_select4", "main", (130, "P", 130, 2000, "P", "P", "P", "P", "P", "P", "P", 0, 0, 0.0, 0.0, 0.001, "P", "P", "P", None, "P", 184960, 0)),
            ("wait", "main", "side"),
            ("lpf_pair_attention_rows4_f32", "main", (256, 130, "P", "P", "P", 184960, "P", 256, "P", 256, "P", "P", "P", "P", "P", 770, 17, 7360, 0.000244140625, "P", "P", "P", "P", "P", 4, "P", "P", 4925, "P", 260, "P", "P")),
            ("lpf_tail_chain_rows_perm_f32", "main", (130, 256, 4, "P", 260, "P", "P", "P", "P", "P", 516, "P", "P", "P", "P", "P", "P", "P", "P", "P", "P", None)),
        ]),
    "d256_mfma": (
        ["lpf_dense_chain_f32", "lpf_gemm_f32", "lpf_gemm_f32", "lpf_pair_gather_f32", "lpf_select4", "lpf_select4",
         "lpf_select4_regions", "lpf_select4", "lpf_select4_regions", "lpf_pair_attention_fused_f32",
         "lpf_pair_attention_merge_f32", "lpf_tail_chain_rows_f32"],
        [
            ("wait", "side", "main"),
            ("lpf_dense_chain_f32", "side", (130, 1, "P", 256, "P", 130, 2000, 256, "P", 256, "P", None, 0, "P", "P", 1, None, 0, None, "P", 516, None)),
            ("wait", "side", "main"),
            ("lpf_pair_gather_f32", "side", (130, 256, "P", 130, 2000, "P", 256, None, 0, "P", 256)),
            ("lpf_select4", "main", (130, "P", 130, 2000, "P", "P", "P", "P", "P", "P", "P", 0, 0, 0.0, 0.0, 0.001, "P", "P", "P", "P", "P", 184960, 0)),
            ("lpf_select4_regions", "main", (130, "P", "P", "P", 184960, "P", "P", 14866, "P")),
            ("wait", "main", "side"),
            ("lpf_pair_attention_fused_f32", "main", (256, 130, "P", "P", 14866, "P", 256, "P", 256, "P", "P", "P", "P", "P", "P", "P", 931)),
            ("lpf_pair_attention_merge_f32", "main", (130, 256, 4, "P", "P", 931, "P", "P", "P", "P", "P", "P", 260)),
            ("lpf_tail_chain_rows_f32", "main", (130, 256, 4, "P", 260, "P", "P", "P", "P", "P", 516, "P", "P", "P", "P", "P", "P", None)),
        ]),
    "calc_pairwise_d128": (
        ["lpf_select4", "lpf_select4", "lpf_select4_regions", "lpf_select4", "lpf_select4_regions",
         "lpf_select_export", "lpf_gemm_f32", "lpf_pair_gather_f32", "lpf_select4", "lpf_select4", "lpf_select4",
         "lpf_pair_attention_rows4_f32", "lpf_dense_chain_f32"],
        [
            ("wait", "side", "main"),
            ("lpf_pair_gather_f32", "side", (130, 128, "P", 130, 2000, "P", 256, None, 0, "P", 128)),
            ("lpf_select4", "main", (130, "P", 130, 2000, "P", "P", "P", "P", "P", "P", "P", 0, 0, 0.0, 0.0, 0.001, "P", "P", "P", None, "P", 184960, 0)),
            ("wait", "main", "side"),
            ("lpf_pair_attention_rows4_f32", "main", (128, 130, "P", "P", "P", 184960, "P", 256, "P", 128, "P", "P", "P", "P", "P", 770, 17, 7360, 0.000244140625, "P", "P", "P", "P", "P", 4, "P", "P", 4925, "P", 132, None, None)),
            ("lpf_dense_chain_f32", "main", (130, 0, "P", 132, None, 0, 0, 132, "P", 132, "P", None, 0, "P", "P", 1, "P", 128, "P", "P", 128, None)),
        ]),
    "calc_pairwise_d64": (
        ["lpf_gemm_f32", "lpf_pair_gather_f32", "lpf_select4", "lpf_select4", "lpf_select4_regions", "lpf_select4",
         "lpf_select4_regions", "lpf_pair_attention_fused_f32", "lpf_pair_attention_merge_f32", "lpf_dense_chain_f32"],
        [
            ("wait", "side", "main"),
            ("lpf_pair_gather_f32", "side", (130, 64, "P", 130, 2000, "P", 128, None, 0, "P", 64)),
            ("lpf_select4", "main", (130, "P", 130, 2000, "P", "P", "P", "P", "P", "P", "P", 0, 0, 0.0, 0.0, 0.001, "P", "P", "P", "P", "P", 184960, 0)),
            ("lpf_select4_regions", "main", (130, "P", "P", "P", 184960, "P", "P", 14866, "P")),
            ("wait", "main", "side"),
            ("lpf_pair_attention_fused_f32", "main", (64, 130, "P", "P", 14866, "P", 128, "P", 64, "P", "P", "P", "P", "P", "P", "P", 931)),
            ("lpf_pair_attention_merge_f32", "main", (130, 64, 4, "P", "P", 931, "P", "P", "P", "P", "P", "P", 68)),
            ("lpf_dense_chain_f32", "main", (130, 0, "P", 68, None, 0, 0, 68, "P", 68, "P", None, 0, "P", "P", 1, "P", 64, "P", "P", 64, None)),
        ]),
    "calc_pairwise_weights_d128": (
        ["lpf_gemm_f32", "lpf_pair_gather_f32", "lpf_select4", "lpf_select4", "lpf_select4_regions", "lpf_select4",
         "lpf_select4_regions", "lpf_select_export", "lpf_pair_scores_f32", "lpf_pair_softmax_gather_f32",
         "lpf_dense_chain_f32", "lpf_dense_chain_f32"],
        [
            ("wait", "side", "main"),
            ("lpf_pair_gather_f32", "side", (130, 128, "P", 130, 2000, "P", 256, None, 0, "P", 128)),
            ("lpf_select4", "main", (130, "P", 130, 2000, "P", "P", "P", "P", "P", "P", "P", 0, 0, 0.0, 0.0, 0.001, "P", "P", "P", "P", "P", 184960, 0)),
            ("lpf_select4_regions", "main", (130, "P", "P", "P", 184960, "P", "P", 14866, "P")),
            ("lpf_select_export", "main", (130, "P", "P", 14866, "P", "P", 132, 4, "P", "P", "P", "P")),
            ("wait", "main", "side"),
            ("lpf_pair_scores_f32", "main", (128, "P", 130, "P", "P", "P", "P", "P", 256, "P", 128, "P", "P", "P", "P", "P", "P", 6621)),
            ("lpf_pair_softmax_gather_f32", "main", (128, 130, "P", "P", "P", "P", "P", "P", 256, "P", "P", "P", 516, "P", "P")),
            ("lpf_dense_chain_f32", "main", (130, 0, "P", 516, None, 0, 0, 388, "P", 128, "P", "P", 516, "P", "P", 0, None, 0, None, "P", 132, None)),
            ("lpf_dense_chain_f32", "main", (130, 0, "P", 132, None, 0, 0, 132, "P", 132, "P", None, 0, "P", "P", 1, "P", 128, "P", "P", 128, None)),
        ]),
    "pair_features_d128": (
        ["lpf_dense_chain_f32", "lpf_select4", "lpf_select4", "lpf_select4_regions", "lpf_select4",
         "lpf_select4_regions", "lpf_select_export", "lpf_gemm_f32", "lpf_pair_gather_f32", "lpf_select4",
         "lpf_select4", "lpf_select4", "lpf_pair_attention_rows4_f32", "lpf_dense_chain_f32"],
        [
            ("wait", "side", "main"),
            ("lpf_dense_chain_f32", "side", (130, 1, "P", 128, "P", 130, 2000, 128, "P", 128, "P", None, 0, "P", "P", 1, "P", 128, "P", "P", 256, None)),
            ("wait", "side", "main"),
            ("lpf_pair_gather_f32", "side", (130, 128, "P", 130, 2000, "P", 256, None, 0, "P", 128)),
            ("lpf_select4", "main", (130, "P", 130, 2000, "P", "P", "P", "P", "P", "P", "P", 0, 0, 0.0, 0.0, 0.001, "P", "P", "P", None, "P", 184960, 0)),
            ("wait", "main", "side"),
            ("lpf_pair_attention_rows4_f32", "main", (128, 130, "P", "P", "P", 184960, "P", 256, "P", 128, "P", "P", "P", "P", "P", 770, 17, 7360, 0.000244140625, "P", "P", "P", "P", "P", 4, "P", "P", 4925, "P", 132, None, None)),
            ("lpf_dense_chain_f32", "main", (130, 0, "P", 132, None, 0, 0, 132, "P", 132, "P", None, 0, "P", "P", 1, "P", 128, "P", "P", 256, None)),
        ]),
    "planned_d128": (
        ["PlannedScorer", 1],
        [
            ("wait", "side", "main"),
            ("lpf_dense_chain_side_f32", "side", (130, 1, "P", 128, "P", 130, 2000, 128, "P", 128, "P", None, 0, "P", "P", 1, None, 0, None, "P", 260, None, "P", 256, 128, "P", 128)),
            ("lpf_select4", "main", (130, "P", 130, 2000, "P", "P", "P", "P", "P", "P", "P", 0, 0, 0.0, 0.0, 0.001, "P", "P", "P", None, "P", 184960, 0)),
            ("wait", "main", "side"),
            ("lpf_pair_attention_rows4_f32", "main", (128, 130, "P", "P", "P", 184960, "P", 256, "P", 128, "P", "P", "P", "P", "P", 770, 17, 7360, 0.000244140625, "P", "P", "P", "P", "P", 4, "P", "P", 4925, "P", 132, "P", "P")),
            ("lpf_tail_chain_rows_perm_f32", "main", (130, 128, 4, "P", 132, "P", "P", "P", "P", "P", 260, "P", "P", "P", "P", "P", "P", "P", "P", "P", "P", None)),
        ]),
    "graphed_d128": (
        ["GraphedScorer", 1],
        []),
}


@pytest.mark.parametrize("name", list(CASES))
def test_launches_arguments_and_streams_of_a_step(name):
    first, third, out = trace(name)
    want_first, want_third = EXPECTED[name]
    assert first == want_first
    if first == "raises":
        assert third == want_third
        return
    assert len(third) == len(want_third), [e[0] for e in third]
    for i, (got, want) in enumerate(zip(third, want_third)):
        assert got == want, f"entry {i}"
    if out is not None:
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())


if __name__ == "__main__":
    print("EXPECTED = {")
    sums = {}
    for case in CASES:
        a, b, scores = trace(case)
        sums[case] = None if scores is None else digest(scores)
        if a == "raises":
            print(f"    {case!r}: ({a!r}, {b!r}),")
            continue
        print(f"    {case!r}: (\n        {a!r},\n        [" + "".join(f"\n            {e!r}," for e in b) +
              ("\n        ]" if b else "]") + "),", flush=True)
    print("}")
    for case, s in sums.items():
        print("SHA256", case, s)
