"""Dataset files -> ``lpformer_amd.readers`` -> ``LinkTransformer`` -> ``evaluate`` / the training step on the HIP path,
against what the REFERENCE made of the same files from its reader to its metrics (tests/golden/pipeline_*.npz, recorded
by tests/golden/make_pipeline_golden.py).  Nothing is converted by hand between the reader and the model: that hand-off
is what is under test -- feature widths 12, 8, 5 and 6, ddi's drawn table, collab's summed weights and repeated pairs,
citation2's weight-2 entries and target-only negatives, validation edges in the test-time graph, shared and HeaRT
negatives.  Run on the GPU box: python -m pytest tests -m gpu.

Bounds: logits and ``x_node`` within ``TOL`` = 1e-4 of the reference's; metrics inside the bracket the generator recorded
for scores within ``TOL`` of the reference's (widened by ``F32_MEAN_TOL``: the bracket's ends are float32 means); the
training step within the bounds of tests/test_gpu_train.py (1e-5 on loss and outputs, 1e-4 relative on gradients,
the gradient on ddi's feature table included).
No recorded bracket is wider than 0.05, so no metric is left out of the bracket check."""
import functools

import numpy as np
import pytest
import torch

import lpformer_amd
from lpformer_amd import epoch
from lpformer_amd import evaluate as E
from oracle.ref_shims import SparseTensor
from tests.pipeline_cases import CASES, F32_MEAN_TOL, SPLITS, TOL, TRAIN_CASES, Case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _err(a, b):
    return float(np.abs(np.asarray(a, np.float64).reshape(-1) - np.asarray(b, np.float64).reshape(-1)).max())


def _model(c, data, **over):
    model = lpformer_amd.LinkTransformer(c.args(**over), data, device=DEV).to(DEV)
    score = lpformer_amd.mlp_score(model.out_dim, model.out_dim, 1, c.cfg["pred_layers"],
                                   over.get("dropout", c.cfg["dropout"])).to(DEV)
    m_sd, s_sd = c.state_dicts()
    model.load_state_dict(m_sd, strict=True)
    score.load_state_dict(s_sd, strict=True)
    return model, score


@functools.lru_cache(maxsize=None)
def _built(case):
    """(fixture, the reader's dict, model, score head) of a case, built once for the tests that share it."""
    c = Case(case)
    data = c.read()
    model, score = _model(c, data)
    return c, data, model.eval(), score.eval()


@pytest.mark.parametrize("case", CASES)
def test_encoder_on_both_graphs(case):
    c, data, model, _ = _built(case)
    with torch.no_grad():
        assert _err(model.propagate(test_set=False).cpu(), c["x_node"]) <= TOL
        assert _err(model.propagate(test_set=True).cpu(), c["x_node_test"]) <= TOL
    if c.cfg["use_val_in_test"]:
        assert _err(c["x_node"], c["x_node_test"]) > 1e-3


def _want_test_neg(c):
    """Test negatives are scored on the test-time graph (``score_splits``): where the reference's own scores come from
    another encoder (HeaRT under use_val_in_test, testing.py:105), the recorded test-graph variant is the expectation."""
    return c["logit.test_neg_fullgraph"] if "logit.test_neg_fullgraph" in c else c["logit.test_neg"]


@pytest.mark.parametrize("case", CASES)
def test_logits_through_the_sweep(case):
    c, data, model, score = _built(case)
    s = E.score_splits(model, score, data, c.batch_size, heart=c.heart, logits=True)
    worst = 0.0
    for split in SPLITS:
        want = _want_test_neg(c) if split == "test_neg" else c["logit." + split]
        assert tuple(s[split].shape) == tuple(want.shape), split
        err = _err(s[split].cpu(), want)
        worst = max(worst, err)
        assert err <= TOL, (split, err)
    print(f"{case}: worst logit error through score_edges / score_negatives {worst:.2e}")
    p = E.score_splits(model, score, data, c.batch_size, heart=c.heart)
    for split in SPLITS:
        want = c["prob.test_neg_fullgraph"] if (split == "test_neg" and "prob.test_neg_fullgraph" in c) else c["prob." + split]
        assert _err(p[split].cpu(), want) <= TOL, split


@pytest.mark.parametrize("case", CASES)
def test_logits_through_the_eager_model(case):
    """``score_func(model(edge, test_set=...))``, the reference's ``test_edge`` call, batch by batch with a ragged last
    batch; on a case with validation edges in the test graph a split scored on the other graph must miss."""
    c, data, model, score = _built(case)
    worst = 0.0

    def eager(split, test_set):
        pairs = c.split_pairs(data, split)
        out = []
        with torch.no_grad():
            for lo in range(0, pairs.shape[0], c.batch_size):
                out.append(score.logits(model(pairs[lo:lo + c.batch_size].t(), test_set=test_set)).cpu())
        assert len(out) >= 2 and out[-1].numel() < c.batch_size
        return torch.cat(out).numpy()

    for split in SPLITS:
        want = _want_test_neg(c) if split == "test_neg" else c["logit." + split]
        err = _err(eager(split, split.startswith("test")), want)
        worst = max(worst, err)
        assert err <= TOL, (split, err)
    print(f"{case}: worst logit error through model() + score head {worst:.2e}")
    if c.cfg["use_val_in_test"]:
        assert _err(eager("valid_pos", True), c["logit.valid_pos"]) > 1e-3
        assert _err(eager("test_pos", False), c["logit.test_pos"]) > 1e-3


def _in_bracket(got, c, variant, cols=(0, 1, 2)):
    names = c.metric_names(variant)
    assert set(names) == {"Hits@10", "Hits@20", "MRR"}
    for m in names:
        lo, hi = c[f"metric_lo.{variant}{m}"], c[f"metric_hi.{variant}{m}"]
        for i in cols:
            assert lo[i] - F32_MEAN_TOL <= got[m][i] <= hi[i] + F32_MEAN_TOL, (variant, m, i, got[m][i], lo[i], hi[i])


@pytest.mark.parametrize("case", CASES)
def test_evaluate_model_metrics_in_the_reference_bracket(case):
    """Hits@10, Hits@20 and MRR of ``evaluate_model`` for train, valid and test.  The reference's paths compute neither
    AUC nor AP, so those are not compared."""
    c, data, model, score = _built(case)
    if not int(c["has_metrics"]):
        # ppa_heart: more HeaRT negative rows than positives kept by the index files; the reference's metrics raise on
        # these shapes (asserted by the generator) and evaluate_model refuses them too
        with pytest.raises(ValueError):
            E.evaluate_model(model, score, data, c.batch_size, k_list=c.ks, heart=c.heart)
        return
    got = E.evaluate_model(model, score, data, c.batch_size, k_list=c.ks, heart=c.heart)
    assert got["nan_pos"] == (0, 0, 0) and got["nan_neg"] == (0, 0, 0)
    if case == "citation2":
        # DECISION (evaluate_model's docstring): the train column comes from the train positives; test_citation2 reports
        # the validation positives there (testing.py:70).  Its column is reproduced by passing them explicitly.
        _in_bracket(got, c, "own.")
        s = E.score_splits(model, score, data, c.batch_size)
        quirk = E.split_metrics(s["valid_pos"], s["valid_pos"], s["valid_neg"], s["test_pos"], s["test_neg"],
                                k_list=c.ks, layout="rows", auc=False)
        _in_bracket(quirk, c, "")
        assert quirk["MRR"][0] == quirk["MRR"][1] and abs(got["MRR"][0] - quirk["MRR"][0]) > 1e-3
    elif "logit.test_neg_fullgraph" in c:
        # DECISION (score_splits' docstring): HeaRT test negatives are encoded on the test-time graph; the reference
        # encodes them on the training graph (testing.py:105).
        _in_bracket(got, c, "fullgraph.")
        h_train = model.propagate(test_set=False)
        ref_neg = E.score_negatives(model, score, data["test_neg"], c.batch_size, h=h_train, test_set=True, logits=True)
        assert _err(ref_neg.cpu(), c["logit.test_neg"]) <= TOL          # the reference's scores, on request
        own_neg = E.score_splits(model, score, data, c.batch_size, heart=True, logits=True)["test_neg"]
        assert _err(own_neg.cpu(), c["logit.test_neg_fullgraph"]) <= TOL
        assert _err(own_neg.cpu(), c["logit.test_neg"]) > 1e-3         # and the two are told apart
        s = E.score_splits(model, score, data, c.batch_size, heart=True)
        quirk = E.split_metrics(s["train_pos_val"], s["valid_pos"], s["valid_neg"], s["test_pos"], torch.sigmoid(ref_neg),
                                k_list=c.ks, layout="rows", auc=False)
        _in_bracket(quirk, c, "")
    else:
        _in_bracket(got, c, "")


def _reference_masked_adjt(data, perm):
    """The reference's ``masked_adjt`` (train_model.py:47-52): the rows of ``train_pos`` outside the batch, symmetrised,
    WITHOUT weights."""
    n = int(data["num_nodes"])
    keep = torch.ones(data["train_pos"].shape[0], dtype=torch.bool)
    keep[perm] = False
    return SparseTensor.from_edge_index(data["train_pos"][keep].t(), sparse_sizes=(n, n)).to_symmetric()


def _unit_weights(data):
    val = data["adj_t"].val
    return val is None or bool((np.asarray(val) == 1).all())


def _train_step(case, x_parameter=False):
    c = Case(case, train=True)
    data = Case(case).read()
    if x_parameter:       # the reference's reader hands a feature-less table over as an nn.Parameter (read_datasets.py:76)
        data["x"] = torch.nn.Parameter(data["x"])
    model, score = _model(c, data, att_drop=0.0, dropout=0.0, gnn_drop=0.0, feat_drop=0.0)
    model.train()
    score.train()
    perm = torch.from_numpy(c["train_perm"])
    te = epoch.TrainEdges(data["train_pos"], int(data["num_nodes"]), device=DEV)
    te.check_against(model, False)
    removed = te.mask(perm)
    adj_prop = None
    if c.cfg["mask_input"] and _unit_weights(data):
        adj_prop = removed          # what train_epoch passes: the same difference, to the propagation matrix (ddi)
    elif c.cfg["mask_input"]:
        # collab's adj_t is weighted and the reference's masked propagation matrix is not: train_epoch refuses
        # (test_train_epoch_on_the_reader_dict) and names the tensor to pass instead, built here as the reference builds it
        adj_prop = _reference_masked_adjt(data, perm)
    edges = te.train_pos[perm.to(DEV)].t()
    h = model(edges, adj_prop=adj_prop, adj_mask=removed)
    pos_out = score(h)
    neg_out = score(model(torch.from_numpy(c["train_neg_edges"]).to(DEV)))
    loss = -torch.log(pos_out + 1e-6).mean() - torch.log(1 - neg_out + 1e-6).mean()
    loss.backward()
    return c, data, model, score, loss, pos_out, neg_out


def _rel(got, want):
    return _err(got, want) / max(float(np.abs(want).max()), 1e-6)


@pytest.mark.parametrize("case", TRAIN_CASES)
def test_training_step_matches_reference_gradients(case):
    c, data, model, score, loss, pos_out, neg_out = _train_step(case)
    print(f"{case}: loss error {abs(loss.item() - float(c['train_loss'])):.2e}, pos_out {_err(pos_out.detach().cpu(), c['train_pos_out']):.2e}, "
          f"neg_out {_err(neg_out.detach().cpu(), c['train_neg_out']):.2e}")
    assert abs(loss.item() - float(c["train_loss"])) <= 1e-5
    assert _err(pos_out.detach().cpu(), c["train_pos_out"]) <= 1e-5
    assert _err(neg_out.detach().cpu(), c["train_neg_out"]) <= 1e-5
    worst, worst_key, checked = 0.0, None, 0
    failed = []
    for tag, mod in (("model", model), ("score", score)):
        for name, p in mod.named_parameters():
            key = f"grad.{tag}.{name}"
            if key not in c:
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, name   # unused parameter
                continue
            rel = _rel(p.grad.detach().cpu(), c[key])
            if rel > worst:
                worst, worst_key = rel, key
            checked += 1
            if rel > 1e-4:
                failed.append((key, rel))
    print(f"{case}: {checked} gradients, worst relative error {worst:.2e} ({worst_key})")
    assert not failed, failed
    assert checked >= 50
    assert not data["x"].requires_grad and data["x"].grad is None     # the readers' tables are plain tensors


def test_ddi_feature_table_gradient():
    """The reference's reader makes ogbl-ddi's drawn table an ``nn.Parameter`` (read_datasets.py:76); backward leaves a
    gradient on it that no optimizer steps (train_model.py:99).  ``readers`` returns a plain tensor; a table that does
    require a gradient gets the reference's, and the parameter gradients beside it are unchanged."""
    c, data, model, score, loss, _, _ = _train_step("ddi", x_parameter=True)
    assert abs(loss.item() - float(c["train_loss"])) <= 1e-5
    assert data["x"].grad is not None and data["x"].grad.shape == data["x"].shape
    rel = _rel(data["x"].grad.cpu(), c["grad.data.x"])
    print(f"ddi: relative error of the gradient on x {rel:.2e}")
    assert rel <= 1e-4
    for key in ("grad.model.node_encoder.gnn_encoder.convs.0.lin.weight", "grad.score.lins.0.weight"):
        tag, name = key[5:].split(".", 1)
        got = dict((model if tag == "model" else score).named_parameters())[name].grad
        assert _rel(got.detach().cpu(), c[key]) <= 1e-4, key


@pytest.mark.parametrize("case", TRAIN_CASES)
def test_train_epoch_on_the_reader_dict(case):
    """``epoch.train_epoch`` itself on the reader's dict, one batch: the stored rows and negatives, the learning rate 0.
    Its loss is the reference's; with ``mask_input`` on a weighted ``adj_t`` (collab) it refuses, as documented."""
    c = Case(case, train=True)
    data = Case(case).read()
    model, score = _model(c, data, att_drop=0.0, dropout=0.0, gnn_drop=0.0, feat_drop=0.0)
    opt = torch.optim.SGD(list(model.parameters()) + list(score.parameters()), lr=0.0)
    neg = torch.from_numpy(c["train_neg_edges"]).to(DEV)
    kw = dict(batches=[torch.from_numpy(c["train_perm"])], negatives=lambda step, edges: neg, clip=None,
              mask_input=bool(c.cfg["mask_input"]))
    if c.cfg["mask_input"] and not _unit_weights(data):
        with pytest.raises(ValueError, match="non-unit weights"):
            epoch.train_epoch(model, score, data, opt, **kw)
        kw["mask_input"] = False      # (the typing mask alone: the loop runs; its loss is not the recorded one)
        assert np.isfinite(epoch.train_epoch(model, score, data, opt, **kw))
        return
    loss = epoch.train_epoch(model, score, data, opt, **kw)
    assert abs(loss - float(c["train_loss"])) <= 1e-5
