#!/usr/bin/env python3
"""Record what the REFERENCE computes from dataset files to metrics, as fixtures for tests/test_pipeline_host.py and
tests/test_gpu_pipeline.py:

    python tests/golden/make_pipeline_golden.py --reference /path/to/reference

The reference's readers (``src/util/read_datasets.py``), model (``src/models``), evaluation loops (``src/train/testing.py``)
and metrics (``src/train/evaluation.py``) are imported unmodified (third-party packages replaced by oracle/ref_shims.py,
the OGB dataset class by the stand-in of tests/golden/reference_env.py) and run on the committed tiny datasets under
tests/golden/planetoid_tiny/ and tests/golden/ogb_tiny/, which are only read.  Only DATA is written:
``tests/golden/pipeline_<case>.npz`` and, for the cases with a training step, ``pipeline_<case>_train.npz``.  The reader
is seeded as tests/test_readers.py seeds it and its output is compared with reader_planetoid.npz / reader_ogb.npz wherever
those hold the same call, so the two fixture families cannot drift apart.  Parameters are the seed-derived values of
oracle/fixture_weights.py; a fixture stores only their names and shapes.

Recorded in eval mode, per case: ``x_node`` of both graphs; logit and probability of ``train_pos_val``, ``valid_pos``,
``test_pos``, ``valid_neg``, ``test_neg`` through ``test_edge`` / ``test_heart_negatives`` / ``test_edge_citation2``
(probabilities with the reference's score head, logits with the same head without its sigmoid); the metrics of
``get_metric_score`` / ``get_metric_score_citation2`` (Hits@K through the ``StandInHits`` of make_metrics_golden.py; for
per-row negatives also ``evaluate_mrr``'s Hits@10 and the mean of ``sample_level_hits``' Hits@20, the only Hits the
reference defines for that layout); and the same metrics twice more, with every positive logit lowered and every negative
logit raised by TOL and the reverse: rank metrics are monotone in pos - neg, so scores within TOL of the recorded logits
give metrics inside [lo, hi].

RESTATED here, everything else is the reference's own call:
* ``test_edge_citation2(mrr_mode=True)`` hard-codes 1000 negatives per positive (testing.py:22); the tiny set has 9.  The
  (source, target_neg) pairs are built with K in place of 1000 and scored with the loop body's own three calls
  (testing.py:29-32).
* the test negatives of ``collab_valtest_heart`` ON THE TEST GRAPH (``neg_test_fullgraph``): ``test_heart_negatives``
  always encodes with ``model.propagate()``, the training graph (testing.py:105); the variant uses
  ``model.propagate(test_set=True)`` with the same loop body.

Two things the committed tiny datasets do not allow, asserted here so that they stay visible:
* common neighbours: with thresh_cn = 0 every common neighbour of a pair is selected, and the OGB-layout graphs have
  fewer than 20 of them over a split's positives.  The generator asserts >= 20 selected entries for 1-hop and >1-hop,
  and for CN at least min(20, every common neighbour the split has).
* ``ppa_heart``: the HeaRT sample files hold a row for every validation / test positive, the index files keep 30 of them, so
  ``get_metric_score_citation2`` raises on [30] against [79, 12]; scores are recorded, metrics are not (``has_metrics`` 0).

Recorded in train mode with all dropout probabilities 0 (``collab_valtest`` and ``ddi`` with mask_input -- a weighted and
a unit-weight propagation matrix --, ``citation2`` without): one
step of src/train/train_model.py:35-71 on a stored ``perm`` of 64 rows of the reader's ``train_pos`` -- the reference's
own row-removal masks, stored negatives, ``loss``, ``pos_out``, ``neg_out``, every parameter gradient and, where backward
leaves one (ddi), the gradient on ``data['x']``.
"""
import sys

sys.dont_write_bytecode = True   # nothing may be written into the reference tree

import argparse   # noqa: E402
import json       # noqa: E402
import os         # noqa: E402
import types      # noqa: E402

import numpy as np   # noqa: E402
import torch         # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_metrics_golden import StandInHits                                     # noqa: E402
from oracle import ref_shims                                                    # noqa: E402
from oracle.fixture_weights import make_param                                   # noqa: E402
from reference_env import OGB_DIR, PLANETOID_DIR, patch_reference_readers, save_npz_stable   # noqa: E402

TOL = 1e-4             # the project's logit tolerance (tests/test_gpu_parity.py)
K_LIST = (10, 20)
MIN_SELECTED = 20
TRAIN_ROWS = 64

# thresholds = (thresh_cn, thresh_1hop, thresh_non1hop); eps is the one of reader_planetoid.npz / reader_ogb.npz
CASES = {
    "tinycora": dict(dataset="tinycora", val_in_test=False, heart=False, dim=64, gnn_layers=2, thresholds=(0, 1e-2, 1e-2),
                     eps=1e-4, batch_size=48, seed=31),
    "tinycora_heart": dict(dataset="tinycora", val_in_test=False, heart=True, dim=32, gnn_layers=2, residual=True,
                           thresholds=(0, 5e-3, 1e-2), eps=1e-4, batch_size=48, seed=32),
    "collab_valtest": dict(dataset="ogbl-collab", val_in_test=True, heart=False, dim=128, gnn_layers=3,
                           thresholds=(0, 1e-3, 5e-3), eps=1e-3, batch_size=40, seed=33, train=dict(mask_input=True)),
    "collab_valtest_heart": dict(dataset="ogbl-collab", val_in_test=True, heart=True, dim=64, gnn_layers=2,
                                 thresholds=(0, 2e-3, 5e-3), eps=1e-3, batch_size=40, seed=34),
    "ppa_heart": dict(dataset="ogbl-ppa", val_in_test=False, heart=True, dim=256, gnn_layers=2, layer_norm=False,
                      thresholds=(0, 1e-3, 1e-3), eps=1e-3, batch_size=25, seed=35),
    "ddi": dict(dataset="ogbl-ddi", val_in_test=False, heart=False, dim=32, gnn_layers=2, thresholds=(0, 1e-3, 2e-3),
                eps=1e-3, batch_size=32, seed=36, train=dict(mask_input=True)),
    "citation2": dict(dataset="ogbl-citation2", val_in_test=False, heart=False, dim=64, gnn_layers=2, residual=True,
                      thresholds=(0, 1e-3, 2e-3), eps=1e-3, batch_size=32, seed=37, train=dict(mask_input=False)),
}


class LogitHead(torch.nn.Module):
    """The reference's ``mlp_score`` without its final sigmoid (other_models.py:173-179), so that the reference's loops
    return logits: same modules, same order."""
    def __init__(self, score):
        super().__init__()
        self.score = score

    def forward(self, x):
        for lin in self.score.lins[:-1]:
            x = torch.relu(lin(x))
        return self.score.lins[-1](x).squeeze(-1)


def read(rd, c):
    """The reference reader's dict for case ``c``, seeded as tests/test_readers.py seeds it."""
    if c["dataset"] == "tinycora":
        rd.DATA_DIR, rd.HEART_DIR = PLANETOID_DIR, os.path.join(PLANETOID_DIR, "heart")
        torch.manual_seed(11)
        return rd.read_data_planetoid(types.SimpleNamespace(data_name="tinycora", eps=c["eps"], heart=c["heart"]), "cpu")
    rd.HEART_DIR = os.path.join(OGB_DIR, "heart")
    torch.manual_seed(5)
    return rd.read_data_ogb(types.SimpleNamespace(data_name=c["dataset"], eps=c["eps"], heart=c["heart"],
                                                  use_val_in_test=c["val_in_test"], dim=c["dim"]), "cpu")


def check_against_reader_fixture(c, d):
    """The reader's output equals what make_reader_golden.py recorded for the same call.  Returns the number of arrays
    compared."""
    n_cmp = 0
    if c["dataset"] == "tinycora":
        z = np.load(os.path.join(HERE, "reader_planetoid.npz"))
        tag = "heart_" if c["heart"] else ""
        want = {k: z[k] for k in ("train_pos", "train_pos_val", "valid_pos", "test_pos", "x")}
        want["valid_neg"], want["test_neg"] = z[tag + "valid_neg"], z[tag + "test_neg"]
        for k, v in want.items():
            np.testing.assert_array_equal(d[k].numpy(), v, err_msg=k)
            n_cmp += 1
        assert c["eps"] == 1e-4
        p = d["ppr"].coalesce()
        np.testing.assert_array_equal(p.indices().numpy(), z["ppr_index"])
        np.testing.assert_array_equal(p.values().numpy().view(np.uint32), z["ppr_val"].view(np.uint32))
        return n_cmp + 2
    z = np.load(os.path.join(HERE, "reader_ogb.npz"))
    tag = f"{c['dataset']}|{int(c['val_in_test'])}|{int(c['heart'])}|"
    if tag + "num_nodes" not in z.files:      # (collab with HeaRT negatives is not among the reader cases)
        tag = f"{c['dataset']}|{int(c['val_in_test'])}|0|"
        keys = ("train_pos", "train_pos_val", "valid_pos", "test_pos")
    else:
        keys = ("train_pos", "train_pos_val", "valid_pos", "valid_neg", "test_pos", "test_neg")
    assert c["eps"] == 1e-3 and int(z[tag + "num_nodes"]) == d["num_nodes"]
    for k in keys:
        np.testing.assert_array_equal(d[k].numpy(), z[tag + k], err_msg=k)
        n_cmp += 1
    if "ddi" not in c["dataset"]:             # (ddi's table is drawn for the case's own dim)
        np.testing.assert_array_equal(d["x"].detach().numpy(), z[tag + "x"])
        n_cmp += 1
    for key in ("adj_t", "full_adj_t"):
        r, col, v = d[key].coo()
        got = np.stack([r.numpy().astype(np.float64), col.numpy().astype(np.float64), v.numpy().astype(np.float64)])
        np.testing.assert_array_equal(got, z[tag + key], err_msg=key)
        n_cmp += 1
    for key in ("adj_mask", "full_adj_mask", "ppr", "ppr_test"):
        t = d[key].coalesce()
        np.testing.assert_array_equal(t.indices().numpy(), z[tag + key + "_index"], err_msg=key)
        np.testing.assert_array_equal(t.values().numpy(), z[tag + key + "_val"], err_msg=key)
        n_cmp += 1
    return n_cmp


def train_args_of(c, drop):
    th = c["thresholds"]
    return {"thresh_cn": th[0], "thresh_1hop": th[1], "thresh_non1hop": th[2], "dim": c["dim"], "trans_layers": 1,
            "num_heads": 1, "att_drop": drop, "dropout": drop, "gnn_drop": drop, "feat_drop": drop, "gcn_cache": False,
            "gnn_layers": c["gnn_layers"], "residual": c.get("residual", False), "layer_norm": c.get("layer_norm", True),
            "relu": True}


def build_model(ref, c, d, drop):
    model = ref.LinkTransformer(train_args_of(c, drop), d, device="cpu")
    score = ref.mlp_score(model.out_dim, model.out_dim, 1, 2, drop)
    shapes = {}
    with torch.no_grad():
        for tag, mod in (("model", model), ("score", score)):
            for pname, p in mod.state_dict().items():
                shapes[f"{tag}.{pname}"] = list(p.shape)
                p.copy_(torch.from_numpy(make_param(f"{tag}.{pname}", p.shape, c["seed"])))
    return model, score, shapes


def selection_counts(model, d):
    """Selected entries per node type over the validation and the test positives, and the common neighbours those splits
    have at all (from the typing adjacency, independent of any threshold)."""
    out = {}
    with torch.no_grad():
        for split, test_set in (("valid_pos", False), ("test_pos", True)):
            batch = d[split].t()
            infos = model.compute_node_mask(batch, test_set, None)
            adj = model.get_adj(test_set, mask=True)
            both = (torch.index_select(adj, 0, batch[0]) * torch.index_select(adj, 0, batch[1])).coalesce()
            all_cn = int((both.values() != 0).sum())
            out[split] = (infos[0][0].shape[1], infos[1][0].shape[1], infos[2][0].shape[1], all_cn)
    return out


def loop_body_scores(model, head, h, edges, batch_size, test_set):
    """The loop body of ``test_heart_negatives`` / ``test_edge_citation2`` (testing.py:110-117, :25-32) over ``edges``
    [P, 2] with a given encoder output."""
    from torch.utils.data import DataLoader
    preds = []
    with torch.no_grad():
        for perm in DataLoader(range(edges.size(0)), batch_size):
            e = edges[perm].t()
            elementwise_feats = model.elementwise_lin(h[e[0]] * h[e[1]])
            pairwise_feats, _ = model.calc_pairwise(e, h, test_set=test_set)
            preds += [head(torch.cat((elementwise_feats, pairwise_feats), dim=-1)).squeeze().cpu()]
    return torch.cat(preds, dim=0)


def eval_scores(ref, c, d, model, score):
    """{split: tensor} per head ("prob": the reference's score head, "logit": the same without its sigmoid)."""
    T, bs = ref.testing, c["batch_size"]
    out = {}
    for kind, head in (("prob", score), ("logit", LogitHead(score).eval())):
        s = {}
        with torch.no_grad():
            if "citation2" in c["dataset"] and not c["heart"]:     # test_citation2 (testing.py:50-74)
                h = model.propagate()
                s["valid_pos"] = T.test_edge_citation2(model, head, d["valid_pos"], h, bs)
                s["test_pos"] = T.test_edge_citation2(model, head, d["test_pos"], h, bs, test=True)
                s["train_pos_val"] = T.test_edge_citation2(model, head, d["train_pos_val"], h, bs)
                for split, pos, test in (("valid_neg", "valid_pos", False), ("test_neg", "test_pos", True)):
                    k = d[split].size(1)
                    source = d[pos].t()[0].view(-1, 1).repeat(1, k).view(-1)          # :21-23 with K for 1000
                    pairs = torch.stack((source, d[split].view(-1)), dim=-1)
                    s[split] = loop_body_scores(model, head, h, pairs, bs, test).view(-1, k)
            else:                                                   # test (testing.py:124-161)
                s["train_pos_val"] = T.test_edge(model, head, d["train_pos_val"], bs)
                s["valid_pos"] = T.test_edge(model, head, d["valid_pos"], bs)
                s["test_pos"] = T.test_edge(model, head, d["test_pos"], bs, test_set=True)
                if c["heart"]:
                    s["valid_neg"] = T.test_heart_negatives(d["valid_neg"], model, head, batch_size=bs)
                    s["test_neg"] = T.test_heart_negatives(d["test_neg"], model, head, batch_size=bs, test_set=True)
                    if c["val_in_test"]:
                        k = d["test_neg"].size(1)
                        flat = torch.permute(d["test_neg"], (2, 0, 1)).reshape(2, -1).t()      # :102
                        s["test_neg_fullgraph"] = loop_body_scores(model, head, model.propagate(test_set=True), flat, bs,
                                                                   True).view(-1, k)
                else:
                    s["valid_neg"] = T.test_edge(model, head, d["valid_neg"], bs)
                    s["test_neg"] = T.test_edge(model, head, d["test_neg"], bs, test_set=True)
        out[kind] = {k: v.view(-1) if v.dim() == 1 or not k.endswith(("neg", "fullgraph")) else v for k, v in s.items()}
    for k, v in out["logit"].items():
        assert torch.allclose(torch.sigmoid(v), out["prob"][k], atol=1e-6), k
    return out


def metrics_of(ref, rows, pos_train, pos_valid, neg_valid, pos_test, neg_test):
    """{metric: (train, valid, test)} by the reference's functions.  ``rows``: per-positive negatives [P, K]."""
    E = ref.evaluation
    if not rows:
        res = E.get_metric_score(StandInHits(), object(), pos_train, pos_valid, neg_valid.flatten(), pos_test,
                                 neg_test.flatten(), k_list=list(K_LIST))
        return {k: tuple(float(x) for x in v) for k, v in res.items()}
    res = {"MRR": E.get_metric_score_citation2(object(), pos_train, pos_valid, neg_valid, pos_test, neg_test)["MRR"]}
    parts = ((pos_train, neg_valid), (pos_valid, neg_valid), (pos_test, neg_test))
    res["Hits@10"] = tuple(E.evaluate_mrr(p, n)["Hits@10"] for p, n in parts)
    res["Hits@20"] = tuple(E.sample_level_hits(p, n)["Hits@20"].mean().item() for p, n in parts)
    return {k: tuple(float(x) for x in v) for k, v in res.items()}


def bracket(ref, rows, logit, neg_test_key="test_neg", train_key="train_pos_val"):
    """(recorded, lo, hi) metrics of the scores in ``logit``: at the logits themselves, with positives lowered and
    negatives raised by TOL, and the reverse; probabilities through the score head's sigmoid."""
    def at(shift):
        sg = lambda k, s: torch.sigmoid(logit[k] + s)      # noqa: E731
        return metrics_of(ref, rows, sg(train_key, shift), sg("valid_pos", shift), sg("valid_neg", -shift),
                          sg("test_pos", shift), sg(neg_test_key, -shift))
    return at(0.0), at(-TOL), at(TOL)


def pick_perm(train_pos, n, rng, want_twins):
    """64 distinct rows of ``train_pos``.  ``want_twins``: among them (a) one row of an undirected pair whose other rows
    stay outside and (b) every row of another pair that the list holds more than once."""
    tp = train_pos.numpy()
    key = np.minimum(tp[:, 0], tp[:, 1]) * n + np.maximum(tp[:, 0], tp[:, 1])
    uniq, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    if not want_twins:
        return np.sort(rng.permutation(tp.shape[0])[:TRAIN_ROWS])
    multi = np.nonzero(cnt >= 2)[0]
    ga, gb = multi[0], multi[1]
    rows_a, rows_b = np.nonzero(inv == ga)[0], np.nonzero(inv == gb)[0]
    single = np.nonzero(cnt[inv] == 1)[0]
    fill = rng.permutation(single)[:TRAIN_ROWS - 1 - rows_b.size]
    perm = np.concatenate([rows_a[:1], rows_b, fill])
    assert perm.size == TRAIN_ROWS == np.unique(perm).size
    inside = np.zeros(tp.shape[0], bool)
    inside[perm] = True
    assert inside[rows_a].sum() == 1 and rows_a.size >= 2            # (a) the twin stays outside
    assert inside[rows_b].all() and rows_b.size >= 2                 # (b) both rows inside
    return rng.permutation(perm)


def train_step(ref, c, d, out):
    """One step of train_model.py:35-71, all dropouts 0."""
    from torch_sparse import SparseTensor    # shim
    model, score, _ = build_model(ref, c, d, 0.0)
    model.train()
    score.train()
    n = d["num_nodes"]
    rng = np.random.default_rng(c["seed"])
    train_pos = d["train_pos"]
    perm = torch.from_numpy(pick_perm(train_pos, n, rng, "collab" in c["dataset"]))
    edges = train_pos[perm].t()
    adjmask = torch.ones(train_pos.size(0), dtype=torch.bool)
    adjmask[perm] = 0
    edge2keep = train_pos[adjmask, :]
    masked_adj = SparseTensor.from_edge_index(edge2keep.t(), sparse_sizes=(n, n)).to_device("cpu")
    masked_adj = masked_adj.to_symmetric()
    masked_adjt = masked_adj if c["train"]["mask_input"] else None       # (:47-57: the same rows, unweighted)
    masked_adj = masked_adj.to_torch_sparse_coo_tensor().coalesce().bool().int()
    h = model(edges, adj_prop=masked_adjt, adj_mask=masked_adj)
    pos_out = score(h)
    pos_loss = -torch.log(pos_out + 1e-6).mean()
    neg_edges = torch.from_numpy(rng.integers(0, n, size=(2, edges.size(1))))
    neg_out = score(model(neg_edges))
    neg_loss = -torch.log(1 - neg_out + 1e-6).mean()
    loss = pos_loss + neg_loss
    loss.backward()
    out.update(train_perm=perm.numpy(), train_neg_edges=neg_edges.numpy(), train_loss=np.float32(loss.item()),
               train_pos_out=pos_out.detach().numpy(), train_neg_out=neg_out.detach().numpy(),
               train_masked_index=masked_adj.indices().numpy().astype(np.int32))
    n_grad = 0
    for tag, mod in (("model", model), ("score", score)):
        for pname, p in mod.named_parameters():
            if p.grad is not None:
                out[f"grad.{tag}.{pname}"] = p.grad.numpy().astype(np.float32)
                n_grad += 1
    x = d["x"]
    if getattr(x, "grad", None) is not None:
        out["grad.data.x"] = x.grad.numpy().astype(np.float32)
        x.grad = None
    return f"train step: loss {loss.item():.6f}, {n_grad} gradients" + (", grad on x" if "grad.data.x" in out else "")


def build(ref, rd, name):
    c = CASES[name]
    d = read(rd, c)
    n_cmp = check_against_reader_fixture(c, d)
    model, score, shapes = build_model(ref, c, d, 0.1)
    model.eval()
    score.eval()
    counts = selection_counts(model, d)
    for split, (cn, one, far, all_cn) in counts.items():
        assert one >= MIN_SELECTED and far >= MIN_SELECTED, (name, split, counts)
        assert cn >= min(MIN_SELECTED, all_cn), (name, split, counts)
    bs = c["batch_size"]
    for k in ("train_pos_val", "valid_pos", "test_pos", "valid_neg", "test_neg"):
        rows = d[k].shape[0] * (d[k].shape[1] if d[k].dim() == 3 or ("citation2" in c["dataset"] and k.endswith("neg")) else 1)
        assert rows > bs and rows % bs != 0, (name, k, rows, bs)      # at least two batches, the last one ragged
    out = {}
    with torch.no_grad():
        out["x_node"] = model.propagate(test_set=False).numpy()
        out["x_node_test"] = model.propagate(test_set=True).numpy()
    if "ddi" in c["dataset"]:
        out["x"] = d["x"].detach().numpy()
    s = eval_scores(ref, c, d, model, score)
    for kind in ("prob", "logit"):
        for k, v in s[kind].items():
            out[f"{kind}.{k}"] = v.numpy()
    rows = c["heart"] or "citation2" in c["dataset"]
    lg = s["logit"]
    widths = {}
    has_metrics = not (rows and lg["valid_neg"].shape[0] != lg["valid_pos"].shape[0])
    if has_metrics:
        variants = {"": dict()}
        if "citation2" in c["dataset"]:
            # test_citation2 reports the VALIDATION positives in the train column (testing.py:70); "own" is the column
            # from the train positives it scored four lines earlier
            lg = dict(lg, train_as_valid=lg["valid_pos"])
            variants = {"": dict(train_key="train_as_valid"), "own.": dict(train_key="train_pos_val")}
        if "test_neg_fullgraph" in lg:
            variants["fullgraph."] = dict(neg_test_key="test_neg_fullgraph")
        for vtag, kw in variants.items():
            rec, lo, hi = bracket(ref, rows, lg, **kw)
            for m in rec:
                out[f"metric.{vtag}{m}"] = np.asarray(rec[m], np.float64)
                out[f"metric_lo.{vtag}{m}"] = np.asarray(lo[m], np.float64)
                out[f"metric_hi.{vtag}{m}"] = np.asarray(hi[m], np.float64)
                widths[vtag + m] = float(np.max(np.asarray(hi[m]) - np.asarray(lo[m])))
                assert all(a <= b <= e for a, b, e in zip(lo[m], rec[m], hi[m])), (name, vtag, m)
        if not ("citation2" in c["dataset"]):
            # the reference's test() as a whole gives the recorded probabilities' metrics
            whole = ref.testing.test(model, score, d, StandInHits(), object(), bs, k_list=list(K_LIST), heart=c["heart"])
            pr = s["prob"]
            direct = metrics_of(ref, rows, pr["train_pos_val"], pr["valid_pos"], pr["valid_neg"], pr["test_pos"], pr["test_neg"])
            for m, v in whole.items():
                assert tuple(float(x) for x in v) == direct[m], (name, m)
    else:
        try:
            metrics_of(ref, rows, s["prob"]["train_pos_val"], s["prob"]["valid_pos"], s["prob"]["valid_neg"],
                       s["prob"]["test_pos"], s["prob"]["test_neg"])
            raise SystemExit(f"{name}: expected the reference's metrics to refuse these shapes")
        except RuntimeError:
            pass
    out["has_metrics"] = np.int64(has_metrics)
    train_out = {}
    train_note = train_step(ref, c, d, train_out) if c.get("train") else ""
    cfg = train_args_of(c, 0.1)
    cfg.update(n=int(d["num_nodes"]), f_in=int(d["x"].shape[1]), eps=c["eps"], dataset=c["dataset"],
               use_val_in_test=c["val_in_test"], heart=c["heart"], batch_size=bs, k_list=list(K_LIST), tol=TOL,
               layout="rows" if rows else "shared", pred_layers=2, seed=c["seed"], param_shapes=shapes,
               mask_input=bool(c.get("train", {}).get("mask_input", False)), selected=counts)
    out["config_json"] = np.array(json.dumps(cfg))
    path = os.path.join(HERE, f"pipeline_{name}.npz")
    save_npz_stable(path, out)
    size = os.path.getsize(path)
    if train_out:       # (the gradients of a D = 128 model alone are most of a MiB: a file of their own)
        train_out["config_json"] = out["config_json"]
        save_npz_stable(os.path.join(HERE, f"pipeline_{name}_train.npz"), train_out)
        size = (size, os.path.getsize(os.path.join(HERE, f"pipeline_{name}_train.npz")))
    print(f"[pipeline] {name}: reader arrays checked {n_cmp}; selected (cn, 1-hop, >1-hop, all cn) {counts}")
    print(f"           bracket widths (hi - lo) {({k: round(v, 4) for k, v in widths.items()}) if widths else 'no metrics'}")
    print(f"           {train_note + '; ' if train_note else ''}{size} bytes")
    wide = [k for k, v in widths.items() if v > 0.05]
    by_variant = {}
    for k in wide:
        by_variant.setdefault(k.rsplit(".", 1)[0] if "." in k else "", []).append(k)
    assert all(len(v) <= 1 for v in by_variant.values()), f"{name}: more than one metric wider than 0.05: {wide}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout")
    ap.add_argument("cases", nargs="*", help="only these cases (default: all)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(args.reference), "src"))
    ref_shims.install()
    sys.modules["ogb.linkproppred"].Evaluator = object        # (train_model.py is not imported; testing.py needs none)
    import util.calc_ppr_scores as cps
    import util.read_datasets as rd
    from models.link_transformer import LinkTransformer
    from models.other_models import mlp_score
    from train import evaluation, testing
    patch_reference_readers(rd, cps)
    torch.set_num_threads(1)       # (scatter-adds in a fixed order: the recorded gradients are the same on every run)
    ref = types.SimpleNamespace(LinkTransformer=LinkTransformer, mlp_score=mlp_score, evaluation=evaluation, testing=testing)
    for name in (args.cases or CASES):
        build(ref, rd, name)


if __name__ == "__main__":
    main()
