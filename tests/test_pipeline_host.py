"""The dataset-to-metrics fixtures (tests/golden/pipeline_*.npz, recorded from the reference by
tests/golden/make_pipeline_golden.py) checked without a GPU:

* ``evaluate.split_metrics`` on the recorded reference SCORES gives the recorded reference METRICS -- the wiring of
  splits, layouts and K, independent of any kernel.  Shared-negative Hits@K: equal.  MRR and per-row Hits@K are float32
  means on the reference's side: ``F32_MEAN_TOL`` (derived in tests/test_metrics_host.py).
* the CPU oracle on the dict ``lpformer_amd.readers`` builds reproduces the recorded ``x_node`` and logits within
  ``TOL``: the fixtures and the reader hand-off are checked here before a GPU is involved.  The oracle supports every case.
* the recorded bracket [lo, hi] holds the recorded metric.
* ``epoch.TrainEdges.mask`` of the stored batch, taken from the resident typing adjacency, is the reference's own
  row-removal ``masked_adj`` entry for entry -- on collab with a repeated pair half inside and another wholly inside."""
import numpy as np
import pytest
import torch

from lpformer_amd import evaluate as E
from oracle import lpformer_oracle as O
from tests.pipeline_cases import CASES, F32_MEAN_TOL, SPLITS, TOL, TRAIN_CASES, Case


def _t(c, key):
    return torch.from_numpy(c[key])


def _same(got, c, variant, what):
    for m in c.metric_names(variant):
        want = c[f"metric.{variant}{m}"]
        for i in range(3):
            if c.layout == "shared" and m.startswith("Hits@"):
                assert got[m][i] == float(want[i]), (what, m, i)
            else:
                assert abs(got[m][i] - float(want[i])) <= F32_MEAN_TOL, (what, m, i, got[m][i], float(want[i]))


@pytest.mark.parametrize("case", CASES)
def test_split_metrics_on_reference_scores_gives_reference_metrics(case):
    c = Case(case)
    s = {k: _t(c, "prob." + k) for k in SPLITS}
    if not int(c["has_metrics"]):
        # ppa_heart: the tiny dataset's HeaRT sample files hold more rows than the index files keep positives; the
        # reference's get_metric_score_citation2 raises on these shapes (asserted by the generator), and so do we
        assert s["valid_neg"].shape[0] != s["valid_pos"].shape[0]
        with pytest.raises(ValueError):
            E.split_metrics(s["train_pos_val"], s["valid_pos"], s["valid_neg"], s["test_pos"], s["test_neg"],
                            k_list=c.ks, layout=c.layout)
        return
    assert set(c.metric_names()) == {"Hits@10", "Hits@20", "MRR"}
    train = s["valid_pos"] if case == "citation2" else s["train_pos_val"]      # testing.py:70
    got = E.split_metrics(train, s["valid_pos"], s["valid_neg"], s["test_pos"], s["test_neg"], k_list=c.ks,
                          layout=c.layout, auc=False)
    _same(got, c, "", "as the reference reports them")
    if case == "citation2":          # the train column from the train positives the reference scored and dropped
        own = E.split_metrics(s["train_pos_val"], s["valid_pos"], s["valid_neg"], s["test_pos"], s["test_neg"],
                              k_list=c.ks, layout=c.layout, auc=False)
        _same(own, c, "own.", "train column of its own")
        assert abs(own["MRR"][0] - got["MRR"][0]) > 1e-3 and own["MRR"][1:] == got["MRR"][1:]
    if case == "collab_valtest_heart":
        full = E.split_metrics(s["train_pos_val"], s["valid_pos"], s["valid_neg"], s["test_pos"],
                               _t(c, "prob.test_neg_fullgraph"), k_list=c.ks, layout=c.layout, auc=False)
        _same(full, c, "fullgraph.", "test negatives on the test graph")


@pytest.mark.parametrize("case", CASES)
def test_recorded_bracket_holds_the_recorded_metric(case):
    c = Case(case)
    variants = [""] + (["own."] if case == "citation2" else []) + (["fullgraph."] if case == "collab_valtest_heart" else [])
    for v in variants if int(c["has_metrics"]) else []:
        names = c.metric_names(v)
        assert len(names) == 3
        wide = 0
        for m in names:
            lo, mid, hi = c[f"metric_lo.{v}{m}"], c[f"metric.{v}{m}"], c[f"metric_hi.{v}{m}"]
            assert (lo <= mid).all() and (mid <= hi).all(), (v, m)
            wide += int((hi - lo).max() > 0.05)
        assert wide <= 1


def _graphs(d, test_set):
    pre = "full_" if test_set else ""
    adj, mask, ppr = d[pre + "adj_t"], d[pre + "adj_mask"], d["ppr_test" if test_set else "ppr"]
    n = adj.n
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(adj.rowptr))
    ei = np.stack([rows, adj.col.astype(np.int64)])
    w = None if adj.val is None else np.asarray(adj.val, np.float32)
    return (O.gcn_norm(ei, w, n), (np.asarray(mask.rowptr), np.asarray(mask.col).astype(np.int64)),
            (np.asarray(ppr.rowptr), np.asarray(ppr.col).astype(np.int64), np.asarray(ppr.val)))


@pytest.mark.parametrize("case", CASES)
def test_oracle_on_the_reader_dict_reproduces_the_reference(case):
    c = Case(case)
    d = c.read()
    x = d["x"].detach().numpy()
    if "x" in c:           # ddi: the table drawn under the reader's seed
        np.testing.assert_array_equal(x, c["x"])
    cfg = dict(c.cfg, pred_layers=2)
    g = {ts: _graphs(d, ts) for ts in (False, True)}
    h = {ts: O.propagate(x, g[ts][0], c.params, cfg) for ts in (False, True)}
    assert np.abs(h[False] - c["x_node"]).max() <= TOL and np.abs(h[True] - c["x_node_test"]).max() <= TOL
    worst = 0.0

    def logits(split, test_set, encoder_graph):
        batch = c.split_pairs(d, split).t().numpy()
        _, mask, ppr = g[test_set]
        return O.forward(batch, x, None, mask, ppr, c.params, cfg, x_node=h[encoder_graph])["logit"]

    for split in SPLITS:
        ts = split.startswith("test")
        # the reference encodes HeaRT negatives on the training graph whatever the split (testing.py:105)
        got = logits(split, ts, False if (c.heart and split.endswith("neg")) else ts)
        err = float(np.abs(got - c["logit." + split].reshape(-1)).max())
        worst = max(worst, err)
        assert err <= TOL, (split, err)
    if "logit.test_neg_fullgraph" in c:
        full = logits("test_neg", True, True)
        assert np.abs(full - c["logit.test_neg_fullgraph"].reshape(-1)).max() <= TOL
        assert np.abs(full - c["logit.test_neg"].reshape(-1)).max() > 1e-3      # the two encoders do differ
    print(f"{case}: worst oracle logit error {worst:.2e}")


@pytest.mark.parametrize("case", TRAIN_CASES)
def test_train_edges_mask_is_the_reference_masked_adjacency(case):
    from lpformer_amd import epoch
    c = Case(case, train=True)
    d = Case(case).read()
    n = int(d["num_nodes"])
    perm = torch.from_numpy(c["train_perm"])
    assert perm.numel() == 64 and perm.unique().numel() == 64
    te = epoch.TrainEdges(d["train_pos"], n)
    cov = te.covered(perm)
    cov = cov[:, cov[0] >= 0]
    gone = set((cov[0] * n + cov[1]).tolist()) | set((cov[1] * n + cov[0]).tolist())
    m = d["adj_mask"]
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(m.rowptr))
    resident = set((rows * n + np.asarray(m.col).astype(np.int64)).tolist())
    assert gone <= resident
    want = c["train_masked_index"].astype(np.int64)
    assert sorted(resident - gone) == (want[0] * n + want[1]).tolist()
    if case == "collab_valtest":     # (a) one row of a repeated pair inside, its twin outside: the edge stays; (b) both inside
        tp = d["train_pos"][perm]
        key = torch.minimum(tp[:, 0], tp[:, 1]) * n + torch.maximum(tp[:, 0], tp[:, 1])
        all_key = torch.minimum(d["train_pos"][:, 0], d["train_pos"][:, 1]) * n + torch.maximum(d["train_pos"][:, 0], d["train_pos"][:, 1])
        total = {int(k): int((all_key == k).sum()) for k in key.unique()}
        inside = {int(k): int((key == k).sum()) for k in key.unique()}
        assert any(total[k] >= 2 and inside[k] < total[k] for k in total)
        assert any(total[k] >= 2 and inside[k] == total[k] for k in total)
        assert int((cov[0] >= 0).sum()) < 64
