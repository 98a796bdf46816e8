"""Record what the reference's evaluation code computes, as fixtures for tests/test_metrics_host.py and
tests/test_gpu_metrics.py:

    python tests/golden/make_metrics_golden.py --reference /path/to/reference

It imports the reference's ``src/train/evaluation.py`` unmodified (torch and sklearn only) and writes
``tests/golden/metrics_<case>.npz``: inputs and recorded outputs, no program text.

Recorded per case
* rows layout (pos [P] against neg_rows [P, K]): ``evaluate_mrr`` (float32 means), ``get_ranking_list``,
  ``sample_level_hits``; and mean(1 / rank) of that ranking list taken in fp64;
* shared layout (pos_train / pos [P], pos_test [Pt] against neg [M] / neg_test [Mt]): ``get_metric_score`` with the
  reference's own ``neg.repeat(P, 1)`` (MRR as float32 means, Hits through the stand-in below), the ranking list of that
  repeat and its fp64 mean reciprocal; ``evaluate_auc`` (rounded to 4 places) and sklearn's unrounded
  ``roc_auc_score`` / ``average_precision_score`` on the same vectors (``has_auc`` = 0 where sklearn refuses the
  input: it rejects infinities).

Hits@K in the reference comes from an ``ogb`` Evaluator, which is not a dependency here.  ``StandInHits`` below is a
STAND-IN of a few lines for ``Evaluator(name='ogbl-collab').eval`` with the documented OGB rule, not the ogb code.
"""
import sys

sys.dont_write_bytecode = True   # nothing may be written into the reference tree

import argparse          # noqa: E402
import importlib.util    # noqa: E402
import os                # noqa: E402

import numpy as np       # noqa: E402
import torch             # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
KS = (20, 50, 100)


class StandInHits:
    """STAND-IN for the ogb hits@K evaluator: the fraction of positives strictly above the K-th largest negative;
    1.0 when there are fewer than K negatives."""
    K = None

    def eval(self, d):
        pos, neg = d["y_pred_pos"], d["y_pred_neg"]
        if len(neg) < self.K:
            return {f"hits@{self.K}": 1.0}
        kth = torch.topk(neg, self.K)[0][-1]
        return {f"hits@{self.K}": float(torch.sum(pos > kth).cpu()) / len(pos)}


def load_reference(root):
    path = os.path.join(root, "src", "train", "evaluation.py")
    spec = importlib.util.spec_from_file_location("reference_evaluation", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def draw(kind, rng, shape):
    if kind == "continuous":
        return rng.random(shape, dtype=np.float32)
    if kind == "quantised":   # about 8 levels: heavy ties inside and across the classes
        return (np.floor(rng.random(shape) * 8) / 8).astype(np.float32)
    if kind == "equal":
        return np.full(shape, 0.25, dtype=np.float32)
    if kind == "inf":
        x = rng.standard_normal(shape).astype(np.float32)
        flat = x.reshape(-1)
        idx = rng.permutation(flat.size)[:max(2, flat.size // 10)]
        flat[idx[::2]] = np.inf
        flat[idx[1::2]] = -np.inf
        return x
    raise ValueError(kind)


# name: (kind, P, M, K of the rows layout, P of the test split, M of the test split)
CASES = {
    "continuous": ("continuous", 300, 500, 37, 211, 450),
    "quantised": ("quantised", 300, 500, 37, 211, 450),
    "equal": ("equal", 64, 130, 9, 40, 77),
    "p1": ("continuous", 1, 200, 25, 1, 120),
    "m1": ("quantised", 50, 1, 1, 30, 1),          # M = 1 shared; K = 1 rows
    "m_lt_k": ("continuous", 40, 15, 5, 25, 19),   # fewer shared negatives than any K of KS
    "inf": ("inf", 120, 260, 21, 90, 150),
}


def away_from_boundary(x):
    """Whether round(x, 4) is stable: x lies at least 1e-6 from a rounding boundary."""
    frac = (x * 1e4) % 1.0
    return abs(frac - 0.5) >= 1e-2


def record(ref, name, seed):
    from sklearn.metrics import average_precision_score, roc_auc_score
    kind, P, M, K, Pt, Mt = CASES[name]
    rng = np.random.default_rng(seed)
    z = {"ks": np.asarray(KS, np.int64), "seed": np.int64(seed)}
    for key, shape in (("pos", P), ("pos_train", P), ("neg", M), ("neg_rows", (P, K)), ("pos_test", Pt),
                       ("neg_test", Mt)):
        z[key] = draw(kind, rng, shape)
    t = {k: torch.from_numpy(v) for k, v in z.items() if k not in ("ks", "seed")}
    # rows layout
    res = ref.evaluate_mrr(t["pos"], t["neg_rows"])
    for k, v in res.items():
        z["rows_" + k] = np.float64(v)
    rl = ref.get_ranking_list(t["pos"], t["neg_rows"])
    z["rows_ranking_list"] = rl.numpy().astype(np.float32)
    z["rows_mrr64"] = np.float64((1.0 / rl.double()).mean().item())
    for k, v in ref.sample_level_hits(t["pos"], t["neg_rows"]).items():
        z["rows_sample_" + k] = v.numpy()
    # shared layout, through the reference's own repeat
    out = ref.get_metric_score(StandInHits(), object(), t["pos_train"], t["pos"], t["neg"], t["pos_test"],
                               t["neg_test"], k_list=list(KS))
    for k, v in out.items():
        z["split_" + k] = np.asarray(v, np.float64)
    mrr64 = []
    for tag, p, n in (("train", "pos_train", "neg"), ("valid", "pos", "neg"), ("test", "pos_test", "neg_test")):
        rl = ref.get_ranking_list(t[p], t[n].repeat(t[p].size(0), 1))
        z[f"shared_ranking_list_{tag}"] = rl.numpy().astype(np.float32)
        mrr64.append((1.0 / rl.double()).mean().item())
        for k, v in ref.sample_level_hits(t[p], t[n].repeat(t[p].size(0), 1)).items():
            z[f"shared_sample_{tag}_{k}"] = v.numpy()
    z["split_mrr64"] = np.asarray(mrr64, np.float64)
    # AUC / AP on the valid split: the reference's rounded values and sklearn's unrounded ones
    pred = np.concatenate([z["pos"], z["neg"]])
    true = np.concatenate([np.ones(P, np.int64), np.zeros(M, np.int64)])
    try:
        auc, ap = float(roc_auc_score(true, pred)), float(average_precision_score(true, pred))
        rounded = ref.evaluate_auc(torch.from_numpy(pred), torch.from_numpy(true))
    except ValueError:     # sklearn refuses infinities
        z["has_auc"] = np.int64(0)
        return z, True
    z["has_auc"] = np.int64(1)
    z["auc"], z["ap"] = np.float64(auc), np.float64(ap)
    z["auc_rounded"], z["ap_rounded"] = np.float64(rounded["AUC"]), np.float64(rounded["AP"])
    return z, away_from_boundary(auc) and away_from_boundary(ap)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    ref = load_reference(args.reference)
    for i, name in enumerate(CASES):
        for seed in range(100 * i, 100 * i + 50):
            z, ok = record(ref, name, seed)
            if ok:
                break
        else:
            raise SystemExit(f"{name}: no seed keeps AUC / AP away from a rounding boundary")
        path = os.path.join(args.out, f"metrics_{name}.npz")
        np.savez_compressed(path, **z)
        print(f"{path}: seed {int(z['seed'])}, {os.path.getsize(path)} bytes, has_auc = {int(z['has_auc'])}")


if __name__ == "__main__":
    main()
