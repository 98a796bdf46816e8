"""What tests/test_pipeline_host.py and tests/test_gpu_pipeline.py share: the fixtures of
tests/golden/make_pipeline_golden.py and the data dict ``lpformer_amd.readers`` builds for each of them from the
committed tiny datasets, under the seeds tests/test_readers.py uses."""
import json
import os

import numpy as np
import torch

from lpformer_amd import readers as R
from oracle.fixture_weights import make_state
from tests.golden_util import GOLDEN_DIR

CASES = ["tinycora", "tinycora_heart", "collab_valtest", "collab_valtest_heart", "ppa_heart", "ddi", "citation2"]
TRAIN_CASES = ["collab_valtest", "ddi", "citation2"]
SPLITS = ("train_pos_val", "valid_pos", "test_pos", "valid_neg", "test_neg")
TOL = 1e-4              # the project's logit tolerance (tests/test_gpu_parity.py)
F32_MEAN_TOL = 2e-6     # the reference's metrics are float32 means (bound derived in tests/test_metrics_host.py)
ARG_KEYS = ("thresh_cn", "thresh_1hop", "thresh_non1hop", "dim", "trans_layers", "num_heads", "att_drop", "dropout",
            "gnn_drop", "feat_drop", "gcn_cache", "gnn_layers", "residual", "layer_norm", "relu")


class Case:
    def __init__(self, name, train=False):
        self.name = name
        self.z = np.load(os.path.join(GOLDEN_DIR, f"pipeline_{name}{'_train' if train else ''}.npz"))
        self.cfg = json.loads(str(self.z["config_json"]))
        self.params = make_state(self.cfg["param_shapes"], self.cfg["seed"])
        self.heart = bool(self.cfg["heart"])
        self.layout = self.cfg["layout"]
        self.batch_size = int(self.cfg["batch_size"])
        self.ks = tuple(self.cfg["k_list"])

    def __getitem__(self, k):
        return self.z[k]

    def __contains__(self, k):
        return k in self.z.files

    def args(self, **over):
        return dict({k: self.cfg[k] for k in ARG_KEYS}, **over)

    def state_dicts(self):
        m = {k[len("model."):]: torch.from_numpy(v) for k, v in self.params.items() if k.startswith("model.")}
        s = {k[len("score."):]: torch.from_numpy(v) for k, v in self.params.items() if k.startswith("score.")}
        return m, s

    def read(self):
        """The reader's dict, exactly as ``lpformer_amd.readers`` returns it."""
        cfg = self.cfg
        if cfg["dataset"] == "tinycora":
            src = os.path.join(GOLDEN_DIR, "planetoid_tiny")
            torch.manual_seed(11)
            return R.read_data_planetoid(src, "tinycora", eps=cfg["eps"],
                                         heart_dir=os.path.join(src, "heart") if self.heart else None)
        root = os.path.join(GOLDEN_DIR, "ogb_tiny")
        torch.manual_seed(5)
        return R.read_data_ogb(root, cfg["dataset"], eps=cfg["eps"], dim=cfg["dim"], use_val_in_test=cfg["use_val_in_test"],
                               heart_dir=os.path.join(root, "heart") if self.heart else None)

    def metric_names(self, variant=""):
        pre = f"metric.{variant}"
        return [k[len(pre):] for k in self.z.files if k.startswith(pre) and "." not in k[len(pre):]]

    def split_pairs(self, data, split):
        """[P, 2] pairs of a split in the order the recorded scores are flattened."""
        t = data[split]
        if t.dim() == 3:
            return t.reshape(-1, 2)
        if t.dim() == 2 and t.shape[1] != 2 or (self.cfg["dataset"] == "ogbl-citation2" and split.endswith("neg")):
            pos = data[split.replace("neg", "pos")]
            return torch.stack((pos[:, :1].expand_as(t), t), dim=-1).reshape(-1, 2)
        return t
