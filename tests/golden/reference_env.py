"""What the fixture generators share when they run the REFERENCE's readers on the committed tiny datasets
(tests/golden/planetoid_tiny/, tests/golden/ogb_tiny/): the stand-in for the OGB package's dataset class and the
PPR call without the reference's disk cache.  Used by make_reader_golden.py and make_pipeline_golden.py; nothing
here is reference code."""
import io
import os
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PLANETOID_DIR = os.path.join(HERE, "planetoid_tiny")
OGB_DIR = os.path.join(HERE, "ogb_tiny")
OGB_SPLIT = {"ogbl-collab": ("time", True), "ogbl-ppa": ("throughput", True), "ogbl-ddi": ("target", True),
             "ogbl-citation2": ("time", False)}


class _Data:
    """What the reference touches of a PyG ``Data`` object (read_datasets.py:31-129)."""
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def to(self, device):
        return self

    def __getitem__(self, k):
        return getattr(self, k)

    def __setitem__(self, k, v):
        setattr(self, k, v)


class _OgbDataset:
    """Stand-in for ``ogb.linkproppred.PygLinkPropPredDataset`` over the tiny raw files: the graph object as the OGB
    package is DOCUMENTED to build it -- edge list from raw/edge.csv.gz with the inverse edges appended for the
    undirected datasets (edge features repeated), float node features, [E, 1] edge attributes -- and the split
    dictionaries of split/<type>/*.pt.  (The package itself is not available offline: this part of the pipeline -- files to
    graph object -- stays an assumption of lpformer_amd/readers.py; everything the REFERENCE does with the object is what
    the generators record.)"""
    def __init__(self, name):
        import gzip
        self.name = name
        base = os.path.join(OGB_DIR, name.replace("-", "_"))
        split_type, add_inverse = OGB_SPLIT[name]

        def csv(fn, dt):
            path = os.path.join(base, "raw", fn)
            if not os.path.isfile(path):
                return None
            with gzip.open(path, "rt") as f:
                return np.loadtxt(f, delimiter=",", dtype=dt, ndmin=2)
        e = csv("edge.csv.gz", np.int64).T
        n = int(csv("num-node-list.csv.gz", np.int64).reshape(-1)[0])
        feat, w, yr = csv("node-feat.csv.gz", np.float32), csv("edge_weight.csv.gz", np.int64), csv("edge_year.csv.gz", np.int64)
        rep = (lambda a: None if a is None else torch.from_numpy(np.concatenate([a, a]) if add_inverse else a))
        ei = np.concatenate([e, e[::-1]], axis=1) if add_inverse else e
        self._data = _Data(num_nodes=n, edge_index=torch.from_numpy(np.ascontiguousarray(ei)),
                           x=None if feat is None else torch.from_numpy(feat), edge_weight=rep(w), edge_year=rep(yr))
        self._split = {s: torch.load(os.path.join(base, "split", split_type, f"{s}.pt")) for s in ("train", "valid", "test")}

    def __getitem__(self, i):
        return self._data

    def get_edge_split(self):
        return self._split


def patch_reference_readers(rd, cps):
    """Point the reference's ``util.read_datasets`` module ``rd`` at the committed tiny datasets: the OGB stand-in for its
    dataset class, and its own ``get_ppr_matrix`` / ``create_sparse_ppr_matrix`` (module ``cps``) without the disk cache
    (``get_ppr`` writes under the reference tree)."""
    def get_ppr_no_disk(dataset, edge_index, num_nodes, alpha, eps, is_val):
        nb, w = cps.get_ppr_matrix(edge_index, num_nodes, alpha, eps)
        return cps.create_sparse_ppr_matrix(nb, w).to_torch_sparse_coo_tensor()
    rd.get_ppr = get_ppr_no_disk
    rd.PygLinkPropPredDataset = lambda name: _OgbDataset(name)


def save_npz_stable(path, arrays):
    """``np.savez_compressed`` with a fixed member timestamp: the same arrays give the same bytes on every run."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key, val in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())
