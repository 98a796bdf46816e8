"""Device time of common-neighbour pooling (lpformer_amd.ncn.cn_pool) on 32,768 held-out positives of the collab-like
and the ddi-like bench graphs, D = 128 and 256, weights none and "aa"; forward, and forward + backward.  The positives
are edges drawn from the graph's edge list and removed from it, so the adjacency is a training graph.

Per (graph, D, weights), the median of LPF_REPS with min and max, after one warm-up:
    kernel_ms          device events in front of and behind each C-ABI call (through _lib.recording), by entry: the
                       forward entry only -- autograd runs the backward on a thread of its own, which a recording does
                       not follow
    forward_ms         host clock around cn_pool(...) without a gradient, ending in a synchronise
    train_ms           host clock around cn_pool(...) with table.requires_grad and pool.backward(g), ending in one
    index_add_*        torch on the same device from the READY entry list: zeros.index_add_(0, pair, w[node] T[node]),
                       forward alone and with autograd's backward (the list itself is not charged to it)
    dense_rows_*       the reference's way (src/train/eval.py:21-41) with the gather added: per LPF_DENSE_ROWS pairs the
                       dense rows adj[a].to_dense() * adj[b].to_dense() ([rows, N]) times diag(w) T; timed on the first
                       LPF_DENSE_PAIRS pairs (median of at most 3) and scaled to all of them
    host_reference_s   cn_pool_reference on one host process (fp64), once, on the first LPF_HOST_PAIRS pairs and scaled
No pass / fail threshold.  This process never touches the GPU: every (graph) is a child process of its own under
LPF_STEP_TIMEOUT seconds, and the first child that fails or runs out of time ends the run.
    LPF_CFGS="collab ddi" LPF_REPS=7 LPF_OUT=profiles/cn_pool_timing.json python tools/cn_pool_time.py"""
import json, os, statistics, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

CFGS = os.environ.get("LPF_CFGS", "collab ddi").split()
REPS = int(os.environ.get("LPF_REPS", "7"))
OUT = os.environ.get("LPF_OUT", "profiles/cn_pool_timing.json")
STEP_TIMEOUT = int(os.environ.get("LPF_STEP_TIMEOUT", "420"))
DENSE_ROWS = int(os.environ.get("LPF_DENSE_ROWS", "512"))
DENSE_PAIRS = int(os.environ.get("LPF_DENSE_PAIRS", "4096"))
HOST_PAIRS = int(os.environ.get("LPF_HOST_PAIRS", "2048"))
PAIRS, DIMS, WEIGHTS, SEED = 32768, (128, 256), ("none", "aa"), 1


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


class Parts:
    """A _lib.recording recorder: every lpf_* call between two device events, by name."""

    def __init__(self, torch):
        self.torch, self.pairs = torch, []

    def launch(self, name, fn):
        def call(*args):
            e0, e1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*args)
            e1.record()
            self.pairs.append((name, e0, e1))
            return rc
        return call

    def keep(self, t):
        pass

    def wait(self, a, b):
        pass

    def totals(self):
        self.torch.cuda.synchronize()
        out = {}
        for name, e0, e1 in self.pairs:
            out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
        return out


def step(name):
    """One graph, in a process of its own: prints one JSON line."""
    import torch
    from lpformer_amd import _lib, data as D, graph, heuristics, ncn

    assert torch.cuda.is_available(), "cn_pool_time.py measures on an MI355X"
    dev = torch.device("cuda:0")
    cfg = D.CONFIGS[name]
    ei, _ = D.chung_lu_graph(cfg["n"], cfg["edges"], gamma=cfg["gamma"], seed=0, max_weight=cfg["max_weight"])
    ei = np.asarray(ei, np.int64)
    ei = np.unique(np.sort(ei[:, ei[0] != ei[1]], axis=0), axis=1)                 # undirected, once each
    held = np.random.default_rng(SEED).choice(ei.shape[1], PAIRS, replace=False)
    keep = np.ones(ei.shape[1], bool)
    keep[held] = False
    csr = graph.mask_csr(ei[:, keep], cfg["n"], symmetric=True)
    g = csr.to_device(dev)
    n = int(g.n)
    pairs = torch.from_numpy(ei[:, held]).to(dev).contiguous()
    ent = ncn.cn_entries(g, pairs)
    cn = (ent.seg[1:] - ent.seg[:-1])
    pos = torch.repeat_interleave(torch.arange(PAIRS, device=dev), cn)
    node = ent.node.to(torch.int64)
    r = {"n": n, "nnz": int(g.nnz), "pairs": PAIRS, "entries": int(node.numel()), "cn_max": int(cn.max()),
         "cn_median": float(cn.float().median()), "pairs_without": int((cn == 0).sum()),
         "device": torch.cuda.get_device_properties(dev).gcnArchName, "torch": torch.__version__}
    adj = torch.sparse_coo_tensor(torch.stack([torch.repeat_interleave(torch.arange(n, device=dev),
                                                                       g.rowptr[1:] - g.rowptr[:-1]),
                                               g.col.to(torch.int64)]),
                                  torch.ones(int(g.nnz), device=dev), (n, n)).coalesce()

    def timed(fn, reps=REPS):
        out = []
        for rep in range(reps + 1):                                # rep 0 warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                out.append((time.perf_counter() - t0) * 1e3)
        return spread(out)

    for dim in DIMS:
        gen = torch.Generator(device=dev)
        gen.manual_seed(SEED)
        table = torch.randn((n, dim), generator=gen, device=dev)
        up = torch.randn((PAIRS, dim), generator=gen, device=dev)
        for kind in WEIGHTS:
            w = None if kind == "none" else heuristics.weight_tables(g)[0]
            key = f"D{dim}_{kind}"
            q = r[key] = {}
            leaf = table.clone().requires_grad_(True)

            def train():
                leaf.grad = None
                ncn.cn_pool(g, pairs, leaf, weights=kind).backward(up)

            q["forward_ms"] = timed(lambda: ncn.cn_pool(g, pairs, table, weights=kind))
            q["train_ms"] = timed(train)
            parts = {}
            for rep in range(REPS):
                rec = Parts(torch)
                with _lib.recording(rec):
                    train()
                for k, v in rec.totals().items():
                    parts.setdefault(k, []).append(v)
            q["kernel_ms"] = {k: spread(v) for k, v in parts.items()}

            def rows_of(t):
                return t[node] if w is None else w[node, None] * t[node]

            def index_add(t):
                return torch.zeros((PAIRS, dim), device=dev).index_add_(0, pos, rows_of(t))

            def index_add_train():
                leaf.grad = None
                index_add(leaf).backward(up)

            q["index_add_forward_ms"] = timed(lambda: index_add(table))
            q["index_add_train_ms"] = timed(index_add_train)

            def dense_rows():
                wt = table if w is None else w[:, None] * table
                out = torch.empty((DENSE_PAIRS, dim), device=dev)
                for lo in range(0, DENSE_PAIRS, DENSE_ROWS):
                    a, b = pairs[0, lo:lo + DENSE_ROWS], pairs[1, lo:lo + DENSE_ROWS]
                    both = adj.index_select(0, a).to_dense() * adj.index_select(0, b).to_dense()
                    out[lo:lo + DENSE_ROWS] = both @ wt
                return out

            q["dense_rows_forward_ms"] = {k: v * PAIRS / DENSE_PAIRS
                                          for k, v in timed(dense_rows, reps=min(REPS, 3)).items()}
            worst = float((ncn.cn_pool(g, pairs, table, weights=kind) - index_add(table)).abs().max())
            q["max_abs_difference_to_index_add"] = worst
            print(name, key, json.dumps(q), file=sys.stderr, flush=True)
    t0 = time.perf_counter()
    ncn.cn_pool_reference(csr, pairs[:, :HOST_PAIRS].cpu(), torch.randn(n, DIMS[0]), None)
    took = time.perf_counter() - t0
    r["host_reference_s"] = {"dim": DIMS[0], "pairs_timed": HOST_PAIRS, "seconds_timed": took,
                             "seconds_scaled": took * PAIRS / HOST_PAIRS}
    print(json.dumps(r), flush=True)


def main():
    res = {"reps": REPS, "dense_rows_per_chunk": DENSE_ROWS, "dense_pairs_timed": DENSE_PAIRS, "chunk": 64,
           "forward_ms_covers": "host clock around cn_pool without a gradient, ending in a synchronise",
           "train_ms_covers": "host clock around cn_pool with a gradient and pool.backward(g), ending in a synchronise",
           "kernel_ms_covers": "device events in front of and behind each C-ABI call made on the calling thread: the "
                               "forward entry (autograd runs the backward on a thread of its own, which a recording "
                               "does not follow)"}
    for name in CFGS:                                               # a child per graph, under its own time limit
        try:
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], timeout=STEP_TIMEOUT,
                                  stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            sys.exit(f"cn_pool_time: the step {name} ran past {STEP_TIMEOUT} s; nothing more is started")
        if done.returncode != 0:
            sys.exit(f"cn_pool_time: the step {name} ended with status {done.returncode}; nothing more is started")
        res[name] = json.loads(done.stdout.strip().splitlines()[-1])
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--step":
        step(sys.argv[2])
    else:
        main()
