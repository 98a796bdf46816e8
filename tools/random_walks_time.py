"""Device time of lpformer_amd.random_walks on the collab-like and the ddi-like bench graphs: every node x 10 walks of
length 40, at (p, q) = (1, 1) and (0.25, 4), in both kernel forms -- the kernel alone (a device event pair around the
C-ABI call, collected through _lib.recording) and the whole call (host clock around a call that ends in a synchronise),
each the median of LPF_REPS runs after a warm-up, with min and max.  Baselines: (a) the numpy restatement on one host
process, timed on the first LPF_HOST_WALKS walks and SCALED to the whole list (said so in the output), whose walks the
device's are compared with; (b) for p = q = 1 a torch-only walker on the same device, L rounds of
col[rowptr[cur] + floor(rand * deg)].  Then one node2vec_embeddings epoch at its defaults, split into the time of its
random_walks calls and the rest (the skip-gram update in torch).  Writes one JSON document.
    LPF_CFGS="collab ddi" LPF_REPS=7 LPF_OUT=profiles/random_walks_timing.json python tools/random_walks_time.py"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

CFGS = os.environ.get("LPF_CFGS", "collab ddi").split()
REPS = int(os.environ.get("LPF_REPS", "7"))
HOST_WALKS = int(os.environ.get("LPF_HOST_WALKS", "16384"))
EPOCH = os.environ.get("LPF_EPOCH", "1") != "0"
OUT = os.environ.get("LPF_OUT", "profiles/random_walks_timing.json")
WALKS_PER_NODE, LENGTH, SEED = 10, 40, 0
PQ = ((1.0, 1.0), (0.25, 4.0))


class EventPairs:
    """A _lib.recording recorder: every lpf_* call between two device events."""

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

    def total(self):
        self.torch.cuda.synchronize()
        return sum(e0.elapsed_time(e1) for _, e0, e1 in self.pairs)


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def torch_walker(torch, g, starts, length):
    """The first-order walk in plain torch: per step one uniform draw, one multiply, two gathers."""
    cur = starts
    out = [cur]
    for _ in range(length):
        lo = g.rowptr[cur]
        deg = g.rowptr[cur + 1] - lo
        pick = (torch.rand(cur.shape, device=cur.device, dtype=torch.float64) * deg).long()
        nxt = g.col[(lo + torch.minimum(pick, (deg - 1).clamp(min=0))).clamp(max=g.col.numel() - 1)].long()
        cur = torch.where(deg > 0, nxt, cur)
        out.append(cur)
    return torch.stack(out, dim=1)


def main():
    import torch
    from lpformer_amd import _lib, data as D, graph, sources
    from lpformer_amd.random_walks import node2vec_embeddings, random_walks, walks_reference

    res = {"reps": REPS, "walks_per_node": WALKS_PER_NODE, "length": LENGTH, "seed": SEED,
           "kernel_ms_covers": "the device time between an event recorded in front of the lpf_random_walks call and one "
                               "behind it",
           "call_ms_covers": "the whole random_walks call: the start list (arange, repeat), two torch allocations, the "
                             "launch, a final synchronise",
           "host_covers": f"walks_reference on one process for the first {HOST_WALKS} walks of the list, and that time "
                          "scaled by (walks of the list) / (walks timed): an extrapolation, not a run"}
    graphs = {}
    for name in CFGS:
        cfg = D.CONFIGS[name]
        ei, _ = D.chung_lu_graph(cfg["n"], cfg["edges"], gamma=cfg["gamma"], seed=0, max_weight=cfg["max_weight"])
        graphs[name] = graph.mask_csr(np.asarray(ei, np.int64), cfg["n"], symmetric=True)

    # the host baseline first: nothing has touched the GPU yet
    ref = {}
    for name, csr in graphs.items():
        n = int(csr.n)
        W = n * WALKS_PER_NODE
        r = res[name] = {"n": n, "nnz": int(csr.nnz), "max_row": int(np.diff(csr.rowptr).max()), "walks": W, "host": {}}
        m = min(HOST_WALKS, W)
        head = torch.arange(n, dtype=torch.int64).repeat(WALKS_PER_NODE)[:m]
        for p, q in PQ:
            t0 = time.perf_counter()
            ref[name, p, q] = walks_reference(csr, head, length=LENGTH, p=p, q=q, seed=SEED)
            dt = time.perf_counter() - t0
            r["host"][f"p{p}_q{q}"] = {"walks_timed": m, "seconds_timed": dt, "seconds_scaled_to_all_walks": dt * W / m}
            print(f"{name}: host p={p} q={q}: {m} walks {dt:.2f} s, scaled {dt * W / m:.1f} s", flush=True)
        r["host"]["processes"] = 1

    dev = torch.device("cuda:0")
    res["device"] = torch.cuda.get_device_properties(dev).gcnArchName
    res["torch"] = torch.__version__
    for name, csr in graphs.items():
        g = csr.to_device(dev)
        r = res[name]
        for p, q in PQ:
            tag = f"p{p}_q{q}"
            r[tag] = {}
            outs = {}
            for form in ("lane", "group8"):
                def call():
                    return random_walks(g, None, length=LENGTH, walks_per_node=WALKS_PER_NODE, p=p, q=q, seed=SEED,
                                        form=form)
                outs[form] = call()
                torch.cuda.synchronize()
                wall, kern = [], []
                for _ in range(REPS):
                    t0 = time.perf_counter()
                    call()
                    torch.cuda.synchronize()
                    wall.append((time.perf_counter() - t0) * 1e3)
                for _ in range(REPS):
                    rec = EventPairs(torch)
                    with _lib.recording(rec):
                        call()
                    kern.append(rec.total())
                r[tag][form] = {"call_ms": spread(wall), "kernel_ms": spread(kern)}
                print(name, tag, form, json.dumps(r[tag][form]), flush=True)
            a, b = outs["lane"], outs["group8"]
            m = ref[name, p, q].walks.shape[0]
            r[tag]["forms_equal"] = bool(torch.equal(a.walks, b.walks) and torch.equal(a.forced, b.forced))
            r[tag]["matches_host_on_walks_timed"] = bool(torch.equal(a.walks[:m].cpu(), ref[name, p, q].walks) and
                                                         torch.equal(a.forced[:m].cpu(), ref[name, p, q].forced))
            r[tag]["forced_steps"] = int(a.forced.sum())
            r[tag]["steps"] = int(a.forced.numel()) * LENGTH
        # (b) the torch-only first-order walker
        starts = torch.arange(g.n, dtype=torch.int64, device=dev).repeat(WALKS_PER_NODE)
        torch_walker(torch, g, starts, LENGTH)
        torch.cuda.synchronize()
        wall = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            torch_walker(torch, g, starts, LENGTH)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        r["torch_walker_p1_q1"] = {"call_ms": spread(wall), "note": "start list made outside the timed region; int64 "
                                   "walks [W, L + 1] stacked inside it"}
        print(name, "torch walker", json.dumps(r["torch_walker_p1_q1"]), flush=True)
        del starts
        if EPOCH:
            # one node2vec_embeddings epoch at its defaults, and its random_walks calls alone (same chunks)
            kw = dict(walk_length=20, walks_per_node=10, batch_walks=1280)
            node2vec_embeddings(g, 128, epochs=1, seed=1, **dict(kw, walks_per_node=1))      # warm-up: a tenth
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, losses = node2vec_embeddings(g, 128, epochs=1, seed=1, **kw)
            torch.cuda.synchronize()
            epoch_s = time.perf_counter() - t0
            order = torch.arange(g.n, dtype=torch.int64, device=dev).repeat(kw["walks_per_node"])
            t0 = time.perf_counter()
            for lo, m in sources.chunks(order.numel(), kw["batch_walks"]):
                random_walks(g, order[lo:lo + m], length=kw["walk_length"], seed=1, walk_base=lo)
            torch.cuda.synchronize()
            walk_s = time.perf_counter() - t0
            r["node2vec_epoch"] = dict(kw, dim=128, context=10, num_neg=1, steps=-(-order.numel() // kw["batch_walks"]),
                                       epoch_seconds=epoch_s, random_walks_calls_seconds=walk_s,
                                       skipgram_and_rest_seconds=epoch_s - walk_s, loss=losses[0])
            print(name, "node2vec epoch", json.dumps(r["node2vec_epoch"]), flush=True)
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
