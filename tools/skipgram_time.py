"""Device time of one Node2Vec optimiser step, trainer="device" (lpformer_amd.skipgram) against trainer="torch" (the
nn.Embedding(sparse=True) + SparseAdam step of lpformer_amd.random_walks), on the collab-like and the ddi-like bench
graphs at node2vec_embeddings' defaults: dim 128, walk length 20, context 10, 1,280 walks per step, one negative walk
per walk, lr 0.01.  Both trainers step on the SAME walks and noise nodes, interleaved in one process (device, torch,
device, ...), each from its own copy of one initial table; a step is timed with a host clock around work that ends in
a synchronise, the median of LPF_REPS after one warm-up step each, with min and max.  A step covers what
node2vec_embeddings does per step behind the walks and the noise draw: for "device" writing the negative buffer and
skipgram_step; for "torch" cutting the windows, the loss, backward and SparseAdam.  Then the device step's parts, each
between two device events: the three C-ABI entries (through _lib.recording) and the torch-built occurrence list (sort,
unique_consecutive, cumulative sum, two gathers).  Then one whole node2vec_embeddings epoch each way (host clock,
after a warm-up epoch of a tenth of the walks).  Writes one JSON document.
    LPF_CFGS="collab ddi" LPF_REPS=7 LPF_OUT=profiles/skipgram_timing.json python tools/skipgram_time.py"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

CFGS = os.environ.get("LPF_CFGS", "collab ddi").split()
REPS = int(os.environ.get("LPF_REPS", "7"))
EPOCH = os.environ.get("LPF_EPOCH", "1") != "0"
OUT = os.environ.get("LPF_OUT", "profiles/skipgram_timing.json")
DIM, LENGTH, CONTEXT, WALKS_PER_NODE, BATCH, NUM_NEG, LR, SEED = 128, 20, 10, 10, 1280, 1, 0.01, 1


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


class Parts:
    """A _lib.recording recorder: every lpf_* call between two device events, by name."""

    def __init__(self, torch):
        self.torch, self.pairs = torch, []

    def events(self):
        return self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)

    def launch(self, name, fn):
        def call(*args):
            e0, e1 = self.events()
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

    def wrap(self, name, fn):
        def call(*args):
            e0, e1 = self.events()
            e0.record()
            out = fn(*args)
            e1.record()
            self.pairs.append((name, e0, e1))
            return out
        return call

    def totals(self):
        self.torch.cuda.synchronize()
        out = {}
        for name, e0, e1 in self.pairs:
            out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
        return out


def main():
    import torch
    from lpformer_amd import _lib, data as D, graph, skipgram
    import importlib
    RW = importlib.import_module("lpformer_amd.random_walks")      # (the package's attribute of that name is the function)

    assert torch.cuda.is_available(), "skipgram_time.py measures on an MI355X"
    dev = torch.device("cuda:0")
    res = {"reps": REPS, "dim": DIM, "walk_length": LENGTH, "context": CONTEXT, "walks_per_node": WALKS_PER_NODE,
           "batch_walks": BATCH, "num_neg": NUM_NEG, "lr": LR, "chunk": skipgram.CHUNK,
           "device": torch.cuda.get_device_properties(dev).gcnArchName, "torch": torch.__version__,
           "step_ms_covers": "host clock around one step that ends in a synchronise, walks and noise nodes already "
                             "drawn; device: negative buffer + skipgram_step; torch: windows, loss, backward, SparseAdam",
           "parts_ms_covers": "device events in front of and behind each C-ABI call and around occurrence_list "
                              "(torch: stable sort, unique_consecutive, cumsum, two gathers)"}
    for name in CFGS:
        cfg = D.CONFIGS[name]
        ei, _ = D.chung_lu_graph(cfg["n"], cfg["edges"], gamma=cfg["gamma"], seed=0, max_weight=cfg["max_weight"])
        g = graph.mask_csr(np.asarray(ei, np.int64), cfg["n"], symmetric=True).to_device(dev)
        n = int(g.n)
        r = res[name] = {"n": n, "nnz": int(g.nnz)}
        gen = torch.Generator(device=dev)
        gen.manual_seed(SEED)
        table0 = torch.randn((n, DIM), generator=gen, device=dev, dtype=torch.float32)
        m = min(BATCH, n * WALKS_PER_NODE)
        start = torch.randperm(n, generator=gen, device=dev).repeat(WALKS_PER_NODE)[:m]
        walks = RW.random_walks(g, start, length=LENGTH, seed=SEED).walks
        noise = torch.randint(n, (m * NUM_NEG, LENGTH), generator=gen, device=dev)

        table_d, state = table0.clone(), skipgram.skipgram_state(table0)
        emb = torch.nn.Embedding(n, DIM, sparse=True, _weight=table0.clone())
        opt = torch.optim.SparseAdam(list(emb.parameters()), lr=LR)

        def device_step():
            neg = torch.empty((LENGTH + 1, m * NUM_NEG), dtype=torch.int32, device=dev)
            neg[0] = start.repeat(NUM_NEG)
            neg[1:] = noise.t()
            return skipgram.skipgram_step(table_d, state, walks.t(), neg, CONTEXT, lr=LR)

        def torch_step():
            pos = RW._windows(walks, CONTEXT).reshape(-1, CONTEXT).to(torch.int64)
            neg = RW._windows(torch.cat([start.repeat(NUM_NEG)[:, None], noise], dim=1), CONTEXT).reshape(-1, CONTEXT)
            opt.zero_grad()
            loss = RW._skipgram_loss(emb, pos, neg)
            loss.backward()
            opt.step()
            return loss.detach()

        times = {"device": [], "torch": []}
        first = {}
        for rep in range(REPS + 1):                                # rep 0 warms both up
            for tag, fn in (("device", device_step), ("torch", torch_step)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loss = fn()
                torch.cuda.synchronize()
                if rep:
                    times[tag].append((time.perf_counter() - t0) * 1e3)
                else:
                    first[tag] = float(loss)
        r["step_ms"] = {k: spread(v) for k, v in times.items()}
        r["first_step_loss"] = first
        print(name, "step", json.dumps(r["step_ms"]), "first losses", first, flush=True)

        # the device step's parts
        parts = {}
        plain = skipgram.occurrence_list
        for rep in range(REPS):
            rec = Parts(torch)
            skipgram.occurrence_list = rec.wrap("occurrence_list_torch", plain)
            try:
                with _lib.recording(rec):
                    device_step()
            finally:
                skipgram.occurrence_list = plain
            for k, v in rec.totals().items():
                parts.setdefault(k, []).append(v)
        r["parts_ms"] = {k: spread(v) for k, v in parts.items()}
        print(name, "parts", json.dumps(r["parts_ms"]), flush=True)

        # the shape of one step's occurrence list
        M = 2 * m * (LENGTH + 2 - CONTEXT) * (CONTEXT - 1)
        ids = torch.empty(2 * M, dtype=torch.int32, device=dev)
        win = RW._windows(walks, CONTEXT)
        nwin = RW._windows(torch.cat([start.repeat(NUM_NEG)[:, None], noise], dim=1), CONTEXT)
        ids[:M] = torch.cat([win[:, :, :1].expand(-1, -1, CONTEXT - 1).reshape(-1),
                             nwin[:, :, :1].expand(-1, -1, CONTEXT - 1).reshape(-1)])
        ids[M:] = torch.cat([win[:, :, 1:].reshape(-1), nwin[:, :, 1:].reshape(-1)])
        rows, seg, _, _ = plain(ids)
        lens = (seg[1:] - seg[:-1]).cpu().numpy()
        r["occurrence_list"] = {"pairs": M, "occurrences": 2 * M, "rows_touched": int(rows.numel()),
                                "segment_median": float(np.median(lens)), "segment_max": int(lens.max()),
                                "rows_longer_than_chunk": int((lens > skipgram.CHUNK).sum()),
                                "chunks_of_longest": int(-(-int(lens.max()) // skipgram.CHUNK))}
        print(name, "list", json.dumps(r["occurrence_list"]), flush=True)
        del emb, opt, table_d, state

        if EPOCH:
            kw = dict(walk_length=LENGTH, context=CONTEXT, batch_walks=BATCH, num_neg=NUM_NEG, lr=LR, epochs=1, seed=SEED)
            r["epoch"] = {"steps": -(-n * WALKS_PER_NODE // BATCH)}
            for trainer in ("device", "torch"):
                RW.node2vec_embeddings(g, DIM, walks_per_node=1, trainer=trainer, **kw)      # warm-up: a tenth
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, losses = RW.node2vec_embeddings(g, DIM, walks_per_node=WALKS_PER_NODE, trainer=trainer, **kw)
                torch.cuda.synchronize()
                r["epoch"][trainer] = {"seconds": time.perf_counter() - t0, "loss": losses[0]}
            print(name, "epoch", json.dumps(r["epoch"]), flush=True)
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
