"""Time of lpformer_amd.communities on the collab-like and the ddi-like bench graphs: the whole call (host clock around
a call that ends in a synchronise), the kernel time of lpf_community_move per level (a device event pair around every
C-ABI call, collected through _lib.recording) and of lpf_community_quality, rounds and levels -- each the median of
LPF_REPS runs after a warm-up, with min and max -- with the listed rows' table in LDS (the default) and forced into
device memory (lds_slots = 64); and the baselines on one host process: the numpy restatement, whose result the device's
is compared with, and networkx.community.louvain_communities(seed=0) with its modularity.  Two phases, which may run
in separate calls (the second reads the document the first wrote): LPF_PHASES="host device".  Writes one JSON document.
    LPF_CFGS="collab ddi" LPF_REPS=7 LPF_OUT=profiles/communities_timing.json python tools/communities_time.py"""
import hashlib, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

CFGS = os.environ.get("LPF_CFGS", "collab ddi").split()
REPS = int(os.environ.get("LPF_REPS", "7"))
PHASES = os.environ.get("LPF_PHASES", "host device").split()
OUT = os.environ.get("LPF_OUT", "profiles/communities_timing.json")
LEVEL_ARG = 11                                   # lpf_community_move(..., two_m, seed, level, round, ...)


class EventPairs:
    """A _lib.recording recorder: every lpf_* call between two device events; lpf_community_move keyed by its level."""

    def __init__(self, torch):
        self.torch, self.pairs = torch, []

    def launch(self, name, fn):
        def call(*args):
            e0, e1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*args)
            e1.record()
            key = f"{name}[level {args[LEVEL_ARG]}]" if name == "lpf_community_move" else name
            self.pairs.append((key, e0, e1))
            return rc
        return call

    def keep(self, t):
        pass

    def wait(self, a, b):
        pass

    def per_entry(self):
        self.torch.cuda.synchronize()
        out = {}
        for name, e0, e1 in self.pairs:
            out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
        return out


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def digest(c):
    """What identifies a result: its labels, levels and numerator."""
    h = hashlib.sha256(c.label.cpu().numpy().tobytes())
    h.update(json.dumps([c.levels, c.quality_num, c.count], sort_keys=True).encode())
    return h.hexdigest()


def main():
    import torch
    from lpformer_amd import _lib, data as D, graph
    from lpformer_amd.community import communities, communities_reference

    res = {}
    if os.path.exists(OUT) and "host" not in PHASES:
        with open(OUT) as f:
            res = json.load(f)
    res.setdefault("runs", []).append(PHASES)    # one entry per invocation: the phases it ran
    res.update({"reps": REPS,
                "kernel_ms_covers": "sum over the launches of a call of the device time between an event recorded in "
                                    "front of the C-ABI call and one behind it, lpf_community_move per level",
                "call_ms_covers": "the whole communities call: torch allocations, the listed rows, every round's "
                                  "launches, index_add_ / bincount and scalar read-back, the coarse graphs (sort, "
                                  "unique_consecutive, index_add_), a final synchronise"})
    graphs = {}
    for name in CFGS:
        cfg = D.CONFIGS[name]
        ei, _ = D.chung_lu_graph(cfg["n"], cfg["edges"], gamma=cfg["gamma"], seed=0, max_weight=cfg["max_weight"])
        graphs[name] = graph.mask_csr(np.asarray(ei, np.int64), cfg["n"], symmetric=True)

    if "host" in PHASES:                         # nothing has touched the GPU yet
        import networkx as nx
        import scipy.sparse as sp
        for name, csr in graphs.items():
            lens = np.diff(csr.rowptr)
            r = res[name] = {"n": int(csr.n), "nnz": int(csr.nnz), "max_row": int(lens.max()),
                             "rows_over_LPF_COMM_LONG_ROW": int((lens > _lib.CONST["LPF_COMM_LONG_ROW"]).sum())}
            t0 = time.perf_counter()
            ref = communities_reference(csr)
            r["host"] = {"processes": 1, "seconds_restatement": time.perf_counter() - t0, "digest": digest(ref),
                         "modularity": ref.modularity, "communities": ref.count, "levels": ref.levels}
            print(f"{name}: restatement {r['host']['seconds_restatement']:.2f} s, Q = {ref.modularity:.4f}", flush=True)
            A = sp.csr_matrix((np.ones(csr.nnz), csr.col, csr.rowptr), shape=(csr.n, csr.n))
            A.setdiag(0)
            A.eliminate_zeros()
            G = nx.from_scipy_sparse_array(A)
            t0 = time.perf_counter()
            parts = nx.community.louvain_communities(G, seed=0)
            r["networkx"] = {"seconds_louvain_communities": time.perf_counter() - t0, "communities": len(parts),
                             "modularity": nx.community.modularity(G, parts), "version": nx.__version__}
            print(f"{name}: networkx {json.dumps(r['networkx'])}", flush=True)

    if "device" in PHASES:
        dev = torch.device("cuda:0")
        res["device"] = torch.cuda.get_device_properties(dev).gcnArchName
        res["torch"] = torch.__version__
        for name, csr in graphs.items():
            g = csr.to_device(dev)
            r = res.setdefault(name, {})
            first = communities(g)
            r["summary"] = first.summary()
            r["rounds"] = sum(lv["rounds"] for lv in first.levels)
            r["levels"] = first.levels
            if "host" in r:
                r["matches_host"] = digest(first) == r["host"]["digest"]
            r["two_runs_equal"] = digest(communities(g)) == digest(first)
            for label, kw in (("lds_table", {}), ("global_table", {"lds_slots": 64})):
                def call():
                    return communities(g, **kw)
                call()
                torch.cuda.synchronize()
                wall, kern, per_entry = [], [], {}
                for _ in range(REPS):
                    t0 = time.perf_counter()
                    c = call()
                    torch.cuda.synchronize()
                    wall.append((time.perf_counter() - t0) * 1e3)
                for _ in range(REPS):
                    rec = EventPairs(torch)
                    with _lib.recording(rec):
                        call()
                    per_entry = rec.per_entry()
                    kern.append(sum(v for k, v in per_entry.items() if k.startswith("lpf_community_move")))
                r[label] = {"call_ms": spread(wall), "move_kernel_ms": spread(kern),
                            "kernel_ms_by_entry_last_run": per_entry, "calls_in_last_run": len(rec.pairs),
                            "equals_first_run": digest(c) == digest(first)}
                print(name, label, json.dumps(r[label]), flush=True)
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
