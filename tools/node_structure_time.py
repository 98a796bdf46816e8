"""Device time of lpformer_amd.node_structure on the collab-like and the ddi-like bench graphs, per kind: the kernel time
summed over the launches (a device event pair around every C-ABI call, collected through _lib.recording), the time of
the whole call (host clock around a call that ends in a synchronise, events off), the launches the iterative kernels
made -- each the median of LPF_REPS runs after a warm-up, with min and max -- and the numpy / scipy restatement on one
host process, the only baseline there is, whose result the device's is compared with.  The core sweep is timed in both
forms of the long-row h-index (LDS histogram, bisection).  Writes one JSON document.
    LPF_CFGS="collab ddi" LPF_REPS=7 LPF_OUT=profiles/node_structure_timing.json python tools/node_structure_time.py"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

CFGS = os.environ.get("LPF_CFGS", "collab ddi").split()
REPS = int(os.environ.get("LPF_REPS", "7"))
SWEEPS_PER_READ = int(os.environ.get("LPF_SWEEPS_PER_READ", "8"))
OUT = os.environ.get("LPF_OUT", "profiles/node_structure_timing.json")


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

    def per_entry(self):
        self.torch.cuda.synchronize()
        out = {}
        for name, e0, e1 in self.pairs:
            out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
        return out


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def main():
    import torch
    from lpformer_amd import _lib, data as D, graph
    from lpformer_amd.structure import KINDS, node_structure, structure_reference

    res = {"reps": REPS, "sweeps_per_read": SWEEPS_PER_READ,
           "kernel_ms_covers": "sum over the launches of a call of the device time between an event recorded in front "
                               "of the C-ABI call and one behind it (core: lpf_node_degree + every lpf_core_sweep; "
                               "component: every lpf_components_hook and _jump; triangles: memset, three launches)",
           "call_ms_covers": "the whole node_structure call for that kind alone: torch allocations, the long-row list "
                             "or the entry-row table (cached per graph after the first call), the launches, the "
                             "read-back of every batch of counters, a final synchronise"}
    graphs = {}
    for name in CFGS:
        cfg = D.CONFIGS[name]
        ei, _ = D.chung_lu_graph(cfg["n"], cfg["edges"], gamma=cfg["gamma"], seed=0, max_weight=cfg["max_weight"])
        graphs[name] = graph.mask_csr(np.asarray(ei, np.int64), cfg["n"], symmetric=True)

    # the host baseline first: nothing has touched the GPU yet
    ref = {}
    for name, csr in graphs.items():
        r = res[name] = {"n": int(csr.n), "nnz": int(csr.nnz), "max_row": int(np.diff(csr.rowptr).max()), "host": {}}
        for k in KINDS:
            t0 = time.perf_counter()
            ref[name, k] = getattr(structure_reference(csr, kinds=(k,)), k)
            r["host"][f"seconds_{k}"] = time.perf_counter() - t0
            print(f"{name}: host {k} {r['host'][f'seconds_{k}']:.2f} s", flush=True)
        r["host"]["processes"] = 1

    dev = torch.device("cuda:0")
    res["device"] = torch.cuda.get_device_properties(dev).gcnArchName
    res["torch"] = torch.__version__
    for name, csr in graphs.items():
        g = csr.to_device(dev)
        r = res[name]
        full = node_structure(g, sweeps_per_read=SWEEPS_PER_READ)
        r["summary"] = full.summary()
        r["matches_host"] = {k: bool(torch.equal(getattr(full, k).cpu(), ref[name, k])) for k in KINDS}
        again = node_structure(g, sweeps_per_read=1)
        r["two_runs_equal"] = all(torch.equal(getattr(full, k), getattr(again, k)) for k in KINDS)
        r["launches_sweeps_per_read_1"] = again.sweeps
        runs = [("degree", {}), ("core", {}), ("core_bisect", {"hv_form": "bisect"}), ("component", {}),
                ("triangles", {})]
        for label, kw in runs:
            kind = label.split("_")[0]

            def call():
                return node_structure(g, kinds=(kind,), sweeps_per_read=SWEEPS_PER_READ, **kw)
            call()
            torch.cuda.synchronize()
            wall, kern, per_entry, launches = [], [], {}, None
            for _ in range(REPS):
                t0 = time.perf_counter()
                ns = call()
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
                launches = ns.sweeps.get(kind)
            for _ in range(REPS):
                rec = EventPairs(torch)
                with _lib.recording(rec):
                    call()
                per_entry = rec.per_entry()
                kern.append(sum(per_entry.values()))
            r[label] = {"call_ms": spread(wall), "kernel_ms": spread(kern), "kernel_ms_by_entry_last_run": per_entry,
                        "launches": launches, "calls_in_last_run": len(rec.pairs)}
            if label == "core_bisect":
                r[label]["equals_default"] = bool(torch.equal(ns.core, full.core))
            print(name, label, json.dumps(r[label]), flush=True)
        lens = g.rowptr[1:] - g.rowptr[:-1]
        r["rows_over_LPF_CORE_LONG_ROW"] = int((lens > _lib.CONST["LPF_CORE_LONG_ROW"]).sum())
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
