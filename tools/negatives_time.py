"""Device time of lpformer_amd.negative_pairs / negative_rows next to the draw they replace: on the collab-like and the
ddi-like graph, ``negative_pairs(unique=False, check=False)`` -- what ``UniformNegatives`` runs per training step -- and
``negative_pairs(unique=True)`` at 16,384 and 32,768 slots against ``torch.randint`` of the same shape (what the parent's
epoch spends), ``negative_rows`` for 8,192 sources x 500 targets, and the share of ``torch.randint`` training negatives
that are edges (or self pairs) on each graph.  Whole calls, device events, one warm-up call, the median of LPF_REPS.
Writes one JSON document.
    LPF_CFGS="collab ddi" LPF_REPS=9 LPF_OUT=profiles/negatives_timing.json python tools/negatives_time.py"""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

CFGS = os.environ.get("LPF_CFGS", "collab ddi").split()
REPS = int(os.environ.get("LPF_REPS", "9"))
SLOTS = [int(v) for v in os.environ.get("LPF_SLOTS", "16384 32768").split()]
ROWS = int(os.environ.get("LPF_ROWS", "8192"))
ROW_K = int(os.environ.get("LPF_ROW_K", "500"))
SHARE_DRAWS = int(os.environ.get("LPF_SHARE_DRAWS", "1048576"))
OUT = os.environ.get("LPF_OUT", "profiles/negatives_timing.json")


def main():
    import torch
    from lpformer_amd import data as D, graph
    from lpformer_amd.negatives import negative_pairs, negative_rows

    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_properties(dev).gcnArchName, "torch": torch.__version__, "reps": REPS,
           "ms_covers": "whole call, median of reps: allocations, counter memset, kernels and, for unique=True, the "
                        "sort-and-compare rounds in torch; check=False, nothing read back"}

    def ms(fn):
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        return statistics.median(times)

    for name in CFGS:
        cfg = D.CONFIGS[name]
        n = cfg["n"]
        ei, _ = D.chung_lu_graph(n, cfg["edges"], gamma=cfg["gamma"], seed=0)
        g = graph.mask_csr(np.asarray(ei, np.int64), n, symmetric=True).to_device(dev)
        r = res[name] = {"n": n, "nnz": int(g.nnz), "density": g.nnz / (n * (n - 1.0)),
                         "max_degree": int((g.rowptr[1:] - g.rowptr[:-1]).max())}
        # how many of the parent's training negatives are no negatives
        gen = torch.Generator(device=dev).manual_seed(0)
        draw = torch.randint(0, n, (2, SHARE_DRAWS), device=dev, generator=gen)
        keys = torch.repeat_interleave(torch.arange(n, device=dev), g.rowptr[1:] - g.rowptr[:-1]) * n + g.col.long()
        q = draw[0] * n + draw[1]
        hit = keys[torch.searchsorted(keys, q).clamp_(max=keys.numel() - 1)] == q
        r["randint_share_edges"] = float(hit.float().mean())
        r["randint_share_self_pairs"] = float((draw[0] == draw[1]).float().mean())
        r["randint_draws"] = SHARE_DRAWS
        for m in SLOTS:
            e = r[f"pairs_{m}"] = {}
            e["ms_torch_randint"] = ms(lambda: torch.randint(0, n, (2, m), device=dev))
            e["ms_negative_pairs_plain"] = ms(lambda: negative_pairs(g, m, seed=1, unique=False, check=False))
            e["ms_negative_pairs_unique_8_rounds"] = ms(lambda: negative_pairs(g, m, seed=1, check=False))
            e["ms_negative_pairs_unique_2_rounds"] = ms(lambda: negative_pairs(g, m, seed=1, rounds=2, check=False))
            out = negative_pairs(g, m, seed=1, check=False)
            e["unresolved_unique_8_rounds"] = int((out[0] < 0).sum())
            e["unresolved_unique_1_round"] = int((negative_pairs(g, m, seed=1, rounds=1, check=False)[0] < 0).sum())
        src = torch.randint(0, n, (ROWS,), device=dev, generator=gen)
        k = min(ROW_K, 1024)
        e = r[f"rows_{ROWS}x{k}"] = {}
        e["ms_negative_rows"] = ms(lambda: negative_rows(g, src, k, seed=1, check=False))
        e["ms_torch_randint"] = ms(lambda: torch.randint(0, n, (ROWS, k), device=dev))
        e["short_rows"] = int((negative_rows(g, src, k, seed=1, check=False)[:, -1] < 0).sum())
        print(name, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
