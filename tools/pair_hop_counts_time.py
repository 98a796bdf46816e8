"""Device time of lpformer_amd.pair_hop_counts on the collab-like bench graph: 32,768 held-out positives and 32,768
uniform random pairs, hops 1 and 2, with and without ignore_direct, and a sweep of the number of workgroups (what the
default workspace_mb would be chosen from).  The first LPF_HOST_PAIRS pairs of each set also go through the numpy
restatement on the host (one process) -- the only baseline there is -- and are compared with the device's tables.
Writes one JSON document.
    LPF_CFG=collab LPF_P=32768 LPF_REPS=5 LPF_HOST_PAIRS=8192 LPF_OUT=profiles/pair_hop_counts_timing.json \
        python tools/pair_hop_counts_time.py"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

P = int(os.environ.get("LPF_P", "32768"))
REPS = int(os.environ.get("LPF_REPS", "5"))
HOST_PAIRS = int(os.environ.get("LPF_HOST_PAIRS", "8192"))       # the restatement takes the first this many pairs
GROUPS = [int(v) for v in os.environ.get("LPF_GROUPS", "256 1024 2048").split()]
OUT = os.environ.get("LPF_OUT", "profiles/pair_hop_counts_timing.json")


def main():
    import torch
    from lpformer_amd import data as D, graph
    from lpformer_amd.hops import WORKSPACE_MB, ball_jaccard, default_groups, hop_counts_reference, pair_hop_counts

    name = os.environ.get("LPF_CFG", "collab")
    cfg = D.CONFIGS[name]
    n = cfg["n"]
    ei, _ = D.chung_lu_graph(n, cfg["edges"], gamma=cfg["gamma"], seed=0, max_weight=cfg["max_weight"])
    ei = np.asarray(ei, np.int64)
    und = ei[:, ei[0] < ei[1]]
    rng = np.random.default_rng(2)
    held = rng.choice(und.shape[1], P, replace=False)
    keep = np.ones(und.shape[1], bool)
    keep[held] = False
    csr = graph.mask_csr(und[:, keep], n, symmetric=True)          # the graph without the held-out positives
    deg = np.diff(csr.rowptr)
    sets = {"held_out_positives": und[:, held], "uniform_random": rng.integers(0, n, (2, P))}
    res = {"config": name, "n": n, "nnz": int(csr.nnz), "max_degree": int(deg.max()), "pairs": P, "reps": REPS}

    # the host baseline first: nothing has touched the GPU yet
    ref = {}
    for key, pairs in sets.items():
        sub = torch.from_numpy(np.ascontiguousarray(pairs[:, :HOST_PAIRS]))
        res[key] = {"pairs": int(pairs.shape[1]), "numpy": {"pairs": int(sub.shape[1]), "processes": 1}}
        for k in (1, 2):
            t0 = time.perf_counter()
            ref[key, k] = hop_counts_reference(csr, sub, hops=k)
            sec = time.perf_counter() - t0
            res[key]["numpy"][f"seconds_hops_{k}"] = sec
            res[key]["numpy"][f"seconds_per_32768_pairs_hops_{k}"] = sec * 32768 / max(sub.shape[1], 1)
            print(f"{key}: numpy hops {k}, {sub.shape[1]} pairs {sec:.1f} s", flush=True)

    dev = torch.device("cuda:0")
    g = csr.to_device(dev)
    res["device"] = torch.cuda.get_device_properties(dev).gcnArchName
    res["torch"] = torch.__version__

    def ms(fn):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / REPS

    # every ms figure is one whole call: orientation, sort and unit cut in torch, the workspace allocation (served by
    # the caching allocator after the first call), the memset of the launched workgroups' state, the kernel, and the
    # un-sorting copy with the transposes
    res["ms_covers"] = ("whole call: torch orientation / sort / unit cut, workspace allocation, state memset, kernel, "
                        "un-sort and transpose")
    res["default_workspace_mb"] = WORKSPACE_MB
    for key, pairs in sets.items():
        e = torch.from_numpy(pairs).to(dev)
        r = res[key]
        r["default_groups"] = default_groups(n, pairs.shape[1], WORKSPACE_MB)
        for k in (1, 2):
            t = pair_hop_counts(g, e, hops=k)
            r[f"matches_numpy_hops_{k}"] = bool(torch.equal(t[:ref[key, k].shape[0]].cpu(), ref[key, k]))
            r[f"all_tables_sum_to_n_hops_{k}"] = bool((t.sum(dim=(1, 2)) == n).all())
            r[f"two_runs_equal_hops_{k}"] = bool(torch.equal(t, pair_hop_counts(g, e, hops=k)))
            r[f"mean_table_hops_{k}"] = t.double().mean(dim=0).cpu().tolist()
            r[f"share_positive_hops_{k}"] = (t > 0).double().mean(dim=0).cpu().tolist()
            r[f"mean_ball_jaccard_hops_{k}"] = float(ball_jaccard(t).double().mean())
            r[f"ms_hops_{k}"] = ms(lambda: pair_hop_counts(g, e, hops=k))
            r[f"ms_hops_{k}_ignore_direct"] = ms(lambda: pair_hop_counts(g, e, hops=k, ignore_direct=True))
        r["groups"] = {}
        for grp in GROUPS:
            r["groups"][grp] = {"workspace_mb": (16 + grp * 8 * n) / 2 ** 20,
                                "ms_hops_1": ms(lambda: pair_hop_counts(g, e, hops=1, groups=grp)),
                                "ms_hops_2": ms(lambda: pair_hop_counts(g, e, hops=2, groups=grp))}
        print(key, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
