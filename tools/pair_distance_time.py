"""Device time of lpformer_amd.pair_distance on the collab-like bench graph, 32,768 pairs: held-out positives and
uniform random pairs, max_dist=3 and no limit, the share of the pairs the front kernel settles, sweeps of
split_threshold and of the number of search workgroups (what LPF_BFS_SPLIT_DEFAULT and the default workspace_mb are
chosen from), and the same pairs through scipy's unweighted shortest_path(indices=...) on 16 host processes -- the only
baseline there is.  The scipy distances are also compared with the device's.  Writes one JSON document.
    LPF_CFG=collab LPF_P=32768 LPF_REPS=5 LPF_SCIPY_PAIRS=16384 LPF_OUT=profiles/pair_distance_timing.json \
        python tools/pair_distance_time.py"""
import json, multiprocessing, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

P = int(os.environ.get("LPF_P", "32768"))
REPS = int(os.environ.get("LPF_REPS", "5"))
SCIPY_PAIRS = int(os.environ.get("LPF_SCIPY_PAIRS", str(P)))      # scipy takes the first this many pairs of each set
PROCS = int(os.environ.get("LPF_PROCS", "16"))
SPLITS = [int(v) for v in os.environ.get("LPF_SPLITS", "0 8 32 128 512").split()]
GROUPS = [int(v) for v in os.environ.get("LPF_GROUPS", "64 128 256 512 1024 2048").split()]
OUT = os.environ.get("LPF_OUT", "profiles/pair_distance_timing.json")
_A = None


def _init(indptr, indices, n):
    import scipy.sparse as sp
    global _A
    _A = sp.csr_matrix((np.ones(indices.size, np.float32), indices, indptr), shape=(n, n))


def _rows(job):
    """Distances from one slice of the distinct sources to the targets asked of each (inf -> -1)."""
    from scipy.sparse.csgraph import shortest_path
    src, inv, b = job
    d = shortest_path(_A, method="D", unweighted=True, indices=src)[inv, b]
    return np.where(np.isfinite(d), d, -1).astype(np.int32)


def scipy_distance(pool, pairs, per_job=32):
    """(int32 [P], seconds): one job per ``per_job`` distinct first endpoints (a dense [per_job, n] block each)."""
    t0 = time.perf_counter()
    order = np.argsort(pairs[0], kind="stable")
    a, b = pairs[0][order], pairs[1][order]
    src, inv = np.unique(a, return_inverse=True)
    cut = np.searchsorted(inv, np.arange(0, src.size, per_job))
    jobs = [(src[k * per_job:(k + 1) * per_job], inv[lo:hi] - k * per_job, b[lo:hi])
            for k, (lo, hi) in enumerate(zip(cut, list(cut[1:]) + [a.size]))]
    parts = []
    for k, part in enumerate(pool.imap(_rows, jobs)):              # in order; a progress line every 128 jobs
        parts.append(part)
        if (k + 1) % 128 == 0:
            print(f"  scipy {k + 1}/{len(jobs)} jobs {time.perf_counter() - t0:.0f} s", file=sys.stderr, flush=True)
    out = np.empty(a.size, np.int32)
    out[order] = np.concatenate(parts)
    return out, time.perf_counter() - t0


def main():
    import torch
    from lpformer_amd import data as D, graph
    from lpformer_amd.distance import WORKSPACE_MB, default_groups, pair_distance

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

    # the host baseline first: nothing has touched the GPU yet, and the workers are fresh processes
    ref = {}
    with multiprocessing.get_context("spawn").Pool(PROCS, _init, (csr.rowptr, csr.col, n)) as pool:
        for key, pairs in sets.items():
            ref[key], sec = scipy_distance(pool, pairs[:, :SCIPY_PAIRS])
            res[key] = {"scipy": {"pairs": int(ref[key].size), "processes": PROCS, "seconds": sec,
                                  "seconds_per_32768_pairs": sec * 32768 / max(ref[key].size, 1)}}
            print(f"{key}: scipy {ref[key].size} pairs on {PROCS} processes {sec:.1f} s", flush=True)

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

    # every ms figure is one pair_distance() call: the workspace allocation (served by the caching allocator after the
    # first call), the memset of the launched workgroups' stamps, and both kernels
    res["ms_covers"] = "whole pair_distance() call: workspace allocation, stamp memset, front and search kernels"
    res["default_groups"] = default_groups(n, P, WORKSPACE_MB)
    res["default_workspace_mb"] = WORKSPACE_MB
    for key, pairs in sets.items():
        e = torch.from_numpy(pairs).to(dev)
        r = res[key]
        d = pair_distance(g, e)
        dh = d.cpu().numpy()
        r["matches_scipy"] = bool(np.array_equal(dh[:ref[key].size], ref[key]))
        r["max_dist_3_is_masked_exact"] = bool(torch.equal(pair_distance(g, e, max_dist=3),
                                                           torch.where((d <= 3), d, torch.full_like(d, -1))))
        vals, cnt = np.unique(dh, return_counts=True)
        r["distance_histogram"] = {int(v): int(c) for v, c in zip(vals, cnt)}
        r["ms_unlimited"] = ms(lambda: pair_distance(g, e))
        r["ms_max_dist_3"] = ms(lambda: pair_distance(g, e, max_dist=3))
        r["ms_unlimited_ignore_direct"] = ms(lambda: pair_distance(g, e, ignore_direct=True))
        # what the front kernel settles (unlimited search, no ignore_direct): a == b, an empty row, distance 1, and
        # distance 2 where the shorter row fits the threshold.  DERIVED on the host from the result and the degrees by
        # the kernel's own classification -- not read from the kernel's list counter, which the search counts down
        a, b = pairs
        short = np.minimum(deg[a], deg[b])
        r["split_threshold"] = {}
        for thr in SPLITS:
            front = (a == b) | (short == 0) | (dh == 1) | ((dh == 2) & (short <= thr))
            r["split_threshold"][thr] = {"front_share_derived": float(front.mean()),
                                         "ms_unlimited": ms(lambda: pair_distance(g, e, split_threshold=thr)),
                                         "ms_max_dist_3": ms(lambda: pair_distance(g, e, split_threshold=thr,
                                                                                   max_dist=3))}
        r["groups"] = {}
        for grp in GROUPS:
            r["groups"][grp] = {"workspace_mb": grp * (8 * n + 8) / 2 ** 20,
                                "ms_unlimited": ms(lambda: pair_distance(g, e, groups=grp)),
                                "ms_max_dist_3": ms(lambda: pair_distance(g, e, groups=grp, max_dist=3))}
        print(key, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
