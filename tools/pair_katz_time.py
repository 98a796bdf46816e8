"""Device time of lpformer_amd.pair_walks / pair_katz on the collab-like bench graph: 32,768 held-out positives, 32,768
uniform random pairs and a HeaRT-shaped batch (64 positives, each against K negatives per side that keep one of its
endpoints: [P, 2 K, 2] pairs, every endpoint repeated K times), max_len 3 and 4, with and without ignore_direct, a
sweep of the number of workgroups (what the default workspace_mb would be chosen from), and the same pairs through scipy
A @ A row products on 16 host processes -- the only baseline there is.  The scipy counts are also compared with the
device's.  Writes one JSON document.
    LPF_CFG=collab LPF_P=32768 LPF_REPS=5 LPF_SCIPY_PAIRS=8192 LPF_OUT=profiles/pair_katz_timing.json \
        python tools/pair_katz_time.py"""
import json, multiprocessing, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

P = int(os.environ.get("LPF_P", "32768"))
REPS = int(os.environ.get("LPF_REPS", "5"))
SCIPY_PAIRS = int(os.environ.get("LPF_SCIPY_PAIRS", "8192"))      # scipy takes the first this many pairs of each set
PROCS = int(os.environ.get("LPF_PROCS", "16"))
GROUPS = [int(v) for v in os.environ.get("LPF_GROUPS", "64 128 256 512 1024 2048").split()]
HEART_POS = int(os.environ.get("LPF_HEART_POS", "64"))
HEART_K = int(os.environ.get("LPF_HEART_K", "250"))
OUT = os.environ.get("LPF_OUT", "profiles/pair_katz_timing.json")
_A = None


def _init(indptr, indices, n):
    import scipy.sparse as sp
    global _A
    _A = sp.csr_matrix((np.ones(indices.size, np.float64), indices, indptr), shape=(n, n))


def _rows(job):
    """W_1 .. W_4 of one slice of pairs: the rows a and b of A2 = A @ A as row products."""
    a, b = job
    Aa, Ab = _A[a], _A[b]
    A2a, A2b = Aa @ _A, Ab @ _A
    w1 = np.asarray(_A[a, b]).ravel()
    w2 = np.asarray(A2a[np.arange(a.size), b]).ravel()
    w3 = np.asarray(A2a.multiply(Ab).sum(axis=1)).ravel()
    w4 = np.asarray(A2a.multiply(A2b).sum(axis=1)).ravel()
    return np.stack([w1, w2, w3, w4], axis=1).astype(np.int64)


def scipy_walks(pool, pairs, per_job=64):
    """(int64 [P, 4], seconds): one job per ``per_job`` pairs."""
    t0 = time.perf_counter()
    jobs = [(pairs[0, lo:lo + per_job], pairs[1, lo:lo + per_job]) for lo in range(0, pairs.shape[1], per_job)]
    parts = []
    for k, part in enumerate(pool.imap(_rows, jobs)):              # in order; a progress line every 32 jobs
        parts.append(part)
        if (k + 1) % 32 == 0:
            print(f"  scipy {k + 1}/{len(jobs)} jobs {time.perf_counter() - t0:.0f} s", file=sys.stderr, flush=True)
    return np.concatenate(parts), time.perf_counter() - t0


def main():
    import torch
    from lpformer_amd import data as D, graph
    from lpformer_amd.katz import WORKSPACE_MB, default_groups, pair_katz, pair_walks

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
    pos = und[:, held[:HEART_POS]]
    neg = rng.integers(0, n, (HEART_POS, 2 * HEART_K))
    heart = np.concatenate([np.stack([np.repeat(pos[0], HEART_K), neg[:, :HEART_K].ravel()]),
                            np.stack([neg[:, HEART_K:].ravel(), np.repeat(pos[1], HEART_K)])], axis=1)
    sets = {"held_out_positives": und[:, held], "uniform_random": rng.integers(0, n, (2, P)), "heart_shaped": heart}
    res = {"config": name, "n": n, "nnz": int(csr.nnz), "max_degree": int(deg.max()), "pairs": P, "reps": REPS,
           "heart_shape": [HEART_POS, 2 * HEART_K, 2]}

    # the host baseline first: nothing has touched the GPU yet, and the workers are fresh processes
    ref = {}
    with multiprocessing.get_context("spawn").Pool(PROCS, _init, (csr.rowptr, csr.col, n)) as pool:
        for key, pairs in sets.items():
            ref[key], sec = scipy_walks(pool, pairs[:, :SCIPY_PAIRS])
            res[key] = {"pairs": int(pairs.shape[1]),
                        "scipy": {"pairs": int(ref[key].shape[0]), "processes": PROCS, "seconds": sec,
                                  "seconds_per_32768_pairs": sec * 32768 / max(ref[key].shape[0], 1)}}
            print(f"{key}: scipy {ref[key].shape[0]} pairs on {PROCS} processes {sec:.1f} s", flush=True)

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
    # the caching allocator after the first call), the memset of the launched workgroups' state, the kernel, the
    # un-sorting copy and, for pair_katz, the fp64 arithmetic
    res["ms_covers"] = "whole call: torch orientation / sort / unit cut, workspace allocation, state memset, kernel, un-sort"
    res["default_workspace_mb"] = WORKSPACE_MB
    for key, pairs in sets.items():
        e = torch.from_numpy(pairs).to(dev)
        r = res[key]
        r["default_groups"] = default_groups(n, pairs.shape[1], WORKSPACE_MB)
        w = pair_walks(g, e, max_len=4)
        wh = w.cpu().numpy()
        k = ref[key].shape[0]
        r["matches_scipy"] = bool(np.array_equal(wh[:k], ref[key]))
        r["max_len_3_is_a_prefix"] = bool(torch.equal(pair_walks(g, e, max_len=3), w[:, :3]))
        r["largest_counts"] = [int(v) for v in wh.max(axis=0)]
        r["share_nonzero"] = [float(v) for v in (wh > 0).mean(axis=0)]
        r["ms_walks_max_len_3"] = ms(lambda: pair_walks(g, e, max_len=3))
        r["ms_walks_max_len_4"] = ms(lambda: pair_walks(g, e, max_len=4))
        r["ms_katz_max_len_3"] = ms(lambda: pair_katz(g, e, max_len=3))
        r["ms_walks_max_len_3_ignore_direct"] = ms(lambda: pair_walks(g, e, max_len=3, ignore_direct=True))
        r["groups"] = {}
        for grp in GROUPS:
            r["groups"][grp] = {"workspace_mb": (16 + grp * 8 * n) / 2 ** 20,
                                "ms_walks_max_len_3": ms(lambda: pair_walks(g, e, max_len=3, groups=grp)),
                                "ms_walks_max_len_4": ms(lambda: pair_walks(g, e, max_len=4, groups=grp))}
        print(key, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
