"""Time the ranking-metric kernels against the torch forms they replace, on one GPU:

    python tools/metrics_time.py [--rounds 7] [--out profiles/metrics_timing.json]

* rows:   ``link_metrics`` (lpf_rank_rows_f32) against ``ranking_metrics`` at the citation2 shape, P = 86,596, K = 1,000;
* shared: ``ranks`` (lpf_rank_shared_f32, sort included) against the reference formulation -- the [4096, M] comparison
  of ``get_ranking_list`` per 4,096-row chunk, as its ``test()`` does -- at the collab valid split, P = 60,084,
  M = 100,000; and a second call on the already sorted negatives;
* kernels: the bare C-ABI calls against their byte floors (rows: 4 P K bytes; shared: 4 (P + M) bytes plus the sort).

Every step runs in a child process of its own under a time limit; the first step that fails ends the run.  Inside a
step the two sides alternate in one process, each timed with HIP events around the call (host-side work and the
read-back of the metric included where the function returns Python numbers), and the median of the rounds is kept.
Peak memory is torch's allocator peak over one call, above what the inputs hold."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEPS = {"rows": 240, "shared": 240, "kernels": 240}   # time limit of each step, seconds
HBM_GBPS = 8000.0                                      # MI355X peak HBM rate (for the floor fractions)


def _timed(fn, dev):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _peak(fn, dev):
    import torch
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    fn()
    torch.cuda.synchronize(dev)
    return int(torch.cuda.max_memory_allocated(dev) - base)


def _interleave(sides, rounds, dev):
    """sides: {name: fn}.  Two warm-up rounds, then `rounds` rounds with the sides alternating."""
    times = {k: [] for k in sides}
    for r in range(rounds + 2):
        for k, fn in sides.items():
            t = _timed(fn, dev)
            if r >= 2:
                times[k].append(t)
    out = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "rounds": len(v)}
           for k, v in times.items()}
    for k, fn in sides.items():
        out[k]["peak_bytes"] = _peak(fn, dev)
    return out


def step_rows(rounds):
    import torch
    from lpformer_amd import evaluate as E
    dev = torch.device("cuda:0")
    P, K = 86_596, 1000
    g = torch.Generator().manual_seed(0)
    pos, neg = torch.rand(P, generator=g).to(dev), torch.rand(P, K, generator=g).to(dev)
    want, got = E.ranking_metrics(pos, neg), E.link_metrics(pos, neg, k_list=(10, 50, 100), mrr=True, auc=False)
    assert all(abs(want[k] - got[k]) <= 2e-6 for k in want), (want, got)
    res = _interleave({"ranking_metrics": lambda: E.ranking_metrics(pos, neg),
                       "link_metrics": lambda: E.link_metrics(pos, neg, k_list=(10, 50, 100), mrr=True, auc=False),
                       "link_metrics_f32": lambda: E.link_metrics(pos, neg, k_list=(10, 50, 100), mrr=True, auc=False,
                                                                  accumulate=torch.float32),
                       "link_metrics_auc_ap": lambda: E.link_metrics(pos, neg, k_list=(10, 50, 100))}, rounds, dev)
    return {"P": P, "K": K, **res}


def step_shared(rounds):
    import torch
    from lpformer_amd import evaluate as E
    dev = torch.device("cuda:0")
    P, M = 60_084, 100_000
    g = torch.Generator().manual_seed(1)
    pos, neg = torch.rand(P, generator=g).to(dev), torch.rand(M, generator=g).to(dev)

    def chunked():   # get_ranking_list on 4,096 positives at a time against all negatives
        out = []
        for lo in range(0, P, 4096):
            col = pos[lo:lo + 4096].view(-1, 1)
            rows = neg.view(1, -1)
            out.append(0.5 * ((rows >= col).sum(dim=1) + (rows > col).sum(dim=1)) + 1)
        return torch.cat(out)

    assert torch.equal(chunked().float(), E.ranks(pos, neg))
    sn = E.sort_negatives(neg)
    res = _interleave({"reference_chunked": chunked, "ranks": lambda: E.ranks(pos, neg),
                       "ranks_presorted": lambda: E.ranks(pos, sn),
                       "link_metrics": lambda: E.link_metrics(pos, neg)}, rounds, dev)
    return {"P": P, "M": M, **res}


def step_kernels(rounds):
    import torch
    from lpformer_amd import _lib
    from lpformer_amd import evaluate as E
    dev = torch.device("cuda:0")
    out = {}
    g = torch.Generator().manual_seed(2)
    for P, K in ((86_596, 1000), (100_000, 100), (8192, 16384)):
        pos, neg = torch.rand(P, generator=g).to(dev), torch.rand(P, K, generator=g).to(dev)
        r = _interleave({"k": lambda: E._counts_rows(pos, neg)}, rounds, dev)["k"]
        floor_ms = 4.0 * P * K / (HBM_GBPS * 1e9) * 1e3
        out[f"rows_P{P}_K{K}"] = {**r, "bytes": 4 * P * K, "floor_ms": floor_ms, "gbps": 4e-6 * P * K / r["median_ms"],
                                  "fraction_of_floor": floor_ms / r["median_ms"]}
    for P, M in ((60_084, 100_000), (1_000_000, 10_000_000)):
        pos, neg = torch.rand(P, generator=g).to(dev), torch.rand(M, generator=g).to(dev)
        keys = torch.empty(M, dtype=torch.int32, device=dev)
        sn = E.SortedNegatives(keys, M)
        r = _interleave({"sort_and_rank": lambda: E._shared_call(pos, neg, keys, M),
                         "sort_only": lambda: E._shared_call(pos[:0], neg, keys, M),
                         "rank_only": lambda: E._counts_shared(pos, sn),
                         "torch_sort": lambda: torch.sort(neg)}, rounds, dev)
        # the searches read pos and write ge, gt (12 P bytes) over a sorted array that stays in cache; the sort reads
        # and writes the keys once per radix pass on top of the 4 (P + M) input bytes
        floor_ms = 4.0 * (P + M) / (HBM_GBPS * 1e9) * 1e3
        out[f"shared_P{P}_M{M}"] = {**r, "input_bytes": 4 * (P + M), "floor_ms_inputs_only": floor_ms,
                                    "workspace_bytes": int(_lib.hip().lpf_rank_shared_workspace_bytes(P, M)),
                                    "rank_only_fraction_of_floor": (12.0 * P / (HBM_GBPS * 1e9) * 1e3) /
                                    r["rank_only"]["median_ms"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_timing.json"))
    ap.add_argument("--step", choices=sorted(STEPS))
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("at least 5 rounds")
    if args.step:     # child: one step, its result as one JSON line
        print("RESULT " + json.dumps({"rows": step_rows, "shared": step_shared, "kernels": step_kernels}[args.step](args.rounds)))
        return
    import torch
    result = {"device": None, "rounds": args.rounds, "hbm_gbps_assumed": HBM_GBPS, "torch": torch.__version__}
    for step, limit in STEPS.items():
        try:
            cp = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--rounds", str(args.rounds)],
                                capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"step {step}: no result within {limit} s; stopping")
        if cp.returncode != 0:
            sys.stderr.write(cp.stdout[-2000:] + cp.stderr[-4000:])
            raise SystemExit(f"step {step} failed with exit status {cp.returncode}; stopping")
        line = [ln for ln in cp.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        result[step] = json.loads(line[len("RESULT "):])
        print(f"{step}: {json.dumps(result[step])}", flush=True)
    from lpformer_amd import _lib
    result["device"] = _lib.device_info()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
