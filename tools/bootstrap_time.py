"""Time of lpformer_amd.bootstrap on an MI355X next to what a user writes without the kernel.  For P positives
(LPF_PS, default 32,768 and 3,000,000), B = LPF_B = 1,000 replicates and the columns of ``bootstrap_metrics`` on one
shared negative set (Hits@20 / 50 / 100 and the AUC term as int64, the reciprocal rank as fp64):

    ms_bootstrap_metrics     the whole call, host clock around a synchronise: counts, columns, kernel, quantiles, read-back
    ms_bootstrap_sums        the whole ``bootstrap_sums`` call, device events: allocations and the launches
    ms_kernel                ``lpf_bootstrap_sums`` alone on preallocated outputs and workspace, device events
    ms_torch_randint_gather  the same sums by chunked ``torch.randint`` + gather + ``sum`` on the same device (other draws:
                             the statistics are the same, the numbers are not reproducible on a host)
    ms_numpy_twin            ``bootstrap_sums_reference`` on the host for LPF_TWIN_B replicates, scaled to B (stated so)

One warm-up call, then the median, minimum and maximum of LPF_REPS runs.  Before any timing the kernel's integer sums
are compared with the restatement's for a few replicates at the timed size.  Writes one JSON document.
    LPF_REPS=7 LPF_OUT=profiles/bootstrap_timing.json python tools/bootstrap_time.py"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

PS = [int(v) for v in os.environ.get("LPF_PS", "32768 3000000").split()]
B = int(os.environ.get("LPF_B", "1000"))
M = int(os.environ.get("LPF_M", "100000"))
REPS = int(os.environ.get("LPF_REPS", "7"))
TWIN_B = int(os.environ.get("LPF_TWIN_B", "4"))
CHUNK = int(os.environ.get("LPF_TORCH_CHUNK", str(1 << 24)))       # draws per torch.randint call of the baseline
OUT = os.environ.get("LPF_OUT", "profiles/bootstrap_timing.json")
KS = (20, 50, 100)


def main():
    import torch
    from lpformer_amd import _lib, bootstrap as bs, evaluate, ops

    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_properties(dev).gcnArchName, "torch": torch.__version__, "reps": REPS,
           "replicates": B, "shared_negatives": M, "columns": "int64: Hits@20, Hits@50, Hits@100, AUC term; fp64: 1 / rank",
           "spread": "every ms_* entry is [median, min, max] of reps runs after one warm-up call"}

    def spread(times):
        return [statistics.median(times), min(times), max(times)]

    def ms_events(fn, reps=REPS):
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        return spread(times)

    def ms_host(fn, reps=REPS):
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        return spread(times)

    gen = torch.Generator(device=dev).manual_seed(0)
    neg = torch.randn(M, device=dev, generator=gen)
    sn = evaluate.sort_negatives(neg)
    for p in PS:
        r = res[f"P_{p}"] = {"draws": p * B}
        pos = torch.randn(p, device=dev, generator=gen) + 2.0
        cols = bs._Columns(pos, sn, KS, True, True)
        icols = torch.stack(cols.icols, dim=1).contiguous()
        fcols = torch.stack(cols.fcols, dim=1).contiguous()
        ci, cf = icols.shape[1], fcols.shape[1]
        r["table_mb"] = (icols.numel() + fcols.numel()) * 8 / 2 ** 20

        # results first: the kernel's integers are the restatement's at this size
        isum, fsum = bs.bootstrap_sums(icols, fcols, TWIN_B, 1)
        t0 = time.perf_counter()
        wi, wf = bs.bootstrap_sums_reference(icols.cpu().numpy(), fcols.cpu().numpy(), TWIN_B, 1)
        twin_ms = 1e3 * (time.perf_counter() - t0)
        r["integer_sums_equal_restatement"] = bool((isum.cpu().numpy() == wi).all())
        r["float_sums_max_rel_diff"] = float(np.abs(fsum.cpu().numpy() - wf).max() / np.abs(wf).max())
        r["ms_numpy_twin"] = {"replicates_timed": TWIN_B, "ms": twin_ms, "ms_scaled_to_B": twin_ms * B / TWIN_B}

        r["ms_bootstrap_metrics"] = ms_host(lambda: bs.bootstrap_metrics(pos, sn, KS, replicates=B, seed=1))
        r["ms_bootstrap_sums"] = ms_events(lambda: bs.bootstrap_sums(icols, fcols, B, 1))

        hip = _lib.hip()
        need = int(hip.lpf_bootstrap_workspace_bytes(p, B, ci, cf, 0))
        ws = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
        oi = torch.empty(B, ci, dtype=torch.int64, device=dev)
        of = torch.empty(B, cf, dtype=torch.float64, device=dev)
        stream = ops.raw_stream(dev)

        def kernel(n_groups=0):
            _lib.check(hip.lpf_bootstrap_sums(p, B, 0, 1, icols.data_ptr(), ci, fcols.data_ptr(), cf, oi.data_ptr(),
                                              of.data_ptr(), n_groups, ws.data_ptr(), ws.numel(), stream))

        r["workspace_mb"] = need / 2 ** 20
        r["ms_kernel"] = ms_events(kernel)
        r["ms_kernel_by_n_groups"] = {str(g): ms_events(lambda g=g: kernel(g)) for g in (512, 1024, 2048, 4096)}
        r["draws_per_second_kernel"] = p * B / (r["ms_kernel"][0] * 1e-3)

        step = max(1, CHUNK // p)

        def torch_baseline():
            outs_i, outs_f = [], []
            for r0 in range(0, B, step):
                idx = torch.randint(0, p, (min(step, B - r0), p), device=dev)
                outs_i.append(icols[idx].sum(dim=1))
                outs_f.append(fcols[idx].sum(dim=1))
            return torch.cat(outs_i), torch.cat(outs_f)

        r["torch_chunk_replicates"] = step
        r["ms_torch_randint_gather"] = ms_events(torch_baseline, reps=max(3, REPS // 2))
        print(p, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
