#!/usr/bin/env python3
"""Headline benchmark: candidate link-pairs scored per second on a synthetic ogbl-collab-shaped graph.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config collab] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A plain run does what the headline needs: set-up, warm-up (and the untimed probes that pick the launch path and the
attention form), ONE timed window of exactly K steps, the scores of its last step under DIR (``--dump-outputs``), the
JSON line.  ``--full`` adds everything else the benchmark measures: five windows (median), the encoder timed alone, the
bf16 mode, per-kernel timing and rooflines, the trained-weights leg and the CPU baseline.

``python bench.py --gpus N`` without torchrun's environment starts its own N ranks (child processes, one per GPU,
before this process touches a GPU) and rank 0 prints the one JSON line with ``n_gpus: N``.

One "step" = the pair stage of the scoring path over one batch of candidate pairs with the encoder output
resident in HBM (the reference's HeaRT / citation2 evaluation pattern, src/train/testing.py:96-121:
``propagate()`` once, then per batch ``elementwise_lin(h[a]*h[b])``, ``calc_pairwise``, ``score_func``):
endpoint gathers, q projection, PPR-thresholded node selection, PE + attention, count features, ``pairwise_lin``,
``elementwise_lin`` and the ``mlp_score`` head, scores landing in device memory.  The encoder (L x GEMM + CSR SpMM;
N > 1: replicated, row-sharded with an RCCL all-gather per layer, or one all-gather of [X | Z] after the last layer,
chosen by a measured cost model) is timed separately and reported as ``encoder_ms``; the
throughput including one encoder pass per batch (the reference's ``test_edge`` pattern) is ``value_incl_encoder``.

Data are synthetic (no datasets offline): Chung-Lu power-law graph with ogbl-collab's node/edge counts and integer
edge weights, N(0,1) features, PPR from the library's own push (alpha 0.15, eps 5e-5), random-init weights.
Pairs are half existing edges, half uniform random; several distinct batches are cycled.

Rank 0 prints ONE JSON line.  N > 1: weak scaling, every rank scores its own 32,768-pair batches, no collective
on the pair path; time = max over ranks, value = pairs of all ranks / time.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def _self_launch(n_gpus: int) -> int:
    """``python bench.py --gpus N`` without torchrun: start N ranks as fresh child processes (this process has made no
    GPU call yet and makes none afterwards -- it only waits), one rank per GPU over RCCL, rendezvous on 127.0.0.1.
    Rank 0's stdout (the JSON line) passes through; returns the worst exit code."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(n_gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n_gpus), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), LPF_BENCH_CHILD="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    for pr in procs:
        rc = max(rc, abs(pr.wait()))
    return rc


if __name__ == "__main__" and "WORLD_SIZE" not in os.environ:
    _ap = argparse.ArgumentParser(add_help=False)
    _ap.add_argument("--gpus", type=int, default=1)
    _n = _ap.parse_known_args()[0].gpus
    if _n > 1:
        sys.exit(_self_launch(_n))

import lpformer_amd  # noqa: E402
from lpformer_amd import data as D  # noqa: E402
from lpformer_amd import dist as LD  # noqa: E402
from lpformer_amd.profile import KernelTimer  # noqa: E402

L2_PEAK_GBS = 34500.0     # MI355X_MICROARCH.md "L2 (per XCD)": 4 MiB per XCD, ~34.5 TB/s aggregate
PMC_SQ_FILE = "r06_pmc_sq_{config}.json"   # committed SQ counter pass of the dominant kernel (tools/pmc_kernel.sh)
PMC_FILE = "r06_pmc_traffic_{config}.json"  # committed rocprofv3 PMC passes (one file per config) `traffic` is read from
# timing span (KernelTimer) -> the HIP kernel that runs under it (what `roofline.kernel` names)
KERNEL_NAMES = {"pair_attention_rows": "pair_rows_kernel", "pair_attention_fused": "pair_flip_kernel / pair_fused_kernel",
                "tail_chain": "tail_chain_kernel", "select_run": "select_run", "select_plan": "select3_plan_kernel",
                "dense_chain_mlp_hidden": "dense_chain_kernel (+ q gather)", "pair_gather_q": "pair_gather_kernel",
                "pair_attention_merge": "pair_merge_kernel", "select_regions": "s4_regions_kernel"}
HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
F32_MFMA_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 = fp32 vector rate


def build_problem(cfg, rank, world, threads, ppr_device=None, barrier=None):
    """Synthetic graph, features and PPR matrix (untimed set-up).  With more than one rank only rank 0 generates the
    graph and runs the PPR push; the others load what it wrote to a memory-backed cache (/dev/shm, removed again by
    rank 0 once every rank has read it) -- the set-up is identical on every rank by construction, there is no point in
    eight processes recomputing it on eight GPUs at once."""
    from lpformer_amd import graph as G
    n = cfg["n"]
    cache = None
    if world > 1:
        base = "/dev/shm" if os.path.isdir("/dev/shm") else None
        import tempfile
        cache = os.path.join(base or tempfile.gettempdir(),
                             f"lpf_bench_setup_{os.environ.get('MASTER_PORT', '0')}_{os.getuid()}.npz")
    t0 = time.time()
    if rank == 0 or cache is None:
        ei, w = D.chung_lu_graph(n, cfg["edges"], gamma=cfg["gamma"], seed=0, max_weight=cfg["max_weight"])
        x = np.random.default_rng(1).standard_normal((n, cfg["f_in"])).astype(np.float32)
        t1 = time.time()
        data = D.build_data(ei, x, n, edge_weight=w, eps=cfg["eps"], ppr_threads=threads, ppr_device=ppr_device)
        t2 = time.time()
        if cache is not None:
            ppr = data["ppr"]
            tmp = cache + ".tmp.npz"
            np.savez(tmp, ei=ei, w=np.zeros(0, np.float32) if w is None else w, x=x, ppr_rowptr=ppr.rowptr,
                     ppr_col=ppr.col, ppr_val=ppr.val)
            os.replace(tmp, cache)
    if cache is not None:
        barrier()                       # the cache is complete
        if rank != 0:
            z = np.load(cache)
            ei, w, x = z["ei"], (z["w"] if z["w"].size else None), z["x"]
            t1 = time.time()
            ppr = G.CSR(z["ppr_rowptr"], z["ppr_col"], z["ppr_val"], n)
            data = D.build_data(ei, x, n, edge_weight=w, eps=cfg["eps"], ppr=ppr)
            t2 = time.time()
        barrier()                       # every rank has read it
        if rank == 0:
            try:
                os.remove(cache)
            except OSError:
                pass
    return ei, w, x, data, {"graph_s": t1 - t0, "ppr_s": t2 - t1}


def relabel_cache_resident(rooflines):
    """A byte-priced entry whose measured HBM traffic is less than half its algorithmic bytes runs out of the caches
    (ddi-like / cora-like tables of a few MB: SURVEY 8(d)'s bytes never reach HBM): priced against the guide's L2 figure
    instead, the HBM fraction kept beside it -- a `frac` above 1 is not a roofline fraction."""
    for r in rooflines.values():
        if r.get("bound") == "hbm" and r.get("traffic") and r.get("algorithmic") and r["algorithmic"] > 2.0 * r["traffic"]:
            r["frac_of_hbm_peak"] = r["frac"]
            r["bound"], r["peak"] = "l2", L2_PEAK_GBS
            r["frac"] = round(r["achieved"] / L2_PEAK_GBS, 4)
            r["note"] = ("tables cache-resident: counter traffic is under half the algorithmic bytes, priced against the "
                         "aggregate L2 rate (MI355X_MICROARCH.md, 34.5 TB/s)")


def pair_stats(data, batch):
    """Per-batch structural sizes (reported beside the roofline: what a both-rows walk would have touched)."""
    adj, ppr = data["adj_mask"], data["ppr"]
    a, b = batch[0], batch[1]
    deg = np.diff(adj.rowptr)
    plen = np.diff(ppr.rowptr)
    return {"sum_deg": int(deg[a].sum() + deg[b].sum()), "sum_ppr_len": int(plen[a].sum() + plen[b].sum())}


def slot_count(model, batch_t):
    """Candidate slots of one batch as the plan kernel lays them out (a-side walk | b-side walk | >1-hop walk, at
    least 16 per pair)."""
    if model._uses_select4() and model._uses_rows():   # the one-launch form: ctl[1] = slots, block by block rounded to 8
        ws = model._select4_device(batch_t, False)     # (ctl[0] is 8 x the fullest allocation region: an upper bound)
        return int(ws.ctl[1].item())
    ws = model._select_device(batch_t, False, None)
    return int(ws.ctl[1 if hasattr(ws, "blk_types") else 0].item())   # (behind lpf_select4: word 1, as above)


def run_cpu_workers(sample, x_node, mask, ppr, P, cfg, n_proc, chunk):
    """Scores ``sample`` ([2, n] pairs) with the numpy oracle on ``n_proc`` worker processes (oracle/bench_worker.py:
    numpy + oracle only), inputs shared through memory-mapped files.  Returns (logits, seconds from the common start
    signal to the last worker's end)."""
    import pickle
    import shutil
    import subprocess
    import tempfile
    n_take = sample.shape[1]
    spans = [(i, min(i + chunk, n_take)) for i in range(0, n_take, chunk)]
    arrays = {"sample": sample, "x_node": x_node, "mask_rowptr": mask.rowptr, "mask_col": mask.col.astype(np.int64),
              "ppr_rowptr": ppr.rowptr, "ppr_col": ppr.col.astype(np.int64), "ppr_val": ppr.val}
    need = sum(np.asarray(v).nbytes for v in arrays.values()) + (64 << 20)
    d = None
    for base in ("/dev/shm", None):   # memory-backed files when they fit there, the default temporary directory otherwise
        try:
            if base is not None and (not os.path.isdir(base) or shutil.disk_usage(base).free < need):
                continue
            d = tempfile.mkdtemp(prefix="lpf_bench_", dir=base)
            for k, v in arrays.items():
                np.save(os.path.join(d, k + ".npy"), np.ascontiguousarray(v))
            break
        except OSError:
            if d is not None:
                shutil.rmtree(d, ignore_errors=True)
            d = None
    if d is None:
        raise RuntimeError("cpu_baseline: no temporary directory could hold the shared inputs")
    procs = []
    try:
        with open(os.path.join(d, "small.pkl"), "wb") as f:
            pickle.dump({"P": P, "cfg": cfg, "spans": spans}, f)
        env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
        procs = [subprocess.Popen([sys.executable, "-m", "oracle.bench_worker", d, str(i), str(n_proc)], cwd=ROOT, env=env)
                 for i in range(n_proc)]
        t_dead = time.time() + 600
        while sum(os.path.exists(os.path.join(d, f"ready.{i}")) for i in range(n_proc)) < n_proc:
            if time.time() > t_dead or any(p.poll() not in (None, 0) for p in procs):
                raise RuntimeError("cpu_baseline: a worker did not come up")
            time.sleep(0.01)
        t_go = time.time()
        open(os.path.join(d, "go"), "w").close()
        for p in procs:
            if p.wait(timeout=1800) != 0:
                raise RuntimeError("cpu_baseline: a worker failed")
        ends = [float(open(os.path.join(d, f"done.{i}")).read().split()[1]) for i in range(n_proc)]
        logits = np.empty(n_take, np.float32)
        for i in range(n_proc):
            part, pos = np.load(os.path.join(d, f"logit.{i}.npy")), 0
            for lo, hi in spans[i::n_proc]:
                logits[lo:hi] = part[pos:pos + hi - lo]
                pos += hi - lo
        return logits, max(ends) - t_go
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        shutil.rmtree(d, ignore_errors=True)


def cpu_baseline(args, model, score, targs, data, batches_np, h, bs, dev):
    """The numpy oracle's pair stage on a bounded sample of the bench's own batches, on ALL host cores (one worker
    process per core), next to the GPU's logits for the same pairs."""
    n_proc = max(1, args.cpu_procs or (os.cpu_count() or 1))
    n_take = min(args.cpu_sample or 1024 * n_proc, bs * len(batches_np))
    sample = np.ascontiguousarray(np.concatenate(batches_np, axis=1)[:, :n_take])
    chunk = max(64, min(1024, n_take // (2 * n_proc) or 64))
    P = {f"model.{k}": v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    P.update({f"score.{k}": v.detach().cpu().numpy() for k, v in score.state_dict().items()})
    ref_logit, cpu_s = run_cpu_workers(sample, h.cpu().numpy(), data["adj_mask"], data["ppr"], P,
                                       dict(targs, pred_layers=2), n_proc, chunk)
    gl = []   # the GPU scores of the same pairs, checked against it while we are here
    for i in range(0, n_take, bs):
        for _attempt in range(3):
            out = model.score_pairs(torch.from_numpy(sample[:, i:i + bs]).to(dev), h, score, logits=True)
            if model.check_selection():
                break
        gl.append(out.cpu().numpy())
    gl = np.concatenate(gl)
    return {"value": round(n_take / cpu_s, 1), "unit": "pairs/s", "cores": n_proc, "kind": "port",
            "sample": f"first {n_take} pairs of the bench's batches (pair stage, encoder output resident) in chunks of "
                      f"{chunk} on {n_proc} worker processes (host has {os.cpu_count()} cores), one BLAS thread each; "
                      f"numpy restatement oracle/lpformer_oracle.py, {cpu_s:.2f} s from the common start signal to the "
                      "last worker's end (process start-up and page-ins excluded)",
            "max_abs_logit_diff_vs_gpu": float(np.abs(gl - ref_logit).max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="collab", choices=sorted(D.CONFIGS))
    ap.add_argument("--batches", type=int, default=32,
                    help="distinct candidate batches cycled through (resident in HBM before the timed region; a captured "
                         "graph copies the ids of the step's batch into its static input).  0 = one per stream: a "
                         "stream then always scores the same resident batch, read in place (round 3's default)")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beyond the headline (the legs switched by --weights, "
                         "--no-cpu-baseline, --no-kernel-timing and --no-bf16, the encoder alone, rooflines) and time "
                         "--repeats windows")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the scores of the last timed step (rank 0: the [pairs_per_step] probabilities the "
                         "timed path returns) as DIR/scores.npy, float32")
    ap.add_argument("--weights", default="both", choices=("random", "both"),
                    help="(--full) both: after the headline (random-init weights, as the bench contract prescribes) "
                         "the model is trained for --train-steps steps of the repo's own training step on the synthetic "
                         "graph and the same timed window is run again (extra key `trained_weights`: flips per entry, the "
                         "attention kernel `auto` then picks, ms per step)")
    ap.add_argument("--train-steps", type=int, default=150)
    ap.add_argument("--train-lr", type=float, default=1e-3)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-sample", type=int, default=0,
                    help="pairs timed on the CPU oracle, taken from the bench's own batches (0 = 1,024 per worker process, "
                         "at most all of them: about 1 s of work per core)")
    ap.add_argument("--cpu-procs", type=int, default=0, help="worker processes of the CPU baseline (0 = all host cores)")
    ap.add_argument("--no-kernel-timing", action="store_true")
    ap.add_argument("--no-bf16", action="store_true", help="skip the extra bf16 throughput-mode measurement")
    ap.add_argument("--ppr", default="gpu", choices=("gpu", "host"),
                    help="PPR producer for the (untimed) setup: lpf_ppr_push_f64 on the GPU or the OpenMP host push")
    ap.add_argument("--spinup", type=float, default=1.0,
                    help="seconds of untimed steps after the W warm-up steps, so that the device holds its clocks")
    ap.add_argument("--side-stream", default="auto", choices=("auto", "on", "off"),
                    help="the elementwise / q branches of a step on a side stream of their own (model.use_side_stream). "
                         "auto = off when the steps already rotate over several streams: the other streams' kernels "
                         "fill the machine, and the fork / join events of a side stream cost more than the overlap "
                         "inside one step gives (collab-like, 6 streams: 0.199 ms/step with, 0.192 without)")
    ap.add_argument("--no-side-stream", action="store_true", help="= --side-stream off")
    ap.add_argument("--repeats", type=int, default=None,
                    help="timed windows of K steps each (default 1, with --full 5); `value` / `ms_per_step` are the "
                         "MEDIAN window, min/median/max of all are reported")
    ap.add_argument("--encoder", default="auto", choices=("auto", "replicated", "sharded", "gather_once"),
                    help="N > 1: every rank runs the whole encoder / rows sharded with an all-gather per layer / the last "
                         "layer and the per-node attention projections sharded with ONE all-gather of [X | Z]; "
                         "auto = the cheapest by lpformer_amd.dist.encoder_plan (measured encoder, last-layer and "
                         "projection times, measured all-gather rate)")
    ap.add_argument("--attention", default="auto", choices=("auto", "flip", "mfma"),
                    help="fp32 one-pass attention kernel: activation-pattern evaluation of the PE key projection "
                         "(pair_flip.hip, gather-bound) or the D x D product on the fp32 matrix cores (pair_fused.hip)")
    ap.add_argument("--rows", default="auto", choices=("auto", "on", "off"),
                    help="activation-pattern attention pair-major with finished rows (pair_rows.hip + the rows mode of the "
                         "dense tail) or unit-major with records merged by the tail (pair_flip.hip); auto: whichever is "
                         "faster in an untimed probe of the pipelined steps (both times are reported in config)")
    ap.add_argument("--launch", default="auto", choices=("auto", "graph", "plan", "eager"),
                    help="auto: whichever of the three is fastest in an untimed probe before the windows (the choice and "
                         "all probe times are reported in config); eager: LinkTransformer.score_pairs per step (~0.15 ms "
                         "of host time per step between its launches: the loop is bound by the host whenever the device "
                         "needs less); graph: every stream replays ONE captured HIP graph of the step "
                         "(lpformer_amd.GraphedScorer; 0.04 ms of host time, but replayed graphs overlap less between "
                         "streams); plan: every stream replays the RECORDED C-ABI launches of the step, one plain launch "
                         "after the other (lpformer_amd.PlannedScorer; 0.04 ms of host time, the overlap of eager "
                         "launches).  The same launches and bitwise the same scores in all three")
    ap.add_argument("--select4-threads", type=int, default=0,
                    help="(tuning) launch shape of lpf_select4: workgroup size + 4096 * (blocks per workgroup - 1); 0 = default")
    ap.add_argument("--select-grid", type=int, default=0,
                    help="(tuning) workgroups of the selection's run kernel; 0 = as many as are resident at once")
    ap.add_argument("--streams", type=int, default=4,
                    help="HIP streams the timed steps rotate over (consecutive batches overlap; 1 = strictly serial).  "
                         "Round 5, collab-like, same lease, ms/step at 20 / 40 / 120 steps per window: 4 streams 0.139 / "
                         "0.1355 / 0.135, 8 streams 0.142 / 0.136 / 0.135 (every kernel fills the chip by itself now: more "
                         "streams only lengthen the fill and drain of a window); 2: 0.144, 16: 0.145 at 20 steps")
    args = ap.parse_args()
    if args.repeats is None:
        args.repeats = 5 if args.full else 1
    if not args.full:   # a plain run: the headline window only, none of the extra legs
        args.weights, args.no_cpu_baseline, args.no_kernel_timing, args.no_bf16 = "random", True, True, True

    rank, world, local = LD.init_from_env()
    if world != args.gpus and rank == 0:
        print(f"[bench] WORLD_SIZE={world} but --gpus {args.gpus}; using WORLD_SIZE", file=sys.stderr)
    assert torch.cuda.is_available(), "bench.py needs an MI355X"
    local = int(os.environ.get("LPF_LOCAL_DEVICE", local))  # (functional multi-rank runs on a one-GPU box)
    dev = torch.device(f"cuda:{local}")
    torch.cuda.set_device(dev)
    cfg = D.CONFIGS[args.config]
    n, d, bs = cfg["n"], cfg["dim"], cfg["batch"]
    host_threads = max(1, (os.cpu_count() or 8) // world)

    def barrier():
        if world > 1:
            torch.distributed.barrier()

    ei, w, x, data, setup = build_problem(cfg, rank, world, host_threads, dev if args.ppr == "gpu" else None, barrier)
    targs = D.train_args_for(cfg)
    torch.manual_seed(0)
    model = lpformer_amd.LinkTransformer(targs, data, device=dev).to(dev).eval()
    score = lpformer_amd.mlp_score(model.out_dim, model.out_dim, 1, 2).to(dev).eval()
    side = "off" if args.no_side_stream else args.side_stream
    model.use_side_stream = side == "on" or (side == "auto" and args.streams <= 1)
    model.attention_impl = args.attention
    model.select_grid = args.select_grid
    model.select4_threads = args.select4_threads
    if os.environ.get("LPF_SELECT_BLOCKS"):                      # A/B aid: "0" = lpf_select3_plan / _run on every path
        model.select_blocks = os.environ["LPF_SELECT_BLOCKS"] != "0"
    enc_plan = None
    if world > 1:
        # encoder layout: measure the whole encoder on one GPU (replicated mode) and the all-gather of an [N, D] fp32
        # matrix on this process group, then take the cheaper layout (or the one asked for)
        model.set_row_shard(rank, world, "replicated")
        for _ in range(2):
            model.propagate()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            model.propagate()
        torch.cuda.synchronize()
        enc1 = LD.max_over_ranks((time.perf_counter() - t0) * 1e3 / 3, dev)
        # the parts the single-gather layout shards: the last layer's aggregation and the two per-node projections
        KernelTimer.reset()
        KernelTimer.enabled = True
        hh = model.propagate()
        model._node_keys(hh, model._fold())
        model._node_y(hh, model._fold())
        kt0 = KernelTimer.summary()
        KernelTimer.enabled = False
        # (a fused layer -- one launch, csrc/gcn_fused.hip -- is row-sharded whole)
        last_key = "gcn_layer_fused" if "gcn_layer_fused" in kt0 else "spmm_csr"
        last_agg = LD.max_over_ranks(kt0[last_key][2] if last_key in kt0 else enc1 / cfg["gnn_layers"], dev)
        # Z is row-shardable in gather_once; the query table Y is computed in full by every rank in every layout
        keys_ms = LD.max_over_ranks(kt0["gemm_node_keys"][1] if "gemm_node_keys" in kt0 else 0.0, dev)
        y_ms = LD.max_over_ranks(kt0["gemm_node_query"][1] if "gemm_node_query" in kt0 else 0.0, dev)
        del hh
        ag = LD.measure_allgather_gbps(n, d, dev)
        enc_plan = LD.encoder_plan(enc1, n, d, cfg["gnn_layers"], world, ag, last_agg_ms=last_agg,
                                   node_keys_ms=keys_ms, replicated_ms=y_ms)
        enc_plan.update(allgather_gbps=round(ag, 1), last_agg_ms=round(last_agg, 4), node_keys_ms=round(keys_ms, 4),
                        node_query_ms=round(y_ms, 4))
        enc_plan["chosen"] = enc_plan["mode"] if args.encoder == "auto" else args.encoder
        model.set_row_shard(rank, world, enc_plan["chosen"])

    # candidate batches resident in HBM before the timed region; distinct per rank
    if args.batches <= 0:
        args.batches = max(1, args.streams)
    batches_np = [D.sample_pairs(ei, n, bs, seed=1000 * rank + i) for i in range(args.batches)]
    batches = [torch.from_numpy(b).to(dev) for b in batches_np]

    # ---- the selection's walk indexes (built once per (adjacency, PPR matrix, thresholds) on the device): timed and
    #      sized here, because the selection's speed is bought with them
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    wi = model._walk_index(model._data_obj("mask", False), model._data_obj("ppr", False))
    torch.cuda.synchronize()
    setup["index_s"] = time.perf_counter() - t0
    idx_tensors = [wi.rec, wi.adj_cv, wi.a1_cv, wi.px_cv, wi.t0_cv, wi.u.cv, wi.u.rowptr, wi.u.len] + \
        [getattr(wi, k) for k in ("mini",) if getattr(wi, k, None) is not None]
    index_bytes = int(sum(t.numel() * t.element_size() for t in idx_tensors if t is not None))
    del wi, idx_tensors

    # ---- encoder output (resident for the pair stage; the encoder itself is timed after the pair stage, warm)
    for _ in range(2):
        h = model.propagate()
    torch.cuda.synchronize()

    def step(i):  # = score(cat(elementwise_lin(x_a * x_b), calc_pairwise(...))) with the boundary Linears folded
        return model.score_pairs(batches[i % len(batches)], h, score)

    # consecutive steps rotate over `--streams` HIP streams: the selection kernels of one batch (latency / issue
    # bound) run under the MFMA kernels of the previous one.  Every step still does all of its work.
    lanes = model.lanes(max(1, args.streams))

    def record_plans():
        """One recorded step per stream (None when the step cannot be recorded on some rank: all ranks agree)."""
        try:
            if os.environ.get("LPF_BENCH_FAIL_CAPTURE_RANK") == str(rank):   # (test switch: tests/test_gpu_dist.py)
                raise RuntimeError("capture failure injected on this rank")
            got = [lpformer_amd.PlannedScorer(model, score, h, batches[k % len(batches)], adopt_input=True)
                   for k in range(len(lanes))]
        except RuntimeError as exc:   # (a step that does work outside the C-ABI launches cannot be recorded)
            if args.launch == "plan":
                raise
            print(f"[bench] recording the step failed ({exc})", file=sys.stderr)
            got = None
            torch.cuda.synchronize()
        return None if LD.max_over_ranks(0.0 if got is not None else 1.0, dev) > 0.0 else got

    # ---- which of the two forms of the activation-pattern attention?  (untimed probe of the pipelined steps; through
    #      recorded plans when the timed windows may use them -- eager launches are bound by the host at D <= 128 and
    #      would time Python, not the kernels)
    rows_probe = None
    planned_by_form = {}
    # the probes time windows as long as the timed one, up to a bound: what a run costs besides its K timed steps must
    # not grow with K
    probe_steps = min(args.steps, 500)
    if os.environ.get("LPF_SELECT4_REGIONS"):                    # A/B aid: "0" = lpf_select3_plan / _run for the type-major consumers
        model.select4_regions = os.environ["LPF_SELECT4_REGIONS"] != "0"
    if os.environ.get("LPF_TAIL_SKIP_EMPTY"):                    # A/B aid: "0" = the plain rows tail
        model.tail_skip_empty = os.environ["LPF_TAIL_SKIP_EMPTY"] != "0"
    if args.rows != "auto":
        model.attention_rows = args.rows == "on"
    elif model.attention_kernel() == "flip":
        rows_probe = {}
        t_spin = time.perf_counter()          # (a cold device ramps its clocks for ~0.5 s: not inside the comparison)
        while time.perf_counter() - t_spin < 0.6:
            for i in range(16):
                with torch.cuda.stream(lanes[i % len(lanes)]):
                    step(i)
            torch.cuda.synchronize()
        for mode in ("rows", "records"):
            model.attention_rows = mode == "rows"
            planned_by_form[mode] = record_plans() if args.launch in ("plan", "auto") else None
        for rnd in range(2):   # rows, records, rows, records: the smaller of a form's two times counts (whatever ran
            #                    first on a box that is still settling would otherwise lose)
            for mode in ("rows", "records"):
                model.attention_rows = mode == "rows"
                pl = planned_by_form[mode]

                def probe_step(i):
                    if pl is not None:
                        return pl[i % len(lanes)](batches[i % len(batches)], validate=False, ordered=False)
                    with torch.cuda.stream(lanes[i % len(lanes)]):
                        return step(i)
                for i in range(2 * len(lanes)):
                    probe_step(i)
                torch.cuda.synchronize()
                barrier()
                t0 = time.perf_counter()
                for i in range(max(probe_steps, 40)):
                    probe_step(i)
                torch.cuda.synchronize()
                barrier()
                t = LD.max_over_ranks(time.perf_counter() - t0, dev) * 1e3 / max(probe_steps, 40)
                rows_probe[mode] = min(t, rows_probe.get(mode, t))
        model.attention_rows = rows_probe["rows"] <= rows_probe["records"]
        rows_probe = {k: round(v, 4) for k, v in rows_probe.items()}

    scorers = planned = None
    if args.launch in ("plan", "auto"):
        planned = planned_by_form.get("rows" if model.attention_rows else "records") or record_plans()
        planned_by_form.clear()
    if args.launch in ("graph", "auto"):
        # one captured step per stream; a scorer owns its workspaces (sized from the batch it is captured with, twice
        # its entry counts) and re-captures by itself when the precision mode or a parameter changes
        KernelTimer.enabled = False
        try:
            # (a scorer whose stream always sees the same batch adopts it as its static input: no copy per replay)
            fixed = len(lanes) % len(batches) == 0
            if os.environ.get("LPF_BENCH_FAIL_CAPTURE_RANK") == str(rank):   # (test switch)
                raise RuntimeError("capture failure injected on this rank")
            scorers = [lpformer_amd.GraphedScorer(model, score, h, batches[k % len(batches)], adopt_input=fixed)
                       for k in range(len(lanes))]
        except RuntimeError as exc:   # a capture that fails leaves the eager path, which is the same work
            if args.launch == "graph":
                raise
            print(f"[bench] graph capture failed ({exc}); timing eager launches", file=sys.stderr)
            scorers = None
            torch.cuda.synchronize()
        # every rank must take the same path from here on (the probe below runs barriers and reductions): if the
        # capture failed on ANY rank, all of them time eager launches
        if LD.max_over_ranks(0.0 if scorers is not None else 1.0, dev) > 0.0:
            scorers = None
            if args.launch == "graph":
                args.launch = "eager"

    launch = args.launch if args.launch != "auto" else "eager"

    def step_on(i):
        # (validate=False: nothing changes a parameter inside a window; stale() is asked after it)
        if launch == "plan":   # the plan's launches go to its own stream; the ids have been resident since set-up
            return planned[i % len(lanes)](batches[i % len(batches)], validate=False, ordered=False)
        with torch.cuda.stream(lanes[i % len(lanes)]):
            if launch == "graph":
                return scorers[i % len(lanes)](batches[i % len(batches)], validate=False)
            return step(i)

    for i in range(max(args.warmup, len(lanes))):
        step_on(i)
    torch.cuda.synchronize()
    # device spin-up (untimed): a freshly started MI355X needs ~0.5 s of sustained work before it holds its clocks --
    # the first process on a cold box measures 55 M pairs/s in a 50 ms timed window and 82 M after this
    t_spin, n_spin = time.perf_counter(), 0
    while args.spinup > 0 and time.perf_counter() - t_spin < args.spinup:
        for i in range(16):
            step_on(i)
        torch.cuda.synchronize()
        n_spin += 16

    launch_probe = None
    if args.launch == "auto":
        # untimed probe: the same K steps through both launch paths; the timed windows use the faster one.  (Eager
        # costs ~0.15 ms of host time per step whatever the batch -- the D = 64 configs need less GPU time than that --
        # while at D = 128 the replayed graphs run a few per cent behind the eager launches.)
        probe = {}
        for mode in ("eager", "graph", "plan"):
            if (mode == "graph" and scorers is None) or (mode == "plan" and planned is None):
                continue
            launch = mode
            for i in range(2 * len(lanes)):
                step_on(i)
            torch.cuda.synchronize()
            barrier()
            t0 = time.perf_counter()
            for i in range(probe_steps):
                step_on(i)
            torch.cuda.synchronize()
            barrier()
            probe[mode] = LD.max_over_ranks(time.perf_counter() - t0, dev) * 1e3 / probe_steps
        launch = min(probe, key=probe.get)
        launch_probe = {k: round(v, 4) for k, v in probe.items()}


    # ---- timed region: windows of EXACTLY `steps` steps, nothing but the scoring path (no event recording); each
    #      window is bracketed by a barrier + device synchronisation on both sides, time = max over ranks.
    KernelTimer.enabled = False

    def window():
        # W untimed steps in front of EVERY window: between windows the host checks the previous one's scores and the
        # device idles; a 20-step window is 3.6 ms long and feels the clocks coming back up
        for i in range(args.warmup):
            step_on(i)
        barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            o = step_on(i)
        torch.cuda.synchronize()
        barrier()
        return LD.max_over_ranks(time.perf_counter() - t0, dev), o

    rep_s = []
    for _ in range(max(1, args.repeats)):
        el, out = window()
        rep_s.append(el)
        assert torch.isfinite(out).all()
    # the steps never read the selection status back (nothing does while they are queued): read it once per lane now --
    # a batch that had outgrown its workspace would have come back as NaN and must not count as scored
    if launch != "eager":
        used = scorers if launch == "graph" else planned
        assert not any(sc.stale() for sc in used), "a parameter changed inside the timed windows"
        overflows = sum(0 if sc.check() else 1 for sc in used)
    else:
        overflows = sum(0 if model.check_selection(lane) else 1 for lane in lanes)
    assert overflows == 0, "a timed step overflowed its selection workspace: the window is invalid"
    if args.dump_outputs and rank == 0:
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "scores.npy"), out.float().cpu().numpy())
    rep_ms = [e * 1e3 / args.steps for e in rep_s]
    elapsed = float(np.median(rep_s))   # `value`: the median window

    # ---- encoder, timed separately (same output: h stays valid); --full
    encoder_ms = node_keys_ms = encoder_bf16 = None
    if args.full:
        barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        enc_reps = 5
        for _ in range(enc_reps):
            h2 = model.propagate()
        torch.cuda.synchronize()
        barrier()
        encoder_ms = LD.max_over_ranks((time.perf_counter() - t0) * 1e3 / enc_reps, dev)
        # ... and with what every NEW encoder output costs on top: the two per-node projections Z | Y of the attention
        # (one [N, D] x [D, 2D] product, cached per encoder output; the gather_once layout computes them inside
        # propagate())
        barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(enc_reps):
            h2 = model.propagate()
            model._node_keys(h2, model._fold())
            if model.query_from == "table":
                model._node_y(h2, model._fold())
        torch.cuda.synchronize()
        barrier()
        node_keys_ms = max(0.0, LD.max_over_ranks((time.perf_counter() - t0) * 1e3 / enc_reps, dev) - encoder_ms)
        # the same with the gathered per-layer table stored in bf16 (lpf_gemm_f32_out_bf16 + lpf_spmm_csr_bf16)
        if not args.no_bf16:
            model.encoder_precision = "bf16"
            h16 = model.propagate()
            torch.cuda.synchronize()
            barrier()
            t0 = time.perf_counter()
            for _ in range(enc_reps):
                h16 = model.propagate()
            torch.cuda.synchronize()
            barrier()
            encoder_bf16 = {"encoder_ms": round(LD.max_over_ranks((time.perf_counter() - t0) * 1e3 / enc_reps, dev), 4),
                            "max_abs_diff_x_node_vs_f32": float((h16 - h).abs().max())}
            model.encoder_precision = "f32"
            del h16
        del h2

    # ---- bf16 throughput mode (extra keys; the headline stays fp32 = the reference's precision): same steps with
    #      model.precision = "bf16" (bf16 storage of Z + bf16 matrix cores in the attention kernel)
    bf16 = None
    if not args.no_bf16 and d in (32, 64, 128, 256):
        model.precision = model.tail_precision = "bf16"
        for i in range(max(args.warmup, len(lanes))):
            step_on(i)
        torch.cuda.synchronize()
        barrier()
        t0 = time.perf_counter()
        for i in range(args.steps):
            out16 = step_on(i)
        torch.cuda.synchronize()
        barrier()
        el16 = LD.max_over_ranks(time.perf_counter() - t0, dev)
        model.precision = model.tail_precision = "f32"
        ref_l = model.score_pairs(batches[0], h, score, logits=True).clone()
        model.precision = model.tail_precision = "bf16"
        got_l = model.score_pairs(batches[0], h, score, logits=True)
        bf16 = {"role": ("an option, not a throughput mode: at D >= 128 the attention waits on its instruction chain, not "
                         "on bytes (DESIGN.md section 8, row g1)" if d >= 128 else
                         "bf16 node table + bf16 matrix cores in the attention and the tail"),
                "value": round(world * bs * args.steps / el16, 1), "unit": "pairs/s",
                "ms_per_step": round(el16 * 1e3 / args.steps, 4),
                "max_abs_logit_diff_vs_f32": float((got_l - ref_l).abs().max()),
                "what": "bf16 storage of the node table Z; attention: "
                        + ("the activation-pattern kernel on the bf16 table, fp32 arithmetic (no D x D product left "
                           "to run in bf16)" if model.attention_kernel() == "flip" else
                           "v_mfma_f32_32x32x16_bf16 for Wfold h")
                        + "; bf16 weights and v_mfma_f32_16x16x16_bf16 for the two GEMMs of the dense tail (fp32 "
                          "accumulate everywhere); selection, q, softmax, record merge, LayerNorms in fp32; selected "
                          "index sets identical to fp32"}
        KernelTimer.reset()
        KernelTimer.enabled = True
        for i in range(args.steps):
            step(i)
        kt16 = KernelTimer.summary()
        KernelTimer.enabled = False
        for att_name in ("pair_attention_rows", "pair_attention_fused"):
            if att_name in kt16:
                bf16["pair_attention_fused_ms"] = round(kt16[att_name][2], 4)
                bf16["attention_kernel"] = KERNEL_NAMES[att_name]
                break
        if "tail_chain" in kt16:
            bf16["tail_chain_ms"] = round(kt16["tail_chain"][2], 4)
        model.precision = model.tail_precision = "f32"
    if bf16 is not None and encoder_bf16 is not None:
        bf16.update(encoder_bf16)
    elif encoder_bf16 is not None:
        bf16 = dict(encoder_bf16, what="bf16 storage of the aggregation's gathered table only (D = 256: the pair stage "
                                      "has no bf16 kernels)")

    # ---- instrumented replay of the same steps: HIP events around every kernel launch on the launch stream
    # (recording ~50 events per step costs ~0.1 ms per step, so it is kept out of the headline timing)
    instrumented_ms = None
    if not args.no_kernel_timing:
        KernelTimer.reset()
        KernelTimer.enabled = True
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for i in range(args.steps):
            step(i)
        torch.cuda.synchronize()
        instrumented_ms = (time.perf_counter() - t1) * 1e3 / args.steps
        KernelTimer.enabled = False

    ms_per_step = elapsed * 1e3 / args.steps
    pairs_per_s = world * bs * args.steps / elapsed
    flips_random = model.flips_per_entry(raw=True) if d >= 128 else None
    attention_random = model.attention_kernel()

    # ---- the same window on TRAINED weights (extra keys): the activation-pattern attention
    #      kernel's cost depends on how many hidden units of the PE MLPs leave the activation pattern of (0, 0), i.e. on
    #      the ppr_encoder_* weights; the headline uses random-init weights as the bench contract prescribes.  A few
    #      hundred steps of the repo's own training step (lpformer_amd/train.py: positives = existing edges, negatives =
    #      uniform pairs, Adam) move them the way training does; `auto` then re-decides between the two kernels.
    trained = None
    if args.weights == "both":
        saved = ({k: v.detach().clone() for k, v in model.state_dict().items()},
                 {k: v.detach().clone() for k, v in score.state_dict().items()})
        pos_e = torch.from_numpy(ei[:, ei[0] < ei[1]]).to(dev)
        opt = torch.optim.Adam(list(model.parameters()) + list(score.parameters()), lr=args.train_lr)
        tb, losses = 4096, []
        gen = torch.Generator(device=dev)
        gen.manual_seed(4321)
        model.train(); score.train()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for it in range(args.train_steps):
            idx = torch.randint(0, pos_e.shape[1], (tb,), device=dev, generator=gen)
            neg = torch.randint(0, n, (2, tb), device=dev, generator=gen)
            loss = (-torch.log(score(model(pos_e[:, idx])) + 1e-6).mean()
                    - torch.log(1 - score(model(neg)) + 1e-6).mean())
            loss.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
            opt.step()
            opt.zero_grad()
            if it < 5 or it >= args.train_steps - 5:
                losses.append(float(loss.detach()))
        torch.cuda.synchronize()
        train_s = time.perf_counter() - t0
        model.eval(); score.eval()
        del opt
        h_rand, scorers_rand, planned_rand = h, scorers, planned
        h = model.propagate()
        torch.cuda.synchronize()
        if launch == "graph":
            scorers = [lpformer_amd.GraphedScorer(model, score, h, batches[k % len(batches)]) for k in range(len(lanes))]
        if launch == "plan":
            planned = [lpformer_amd.PlannedScorer(model, score, h, batches[k % len(batches)], adopt_input=True)
                       for k in range(len(lanes))]
        for i in range(max(args.warmup, 2 * len(lanes))):
            step_on(i)
        torch.cuda.synchronize()
        tr_s = []
        for _ in range(max(1, args.repeats)):
            el, out = window()
            tr_s.append(el)
            assert torch.isfinite(out).all()
        ok = (all(sc.check() for sc in (scorers if launch == "graph" else planned)) if launch != "eager"
              else all(model.check_selection(lane) for lane in lanes))
        assert ok, "a timed step of the trained-weights leg overflowed its selection workspace"
        el_t = float(np.median(tr_s))
        trained = {"train_steps": args.train_steps, "train_batch": f"{tb} positives + {tb} negatives", "lr": args.train_lr,
                   "train_ms_per_step": round(train_s * 1e3 / max(1, args.train_steps), 2),
                   "loss_first5_mean": round(float(np.mean(losses[:5])), 4) if losses else None,
                   "loss_last5_mean": round(float(np.mean(losses[-5:])), 4) if losses else None,
                   "flips_per_entry": None if d < 128 else round(model.flips_per_entry(raw=True), 3),
                   "flips_per_entry_not_tabulated": None if d < 128 else round(model.flips_per_entry(), 3),
                   "attention_impl": model.attention_kernel(),
                   "ms_per_step": round(el_t * 1e3 / args.steps, 4),
                   "value": round(world * bs * args.steps / el_t, 1), "unit": "pairs/s"}
        # back to the random-init weights for everything below (kernel timings, CPU baseline)
        model.load_state_dict(saved[0])
        score.load_state_dict(saved[1])
        scorers, planned = scorers_rand, planned_rand
        del h_rand, saved
        h = model.propagate()
        torch.cuda.synchronize()
    value_incl_encoder = (None if encoder_ms is None else
                          world * bs / ((ms_per_step + encoder_ms + node_keys_ms) * 1e-3))

    kt = KernelTimer.summary() if not args.no_kernel_timing else {}
    enc = {}
    if args.full:
        # one instrumented encoder pass for the aggregation kernel's roofline -- on EVERY rank: a row-sharded encoder
        # all-gathers, and a collective issued by rank 0 alone would wait for ever
        KernelTimer.reset()
        KernelTimer.enabled = True
        model.propagate()
        enc = KernelTimer.summary()
        KernelTimer.enabled = False

    result = None
    if rank == 0:
        # ---- roofline: every modelled kernel, the dominant one of the timed region reported as "roofline"
        roofline, rooflines, kernels, pair_stage = None, {}, {}, None
        if kt:
            tot = sum(v[1] for v in kt.values())
            kernels = {k: {"launches": v[0], "ms_per_step": round(v[1] / args.steps, 4),
                           "share": round(v[1] / tot, 3)} for k, v in sorted(kt.items(), key=lambda kv: -kv[1][1])}
            # structural totals over the batches actually timed
            tp = [model.compute_node_mask(b) for b in batches]
            nsel = [sum(int(t[0].shape[1]) for t in sel if t is not None) for sel in tp]
            # pairs that select at least one node (the others take the short form of the score head)
            nfull = [int(torch.unique(torch.cat([t[0][0] for t in sel if t is not None])).numel()) for sel in tp]
            stats = [dict(pair_stats(data, b), slots=slot_count(model, bt)) for b, bt in zip(batches_np, batches)]
            used = [i % len(batches) for i in range(args.steps)]
            mean = lambda arr: float(np.mean([arr[i] for i in used]))  # noqa: E731
            n_sel, sum_deg = mean(nsel), mean([s["sum_deg"] for s in stats])
            n_full = mean(nfull)
            sum_ppr = mean([s["sum_ppr_len"] for s in stats])
            # algorithmic work per launch: bytes for the HBM-bound kernels, FLOPs for MFMA ones
            slots = mean([s["slots"] for s in stats])
            c = model.count_dim
            tail_short = bool(model.tail_skip_empty and model._uses_rows())
            four = bool(model._uses_select4() and model._uses_rows())
            four_r = bool(not four and model._uses_select4_regions())   # lpf_select4 + lpf_select4_regions (type-major consumers)
            q_rides = model.query_from == "table" and "pair_gather_q" not in kt
            # the WHOLE pair stage against the HBM roof: SURVEY 8(d)'s B_pair summed over the batch (what a both-rows
            # walk of the reference's algorithm must touch) / the measured step time
            b_pair = 4.0 * sum_deg + 8.0 * sum_ppr + (32.0 + 16.0 + 4.0) * bs + 4.0 * d * (2.0 * bs + n_sel)
            pair_stage = {"survey_8d_bytes_per_step": round(b_pair, 0),
                          "hbm_frac_of_8TBs": round(b_pair / (ms_per_step * 1e-3) / (HBM_PEAK_GBS * 1e9), 4),
                          "hbm_frac_of_6.3TBs": round(b_pair / (ms_per_step * 1e-3) / 6.3e12, 4)}
            work = {
                # one-pass attention (score + segment softmax + weighted sum).  "mfma": SURVEY 8(d) n_sel * (2 D^2 +
                # ~20 D) FLOP on the fp32 matrix cores.  "flip" (default): the D x D product is gone, what
                # is left is the gather -- one fp32 Z row + one 16-byte record per selected entry, one q row read and
                # about one (D + 4)-float record written per pair: SURVEY 8(d)'s e D (2 + n_sel) term of B_pair
                "pair_attention_fused": (("hbm", n_sel * (4.0 * d + 16.0) + bs * (4.0 * d + 4.0 * (d + 4)))
                                         if model.attention_kernel() == "flip" else
                                         ("mfma", n_sel * (2.0 * d * d + 20.0 * d))),
                # the pair-major form of the same arithmetic (pair_rows.hip): a finished row per pair instead of records
                "pair_attention_rows": ("hbm", n_sel * (4.0 * d + 16.0) + bs * (4.0 * d + 4.0 * (d + 4))),
                # legacy two-pass kernels (D = 256 and the module-by-module API)
                "pair_scores": ("mfma", n_sel * (2.0 * d * d + 20.0 * d)),
                "pair_softmax_gather": ("hbm", n_sel * (4.0 * d + 16.0) + bs * (4.0 * (4 * d + 4) + 48.0)),
                # selection, run kernel (walk plan): per candidate slot the walked {node, value} entry (8 B) and the
                # answer of its one look-up ({node, value | adjacent}: 8 B of a 64-byte bucket), 148 B per pair
                # (descriptor, offset, three segment starts), one 16-byte record per selected entry
                # (one-launch form, select4.hip: no descriptors or offsets in memory -- per pair two ids, two 64-byte node
                #  records, two 128-byte filters and a 16-byte table entry)
                "select_run": ("hbm", 16.0 * slots + ((16.0 + 128.0 + 256.0 + 16.0) if (four or four_r) else 148.0) * bs + 16.0 * n_sel),
                # pair-major -> type-major (lpf_select4_regions): a table entry in, three pointers out per pair, every kept
                # record read and written once
                "select_regions": ("hbm", (16.0 + 12.0) * bs + 2 * 16.0 * n_sel),
                # plan kernel: two node ids, two 64-byte node records, descriptor + offset per pair
                "select_plan": ("hbm", (16.0 + 2 * 64.0 + 128.0 + 8.0) * bs),
                "select_export": ("hbm", 2 * 16.0 * n_sel + 40.0 * bs),
                # q = lin_l(x_a) + lin_l(x_b) = W_l (x_a + x_b) + 2 b_l: the endpoint rows gathered and added inside the
                # first stage of a [BS, D] x [D, D] product
                "pair_q": ("mfma", 2.0 * bs * d * d),
                # ... or, with the per-node table Y = X W_l^T + b_l (model.query_from = "table", the default): two
                # gathered rows in, one row out per pair
                "pair_gather_q": ("hbm", 3.0 * 4.0 * d * bs + 16.0 * bs),
                "dense_chain_score": ("mfma", 2.0 * bs * (2 * d) * (2 * d + c + 1)),  # folded first layer
                "dense_chain_mlp": ("mfma", (2.0 * bs * (2 * d * d) + 2.0 * bs * (d + c) * (2 * d + c)) / 2.0),
                "dense_chain_attn_out": ("mfma", 2.0 * bs * d * (3 * d + 4)),
                # merged dense tail: record merge + post-norm (no GEMM), first layer of pairwise_lin, folded score head
                # (pairs without selected nodes -- workgroups of 64 of them -- need the r_e half of the head only: the
                #  FLOPs counted are the ones the launch has to do, not the ones the reference spends on constants)
                "tail_chain": ("mfma", (2.0 * bs * ((d + c) ** 2 + 2 * d * (2 * d + c)) if not tail_short else
                                        2.0 * (n_full * ((d + c) ** 2 + 2 * d * (2 * d + c)) + (bs - n_full) * 2 * d * d))),
                # first layer of elementwise_lin alone (score_pairs): D x D -- and, in the same launch, the query gather
                # q = Y[a] + Y[b]: two table rows per endpoint in, two rows out, 1.1 GFLOP beside them
                "dense_chain_mlp_hidden": (("hbm", (6.0 * 4.0 * d + 16.0) * bs) if q_rides else
                                           ("mfma", 2.0 * bs * d * d)),
            }
            for name, (bound, units) in work.items():
                if name not in kt:
                    continue
                dur_s = kt[name][2] * 1e-3
                peak = HBM_PEAK_GBS if bound == "hbm" else F32_MFMA_PEAK_TFLOPS
                ach = units / dur_s / (1e9 if bound == "hbm" else 1e12)
                kname = KERNEL_NAMES.get(name, name)
                if name == "select_run":
                    kname = "select4_kernel" if (four or four_r) else "select3_run_kernel"
                if name == "pair_attention_fused":
                    kname = "pair_flip_kernel" if model.attention_kernel() == "flip" else "pair_fused_kernel"
                rooflines[name] = {"kernel": kname, "span": name, "bound": bound, "achieved": round(ach, 2), "peak": peak,
                                   "unit": "GB/s" if bound == "hbm" else "TFLOP/s", "frac": round(ach / peak, 4),
                                   "traffic": None, "launch_ms": round(kt[name][2], 4),
                                   "launches_per_step": kt[name][0] / args.steps,
                                   "algorithmic": round(units, 0)}
            # HBM traffic per launch: NOT measured in this run -- read from the committed rocprofv3 PMC passes
            # (FETCH_SIZE / WRITE_SIZE, gfx950-corrected; tools/collect_profiles.sh) and tagged with that file
            try:
                if world > 1:
                    raise KeyError("the committed PMC passes were collected on one GPU")
                pmc_file = os.path.join("profiles", PMC_FILE.format(config=args.config))
                pmc = json.load(open(os.path.join(ROOT, pmc_file)))
                rows_form = model._uses_rows()
                for name, r in rooflines.items():
                    key = {"tail_chain": "tail_chain_rows"}.get(name, name) if rows_form else name
                    if name == "select_run":
                        key = "select4" if (four or four_r) else "select3_run"
                    if name == "pair_attention_fused" and model.attention_kernel() != "flip":
                        key = "pair_attention_fused_mfma"
                    if key in pmc["kernels"]:
                        r["traffic"] = pmc["kernels"][key]["hbm_bytes_per_launch_corrected"]
                        r["traffic_source"] = f"{pmc_file} (offline rocprofv3 PMC passes at {pmc.get('commit', '?')})"
            except (OSError, KeyError, ValueError):
                pass
            relabel_cache_resident(rooflines)
            # how much of the dominant kernel's wave time is waiting (SQ_WAIT_ANY / SQ_WAVE_CYCLES of a committed SQ
            # counter pass): "hbm" is a nominal bound for a kernel that waits on its own instruction chain
            try:
                sq = json.load(open(os.path.join(ROOT, "profiles", PMC_SQ_FILE.format(config=args.config))))
                for name, r in rooflines.items():
                    hit = sq["kernels"].get(r["kernel"].split("<")[0])
                    if hit:
                        r["wave_wait_frac"] = round(hit["SQ_WAIT_ANY"] / max(hit["SQ_WAVE_CYCLES"], 1.0), 4)
                        r["valu_insts_per_launch"] = hit.get("SQ_INSTS_VALU")
                        r["sq_source"] = f"profiles/{PMC_SQ_FILE.format(config=args.config)} at {sq.get('commit', '?')}"
            except (OSError, KeyError, ValueError):
                pass
            if bf16 is not None and "pair_attention_fused_ms" in bf16:
                # bf16 mode: the attention kernel is HBM-bound -- one bf16 Z row + one 16-byte record per selected
                # entry, one fp32 q row read and about one fp32 record written per pair
                byts = n_sel * (2.0 * d + 16.0) + bs * (4.0 * d + 4.0 * d + 16.0)
                ach = byts / (bf16["pair_attention_fused_ms"] * 1e-3) / 1e9
                bf16["roofline"] = {"kernel": bf16.get("attention_kernel", "pair_fused_kernel") + " (bf16 node table)", "bound": "hbm", "achieved": round(ach, 1),
                                    "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4),
                                    "traffic": None, "launch_ms": bf16["pair_attention_fused_ms"]}
            modelled = [k for k in sorted(kt, key=lambda k: -kt[k][1]) if k in rooflines]
            if modelled:
                roofline = dict(rooflines[modelled[0]])
                roofline["batch_stats"] = {"n_sel": n_sel, "sum_deg": sum_deg, "sum_ppr_len": sum_ppr, "slots": slots,
                                           "pairs_with_selected_nodes": n_full}
        # encoder aggregation kernel (outside the timed pair-stage region): SURVEY 8(d) bytes per layer.  A square layer
        # runs as ONE launch (gcn_layer_fused: aggregation + transform + epilogue, csrc/gcn_fused.hip) with the same
        # algorithmic bytes as the aggregation alone -- the D x D product adds no memory traffic
        for ename, label in (("gcn_layer_fused", "gcn_layer_fused + spmm_row_parts (encoder layer: aggregation + transform)"),
                             ("spmm_csr", "spmm_csr (encoder, per layer)")):
            if ename not in enc:
                continue
            a_hat = model._device_graph("prop", data["adj_t"])
            nnz, n_rows = a_hat.nnz, n
            if world > 1 and model.encoder_mode == "sharded":  # this rank aggregates its row block only
                # (gather_once: the per-launch average mixes whole-graph and row-block launches; N = 1 figures are the
                #  ones the roofline is quoted on)
                lo, hi = LD.row_range(n, world, rank)
                nnz, n_rows = int(a_hat.rowptr[hi] - a_hat.rowptr[lo]), hi - lo
            byts = nnz * 8.0 + 8.0 * (n_rows + 1) + 4.0 * d * nnz + 4.0 * d * n_rows
            # the fused layer's hub rows are summed by a launch of their own in front of it (spmm_row_parts): the two
            # launches together are the layer, and together they are priced
            layer_ms = enc[ename][2] + (enc["spmm_row_parts"][2] if ename == "gcn_layer_fused" and
                                        "spmm_row_parts" in enc else 0.0)
            ach = byts / (layer_ms * 1e-3) / 1e9
            # every feature row read once (all of them: any row can be a neighbour) + the local rows written once
            floor = nnz * 8.0 + 8.0 * (n_rows + 1) + 4.0 * d * n + 4.0 * d * n_rows
            ach_floor = floor / (layer_ms * 1e-3) / 1e9
            rooflines[ename] = {"kernel": label, "bound": "hbm",
                                "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": None, "algorithmic": round(byts, 0),
                                "launch_ms": round(layer_ms, 4),
                                # gathered bytes (every neighbour row counted, L2 / Infinity Cache
                                # serve most of them) above; the compulsory floor (each row once) here
                                "achieved_compulsory_floor": round(ach_floor, 1),
                                "frac_compulsory_floor": round(ach_floor / HBM_PEAK_GBS, 4)}
            try:
                pmc_file = os.path.join("profiles", PMC_FILE.format(config=args.config))
                pmc = json.load(open(os.path.join(ROOT, pmc_file)))
                if world == 1 and ename in pmc["kernels"]:
                    rooflines[ename]["traffic"] = pmc["kernels"][ename]["hbm_bytes_per_launch_corrected"] + (
                        pmc["kernels"].get("spmm_row_parts", {}).get("hbm_bytes_per_launch_corrected", 0)
                        if ename == "gcn_layer_fused" else 0)
                    rooflines[ename]["traffic_source"] = f"{pmc_file} (offline rocprofv3 PMC passes)"
            except (OSError, KeyError, ValueError):
                pass
        relabel_cache_resident({k: v for k, v in rooflines.items() if k in ("gcn_layer_fused", "spmm_csr")})
        if roofline is not None and roofline.get("span") in rooflines:   # (the headline entry follows its relabelled twin)
            roofline.update({k: v for k, v in rooflines[roofline["span"]].items() if k != "batch_stats"})

        # ---- CPU baseline: the oracle's pair stage on a bounded sample of the same workload (rank 0, N = 1 only)
        cpu = None
        if not args.no_cpu_baseline and world == 1:
            try:
                cpu = cpu_baseline(args, model, score, targs, data, batches_np, h, bs, dev)
            except (RuntimeError, OSError) as exc:   # the GPU measurement above stands on its own
                cpu = {"value": None, "unit": "pairs/s", "cores": 0, "kind": "port", "sample": f"not measured: {exc}"}

        result = {
            "metric": "candidate link-pairs scored/sec (whole node)", "value": round(pairs_per_s, 1),
            "unit": "pairs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"{args.config}-like synthetic graph (N={n}, {cfg['edges']} undirected edges, "
                                   f"F={cfg['f_in']}, D={d}, L={cfg['gnn_layers']}, thresholds={cfg['thresholds']}, "
                                   f"PPR eps={cfg['eps']}), {bs} candidate pairs per GPU per step, pair stage with "
                                   "encoder output resident",
                       "pairs_per_step_per_gpu": bs, "distinct_batches": len(batches),
                       "streams": len(lanes), "side_stream": bool(model.use_side_stream), "launch": {"graph": "one captured HIP graph of the step per stream, replayed",
                                  "plan": "the recorded C-ABI launches of the step per stream, replayed as plain launches",
                                  "eager": "eager (LinkTransformer.score_pairs per step)"}[launch],
                       "launch_probe_ms_per_step": launch_probe,
                       "spinup_s": args.spinup, "attention_impl": attention_random,
                       "attention_impl_requested": args.attention, "flips_per_entry": flips_random,
                       "attention_form": ("pair-major, finished rows (pair_rows.hip)" if model._uses_rows() else
                                          "unit-major, records merged by the tail (pair_flip.hip / pair_fused.hip)"),
                       "attention_form_probe_ms_per_step": rows_probe,
                       "selection_form": ("one launch, pair-major entries + a table entry per pair (select4.hip)"
                                          if model._uses_select4() and model._uses_rows() else
                                          ("one launch, pair-major (select4.hip) + lpf_select4_regions: type-major regions"
                                           if model._uses_select4_regions() else
                                           "plan + run launches, type-major regions (select3.hip)")),
                       "flip_break_even": model.flip_break_even() if d >= 128 else None,
                       # the activation-pattern table of the attention behind select4 (random-init weights): share of a
                       # sample's ordered (pa, pb) points per type whose cell holds a tabulated pattern, and the flipped
                       # units per entry left for the exact path (lpformer_amd/patterns.py)
                       "pattern_table": (None if not (d >= 128 and model._uses_select4() and model._uses_rows()) else
                                         {"covered_per_type": [s_["covered"] for s_ in model._pattern_tables(model._fold())["stats"]],
                                          "flips_per_entry_left": round(model._flip_stats()[1], 4),
                                          "grid_cells_per_axis": model._pattern_tables(model._fold())["geo"]["n"]}),
                       "parallelism": (f"pairs sharded x{world}, encoder {enc_plan['chosen']} " +
                                       {"sharded": "(rows + all-gather per layer)",
                                        "gather_once": "(last layer + Z on row blocks, one all-gather of [X | Z])",
                                        "replicated": "(every rank runs it, no exchange)"}[enc_plan["chosen"]])
                       if world > 1 else "single GPU",
                       "encoder_plan": enc_plan},
            "ms_per_step_repeats": {"n": len(rep_ms), "min": round(min(rep_ms), 4),
                                    "median": round(float(np.median(rep_ms)), 4), "max": round(max(rep_ms), 4)},
            "setup_s": dict({k: round(v, 2) for k, v in setup.items()}, ppr_producer=args.ppr,
                            index_bytes=index_bytes),
        }
        if args.full:
            result.update({
                "encoder_ms": round(encoder_ms, 4), "node_keys_ms": round(node_keys_ms, 4),
                "value_incl_encoder": round(value_incl_encoder, 1),
                "ms_per_step_instrumented": None if instrumented_ms is None else round(instrumented_ms, 4),
                "roofline": roofline, "cpu_baseline": cpu,
                "pair_stage_hbm_frac": None if pair_stage is None else pair_stage["hbm_frac_of_8TBs"],
                "pair_stage": pair_stage, "trained_weights": trained,
                "bf16_mode": bf16, "kernels": kernels, "rooflines": rooflines,
            })
        print(json.dumps(result), flush=True)
    barrier()
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
