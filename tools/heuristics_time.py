"""Device time of pair_heuristics (CN / AA / RA: lpf_pair_heuristics_f32) on the synthetic collab-like and ppa-like
graphs, next to one score_pairs step on the same 32,768-pair batch (HIP events around REPS back-to-back calls, so the
queue runs ahead of the host and the span is the device's).  Also the share of pairs the split threshold sends to the
workgroup-per-pair kernel, and the time at a few other thresholds.
    LPF_CFGS="collab ppa" LPF_REPS=20 LPF_SPLITS="0 16 64 128" python tools/heuristics_time.py"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import lpformer_amd
from lpformer_amd import data as D
from lpformer_amd.heuristics import pair_heuristics

REPS = int(os.environ.get("LPF_REPS", "20"))
SPLITS = [int(s) for s in os.environ.get("LPF_SPLITS", "0 16 64 128").split()]
dev = torch.device("cuda:0")


def span_ms(fn, reps=REPS):
    fn(); fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    host = (time.perf_counter() - t0) / reps * 1e3
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, host


for name in os.environ.get("LPF_CFGS", "collab ppa").split():
    cfg = D.CONFIGS[name]
    n = cfg["n"]
    t0 = time.perf_counter()
    ei, w = D.chung_lu_graph(n, cfg["edges"], gamma=cfg["gamma"], seed=0, max_weight=cfg["max_weight"])
    x = np.random.default_rng(1).standard_normal((n, cfg["f_in"])).astype(np.float32)
    data = D.build_data(ei, x, n, edge_weight=w, eps=cfg["eps"], ppr_device=dev)
    torch.manual_seed(0)
    model = lpformer_amd.LinkTransformer(D.train_args_for(cfg), data, device=dev).to(dev).eval()
    score = lpformer_amd.mlp_score(model.out_dim, model.out_dim, 1, 2).to(dev).eval()
    batch = torch.from_numpy(D.sample_pairs(ei, n, 32_768, seed=7)).to(dev)
    print(f"# {name}: n {n}, {ei.shape[1]} directed edges, setup {time.perf_counter() - t0:.1f} s", flush=True)

    adj = model._device_graph("mask", model._data_obj("mask", False))
    deg = (adj.rowptr[1:] - adj.rowptr[:-1]).cpu().numpy()
    b = batch.cpu().numpy()
    walk = np.minimum(deg[b[0]], deg[b[1]])
    print(f"  walked row per pair: mean {walk.mean():.1f}, p99 {np.percentile(walk, 99):.0f}, max {walk.max()}; "
          f"probes x log2(longer row) {float((walk * np.log2(np.maximum(np.maximum(deg[b[0]], deg[b[1]]), 2))).sum()):.3g}")

    h = model.propagate()
    with torch.no_grad():
        score_ms, score_host = span_ms(lambda: model.score_pairs(batch, h, score))
    heur_ms, heur_host = span_ms(lambda: pair_heuristics(model, batch))
    cn_ms, _ = span_ms(lambda: pair_heuristics(model, batch, kinds=("cn",)))
    all_ms, _ = span_ms(lambda: pair_heuristics(model, batch, kinds=("cn", "aa", "ra", "ppr", "feat")))
    print(f"  score_pairs step      {score_ms:8.3f} ms device  ({score_host:.3f} ms host per call)")
    print(f"  cn + aa + ra          {heur_ms:8.3f} ms device  ({heur_host:.3f} ms host per call)  "
          f"{heur_ms / score_ms:.2f} x the scoring step")
    print(f"  cn only               {cn_ms:8.3f} ms device")
    print(f"  all five kinds        {all_ms:8.3f} ms device")
    for thr in SPLITS:
        ms, _ = span_ms(lambda: pair_heuristics(model, batch, split_threshold=thr))
        print(f"  split_threshold {thr:5d}  {ms:8.3f} ms device  ({(walk > thr).mean() * 100:.2f} % of pairs on the "
              f"workgroup kernel)", flush=True)
    del model, data, h
    torch.cuda.empty_cache()
