"""Device time of the phases of lpformer_amd.heart_negatives on synthetic graphs -- two-hop rows (count + fill), pool,
feature cosine, top-K x H, interleave; HIP events around each phase, summed over the chunks -- next to one
evaluate.score_negatives sweep over the negatives it made, and the two-hop passes alone against the class threshold.
    LPF_CFGS="collab ppa" LPF_P=32768 LPF_K=500 LPF_HEUR="ra ppr feat" LPF_SPLITS="-1 128 0" LPF_REPS=3 \
        python tools/hard_negatives_time.py"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import lpformer_amd
from lpformer_amd import data as D
from lpformer_amd import evaluate as E
from lpformer_amd.hard_negatives import TwoHop

P = int(os.environ.get("LPF_P", "32768"))
K = int(os.environ.get("LPF_K", "500"))
HEUR = tuple(os.environ.get("LPF_HEUR", "ra ppr feat").split())
SPLITS = [int(v) for v in os.environ.get("LPF_SPLITS", "-1 128 0").split()]
REPS = int(os.environ.get("LPF_REPS", "3"))
dev = torch.device("cuda:0")


def span_ms(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


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
    ei = np.asarray(ei, np.int64)
    pos = torch.from_numpy(ei[:, np.random.default_rng(2).choice(ei.shape[1], P, replace=False)]).to(dev)
    h = model.propagate()
    print(f"{name}: n={n} set-up {time.perf_counter() - t0:.1f} s", flush=True)

    lpformer_amd.heart_negatives(model, pos, K, heuristics=HEUR)        # warm-up
    torch.cuda.synchronize()
    tm = {}
    t0 = time.perf_counter()
    hn = lpformer_amd.heart_negatives(model, pos, K, heuristics=HEUR, timings=tm)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    ms = {k: sum(a.elapsed_time(b) for a, b in v) for k, v in tm.items()}
    r = hn.list_ranked.double()
    print(f"  {P} positives, {hn.nodes.numel()} endpoints, k={K}, heuristics {HEUR}: ranked per list mean "
          f"{float(r.mean()):.1f} of {K // 2}, lists fully ranked {float((r == K // 2).double().mean()) * 100:.1f} %")
    print("  " + " | ".join(f"{k} {v:.3f} ms" for k, v in ms.items()) +
          f" | phases {sum(ms.values()):.3f} ms | heart_negatives() wall {wall:.1f} ms", flush=True)
    t_score = span_ms(lambda: E.score_negatives(model, score, hn.negatives, h=h), reps=1)
    print(f"  score_negatives over [{P}, {K}, 2]: {t_score:.3f} ms | generation / scoring = "
          f"{sum(ms.values()) / t_score * 100:.1f} %", flush=True)
    adj = model._device_graph("mask", model._data_obj("mask", False))
    for thr in SPLITS:
        def passes():
            th = TwoHop(adj, hn.nodes, ("ra",), 3, thr)
            lo = 0
            step = max(1, hn.nodes.numel() // 8)
            cnt = th.counts.cpu().numpy()
            for lo in range(0, cnt.size, step):
                th.fill(lo, min(lo + step, cnt.size), int(cnt[lo:lo + step].sum()))
        print(f"  two-hop count + fill, split_threshold {thr}: {span_ms(passes):.3f} ms", flush=True)
    del hn, model, data
    torch.cuda.empty_cache()
