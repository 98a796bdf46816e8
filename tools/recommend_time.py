"""Device time of the three stages of lpformer_amd.recommend on synthetic graphs: the candidate passes
(lpf_rec_candidate_count + exclusive scan + lpf_rec_candidate_fill), the scoring (evaluate.score_edges, logits) and the
segmented top-K (lpf_segment_topk_f32), plus the candidates per source (mean, p99).  HIP events around each stage,
one chunk holding every source.  Then the top-K kernel against a torch baseline on synthetic segments: a stable
torch.sort of the same keys (order-preserving uint32 of the score, descending; ties by position through stability),
then a stable sort by segment id, then the first k of each segment.
    LPF_RECS="collab:4096:ppr ddi:0:all" LPF_K=100 LPF_REPS=5 python tools/recommend_time.py
(config:sources:mode; 0 sources = every node)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import lpformer_amd
from lpformer_amd import data as D
from lpformer_amd import evaluate as E
from lpformer_amd.recommend import generate_candidates, segment_topk

K = int(os.environ.get("LPF_K", "100"))
REPS = int(os.environ.get("LPF_REPS", "5"))
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


def torch_topk(seg_ptr, score, cand, k):
    b = score.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    b = torch.where(b == 0x80000000, torch.zeros_like(b), b)
    key = torch.where(b >= 0x80000000, 0xFFFFFFFF - b, b | 0x80000000)
    key = torch.where(torch.isnan(score), torch.zeros_like(key), key)
    lens = seg_ptr[1:] - seg_ptr[:-1]
    seg = torch.repeat_interleave(torch.arange(lens.numel(), device=score.device), lens)
    o1 = torch.sort(key, descending=True, stable=True).indices
    o2 = torch.sort(seg[o1], stable=True).indices
    order = o1[o2]
    rank = torch.arange(order.numel(), device=score.device) - seg_ptr[:-1].repeat_interleave(lens)
    keep = rank < k
    ids = torch.full((lens.numel(), k), -1, dtype=torch.int64, device=score.device)
    ids[seg[order][keep], rank[keep]] = cand[order][keep]
    return ids


for spec in os.environ.get("LPF_RECS", "collab:4096:ppr ddi:0:all").split():
    name, ns, mode = spec.split(":")
    cfg = D.CONFIGS[name]
    n = cfg["n"]
    t0 = time.perf_counter()
    ei, w = D.chung_lu_graph(n, cfg["edges"], gamma=cfg["gamma"], seed=0, max_weight=cfg["max_weight"])
    x = np.random.default_rng(1).standard_normal((n, cfg["f_in"])).astype(np.float32)
    data = D.build_data(ei, x, n, edge_weight=w, eps=cfg["eps"], ppr_device=dev)
    torch.manual_seed(0)
    model = lpformer_amd.LinkTransformer(D.train_args_for(cfg), data, device=dev).to(dev).eval()
    score = lpformer_amd.mlp_score(model.out_dim, model.out_dim, 1, 2).to(dev).eval()
    S = int(ns) or n
    src = torch.from_numpy(np.random.default_rng(2).integers(0, n, size=S) if int(ns) else np.arange(n)).to(dev)
    h = model.propagate()
    ppr = model._device_graph("ppr", model._data_obj("ppr", False)) if mode == "ppr" else None
    adj = model._device_graph("mask", model._data_obj("mask", False))
    print(f"{name}: n={n} set-up {time.perf_counter() - t0:.1f} s", flush=True)

    counts, fill = generate_candidates(n, src, ppr, 0.0, adj, True)
    total = int(counts.sum())
    pairs = fill(0, S, total)
    seg_ptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(counts, 0)])
    lg = E.score_edges(model, score, pairs, h=h, logits=True)
    c = counts.double()

    def cand_passes():
        cnt, f = generate_candidates(n, src, ppr, 0.0, adj, True)
        f(0, S, total)
    t_cand = span_ms(cand_passes)
    t_score = span_ms(lambda: E.score_edges(model, score, pairs, h=h, logits=True), reps=max(1, REPS // 2))
    t_topk = span_ms(lambda: segment_topk(seg_ptr, lg, pairs[1], K))
    t_rec = span_ms(lambda: lpformer_amd.recommend(model, score, src, K, candidates=mode, h=h), reps=max(1, REPS // 2))
    print(f"  {mode}, {S} sources, k={K}: candidates/source mean {float(c.mean()):.1f} p99 "
          f"{float(torch.quantile(c.cpu(), 0.99)):.0f}, pairs {total}", flush=True)
    print(f"  candidate passes {t_cand:.3f} ms | scoring {t_score:.3f} ms | top-K {t_topk:.3f} ms | "
          f"(candidates + top-K) / scoring = {(t_cand + t_topk) / t_score * 100:.1f} % | recommend() {t_rec:.3f} ms",
          flush=True)
    del pairs, lg, model, data
    torch.cuda.empty_cache()

g = torch.Generator(device="cpu").manual_seed(3)
for S, L in ((32768, 110), (64, 1 << 21)):
    lens = torch.full((S,), L, dtype=torch.int64) if L > 1000 else torch.randint(L // 2, 3 * L // 2, (S,), generator=g)
    seg_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)]).to(dev)
    P = int(seg_ptr[-1])
    sc = torch.randn(P, generator=g).to(dev)
    cand = torch.arange(P, dtype=torch.int64, device=dev)
    ids, _, _ = segment_topk(seg_ptr, sc, cand, K)
    assert torch.equal(ids, torch_topk(seg_ptr, sc, cand, K)), "top-K kernel and torch baseline disagree"
    t_k = span_ms(lambda: segment_topk(seg_ptr, sc, cand, K))
    t_t = span_ms(lambda: torch_topk(seg_ptr, sc, cand, K))
    print(f"top-K {S} segments of ~{L} (k={K}): kernel {t_k:.3f} ms, torch sort baseline {t_t:.3f} ms "
          f"({t_t / t_k:.1f}x)", flush=True)
