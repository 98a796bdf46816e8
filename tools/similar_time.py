"""Device time of lpformer_amd.similar_nodes on the collab-like graph of bench.py (table = the encoder's output, D = 128,
m = 128, cosine, the typing adjacency excluded), for S in {16, 1,024, 32,768} sources:
  * the whole similar_nodes call and lpf_similar_topm_f32 alone (buffers made once), median of LPF_REPS runs;
  * next to each the same answer from torch on the same device: Q @ T.T in chunks of at most LPF_CHUNK_MB of scores,
    the two scales, a masked fill of the exclusion rows and the source itself with -inf, torch.topk -- and the share
    of rows on which the two agree id for id (torch.topk fixes no tie rule and its GEMM sums in another order);
  * recommend(candidates="similar") against candidates="all" for 16 sources.
Writes LPF_OUT (default profiles/similar_timing.json).  No ratio is asserted: the numbers are recorded as they fall.
    LPF_REPS=7 python tools/similar_time.py"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

REPS = int(os.environ.get("LPF_REPS", "7"))
CHUNK_MB = int(os.environ.get("LPF_CHUNK_MB", "1024"))
OUT = os.environ.get("LPF_OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                             "similar_timing.json"))
M = 128
SIZES = (16, 1024, 32768)


def spread_ms(fn, reps=REPS):
    """[median, min, max] ms of ``reps`` runs after one warm-up call, each between two device events."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return [float(np.median(ms)), float(min(ms)), float(max(ms))]


def torch_baseline(T, t_scale, rowptr, col, src, m, chunk_rows):
    """ids int64 [S, m] by a chunked score matrix: the [chunk, n] block exists, which the kernel never holds."""
    n = T.shape[0]
    out = []
    for lo in range(0, src.numel(), chunk_rows):
        u = src[lo:lo + chunk_rows]
        q = T[u]
        sc = (q @ T.t()) * t_scale[u][:, None] * t_scale[None, :]
        start, cnt = rowptr[u], rowptr[u + 1] - rowptr[u]
        rows = torch.repeat_interleave(torch.arange(u.numel(), device=T.device), cnt)
        flat = torch.arange(rows.numel(), device=T.device) + torch.repeat_interleave(start - (torch.cumsum(cnt, 0) - cnt),
                                                                                   cnt)
        sc[rows, col[flat].long()] = float("-inf")
        sc[torch.arange(u.numel(), device=T.device), u] = float("-inf")
        out.append(torch.topk(sc, min(m, n), dim=1).indices)
    return torch.cat(out)


def main():
    import lpformer_amd
    from lpformer_amd import _lib, similar
    from lpformer_amd import data as D
    from lpformer_amd._lib import check, ptr
    from lpformer_amd.ops import f32_rows, raw_stream

    assert torch.cuda.is_available(), "similar_time.py measures on an MI355X"
    dev = torch.device("cuda:0")
    cfg = D.CONFIGS["collab"]
    n = cfg["n"]
    t0 = time.perf_counter()
    ei, w = D.chung_lu_graph(n, cfg["edges"], gamma=cfg["gamma"], seed=0, max_weight=cfg["max_weight"])
    x = np.random.default_rng(1).standard_normal((n, cfg["f_in"])).astype(np.float32)
    data = D.build_data(ei, x, n, edge_weight=w, eps=cfg["eps"], ppr_device=dev)
    torch.manual_seed(0)
    model = lpformer_amd.LinkTransformer(D.train_args_for(cfg), data, device=dev).to(dev).eval()
    score = lpformer_amd.mlp_score(model.out_dim, model.out_dim, 1, 2).to(dev).eval()
    h = model.propagate()
    adj = model._device_graph("mask", model._data_obj("mask", False))
    print(f"collab-like graph: n = {n}, D = {h.shape[1]}, set-up {time.perf_counter() - t0:.1f} s", flush=True)

    T = f32_rows(h)
    ts = similar._inv_norm(T)
    hip = _lib.hip()
    res = {"graph": "collab", "n": n, "D": int(T.shape[1]), "m": M, "metric": "cosine", "exclude": "adj", "reps": REPS,
           "spread": "every ms_* entry is [median, min, max] of reps runs after one warm-up call",
           "device": torch.cuda.get_device_properties(0).gcnArchName, "torch": torch.__version__,
           "baseline_chunk_mb": CHUNK_MB}
    chunk_rows = max(1, CHUNK_MB * (1 << 20) // (4 * n))
    for S in SIZES:
        src = torch.from_numpy(np.random.default_rng(S).integers(0, n, size=S)).to(dev)
        Q = f32_rows(T[src])
        qs = similar._inv_norm(Q)
        ids = torch.empty((S, M), dtype=torch.int64, device=dev)
        out = torch.empty((S, M), dtype=torch.float32, device=dev)
        counts = torch.empty(S, dtype=torch.int64, device=dev)
        nbytes = hip.lpf_similar_workspace_bytes(S, M, -1)
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)

        def kernel():
            check(hip.lpf_similar_topm_f32(S, n, T.shape[1], ptr(Q), Q.stride(0), ptr(T), T.stride(0), ptr(qs), ptr(ts),
                                           ptr(src), ptr(adj.rowptr), ptr(adj.col), 1, M, -1, ptr(ws), ptr(ids),
                                           ptr(out), ptr(counts), raw_stream(dev)), "lpf_similar_topm_f32")
        r = {"ms_kernel": spread_ms(kernel),
             "ms_similar_nodes": spread_ms(lambda: lpformer_amd.similar_nodes(model, src, M, h=h)),
             "ms_torch_matmul_mask_topk": spread_ms(lambda: torch_baseline(T, ts, adj.rowptr, adj.col, src, M,
                                                                          chunk_rows)),
             "workspace_mb": nbytes / (1 << 20), "n_ranges": nbytes // (8 * S * M),
             "baseline_score_block_mb": min(S, chunk_rows) * n * 4 / (1 << 20)}
        got = lpformer_amd.similar_nodes(model, src, M, h=h)
        base = torch_baseline(T, ts, adj.rowptr, adj.col, src, M, chunk_rows)
        r["rows_equal_to_torch"] = float((got.ids == base).all(1).float().mean())
        r["ids_in_common_with_torch"] = float(torch.stack([torch.isin(a, b).float().mean()
                                                           for a, b in zip(got.ids[:256], base[:256])]).mean())
        r["kernel_tflops"] = 2.0 * S * n * T.shape[1] / (r["ms_kernel"][0] * 1e-3) / 1e12
        res[f"S_{S}"] = r
        print(f"S = {S}: kernel {r['ms_kernel'][0]:.3f} ms, similar_nodes {r['ms_similar_nodes'][0]:.3f} ms, torch "
              f"matmul + mask + topk {r['ms_torch_matmul_mask_topk'][0]:.3f} ms, rows equal {r['rows_equal_to_torch']:.3f}",
              flush=True)
        del ws, base, got
        torch.cuda.empty_cache()

    src = torch.from_numpy(np.random.default_rng(7).integers(0, n, size=16)).to(dev)
    rec = {"sources": 16, "k": 100, "n_similar": M}
    rec["ms_recommend_similar"] = spread_ms(lambda: lpformer_amd.recommend(model, score, src, 100, candidates="similar",
                                                                           n_similar=M, h=h))
    rec["ms_recommend_all"] = spread_ms(lambda: lpformer_amd.recommend(model, score, src, 100, candidates="all", h=h),
                                        reps=min(REPS, 3))
    a = lpformer_amd.recommend(model, score, src, 100, candidates="similar", n_similar=M, h=h)
    b = lpformer_amd.recommend(model, score, src, 100, candidates="all", h=h)
    rec["pairs_scored_similar"], rec["pairs_scored_all"] = int(a.n_candidates.sum()), int(b.n_candidates.sum())
    rec["top100_of_all_found_among_similar"] = float(torch.stack([torch.isin(y, x).float().mean()
                                                                  for x, y in zip(a.ids, b.ids)]).mean())
    res["recommend_16_sources"] = rec
    print(f"recommend, 16 sources: similar {rec['ms_recommend_similar'][0]:.2f} ms ({rec['pairs_scored_similar']} pairs), "
          f"all {rec['ms_recommend_all'][0]:.2f} ms ({rec['pairs_scored_all']} pairs)", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
