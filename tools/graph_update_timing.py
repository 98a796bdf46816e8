"""update_ppr(device=...) end to end (flag + push + splice) against calc_ppr_gpu on the same edited graph, interleaved in
one process, on bench's synthetic graphs; the flagged fraction; lpf_ppr_affected_rows alone with its roofline line
(4 * nnz bytes over its time against the measured HBM rate); and what update_graph spends outside the PPR refresh.
Writes profiles/graph_update_timing.json (or LPF_OUT).
    LPF_CFGS="collab ppa" LPF_ADDS="1 16 256 4096" LPF_REMOVES="1 16" LPF_REPS=3 python tools/graph_update_timing.py"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import lpformer_amd
from lpformer_amd import data as D
from lpformer_amd import graph, graph_update as U
from lpformer_amd.ppr import calc_ppr_gpu

ADDS = [int(v) for v in os.environ.get("LPF_ADDS", "1 16 256 4096").split()]
REMOVES = [int(v) for v in os.environ.get("LPF_REMOVES", "1 16").split()]
REPS = int(os.environ.get("LPF_REPS", "3"))
MODEL = os.environ.get("LPF_MODEL", "1") == "1"
OUT = os.environ.get("LPF_OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                             "graph_update_timing.json"))
HBM_BYTES_PER_S = 6.29e12     # measured float4 copy rate of the MI355X
dev = torch.device("cuda:0")
ALPHA = 0.15


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def same(a, b):
    return bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and
                torch.equal(a[2].view(torch.int32), b[2].view(torch.int32)))


result = {"alpha": ALPHA, "reps": REPS, "graphs": {}}
for name in os.environ.get("LPF_CFGS", "collab ppa").split():
    cfg = D.CONFIGS[name]
    n, eps = cfg["n"], cfg["eps"]
    ei, w = D.chung_lu_graph(n, cfg["edges"], gamma=cfg["gamma"], seed=0, max_weight=cfg["max_weight"])
    ei = np.asarray(ei, np.int64)
    calc_ppr_gpu(ei, n, ALPHA, eps, device=dev, to_host=False)                     # warm-up (code objects, allocator)
    t_full0, old = wall(lambda: calc_ppr_gpu(ei, n, ALPHA, eps, device=dev, to_host=False))
    nnz = int(old[1].numel())
    print(f"{name}: n={n} directed edges={ei.shape[1]} nnz(PPR)={nnz} full producer {t_full0:.3f} s", flush=True)
    g = {"n": n, "eps": eps, "directed_edges": int(ei.shape[1]), "ppr_nnz": nnz, "full_producer_s": t_full0, "edits": []}
    rng = np.random.default_rng(1)
    edits = [("add", k) for k in ADDS] + [("remove", k) for k in REMOVES]
    for kind, k in edits:
        if kind == "add":
            p = rng.integers(0, n, size=(2, 2 * k + 8))
            add, remove = p[:, p[0] != p[1]][:, :k], None
        else:
            add, remove = None, ei[:, rng.choice(ei.shape[1], k, replace=False)]
        new_keys = U._edit_keys(U._edge_keys(ei, n), U._as_pairs(add, n, "add"), U._as_pairs(remove, n, "remove"), n)[0]
        ei2 = U._keys_to_edge_index(new_keys, n)
        inc_s, full_s, st = [], [], None
        U.update_ppr(old, ei, add=add, remove=remove, alpha=ALPHA, eps=eps, device=dev, full_above=2.0)   # warm-up
        for _ in range(REPS):                                                    # interleaved
            t, (got, st) = wall(lambda: U.update_ppr(old, ei, add=add, remove=remove, alpha=ALPHA, eps=eps,
                                                     device=dev, full_above=2.0))
            inc_s.append(t)
            t, want = wall(lambda: calc_ppr_gpu(ei2, n, ALPHA, eps, device=dev, to_host=False))
            full_s.append(t)
        ok = same(got, want)
        row = {"kind": kind, "k": k, "n_keys": st["n_keys"], "n_affected": st["n_affected"], "fraction": st["fraction"],
               "incremental_s": inc_s, "full_s": full_s, "bit_identical": ok,
               "phases_s": {p: st[p] for p in ("edit_s", "keys_s", "upload_s", "flag_s", "push_s", "splice_s") if p in st}}
        g["edits"].append(row)
        print(f"  {kind} {k}: keys {st['n_keys']} flagged {st['n_affected']} ({st['fraction']:.4f}) incremental "
              f"median {np.median(inc_s):.4f} s min {min(inc_s):.4f} | full median {np.median(full_s):.4f} s min "
              f"{min(full_s):.4f} | bit-identical {ok} | " +
              " ".join(f"{p}={v:.4f}" for p, v in row["phases_s"].items()), flush=True)
        del got, want
    # lpf_ppr_affected_rows alone: both bitmap forms where they exist, HIP events
    old_d = graph.DeviceCSR(old[0], old[1], old[2], n, None)
    mask = np.zeros(n, bool)
    mask[rng.choice(n, 40, replace=False)] = True
    g["affected_rows"] = {}
    for mode in (0, 1):
        if mode == 1 and (n + 31) // 32 * 4 > 64 * 1024:
            continue
        U.affected_rows_device(old_d, mask, mode)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            U.affected_rows_device(old_d, mask, mode)
        e1.record()
        torch.cuda.synchronize()
        s = e0.elapsed_time(e1) / 10 / 1e3
        floor = 4.0 * nnz / HBM_BYTES_PER_S
        g["affected_rows"]["lds" if mode else "global"] = {"s_per_call_incl_upload_and_select": s,
                                                           "floor_s_4nnz_bytes_at_hbm_rate": floor,
                                                           "share_of_floor": floor / s}
        print(f"  lpf_ppr_affected_rows ({'LDS' if mode else 'global'} bitmap, 40 keys; with bitmap upload and select): "
              f"{s * 1e3:.3f} ms per call, floor {floor * 1e3:.3f} ms (4 * nnz bytes at 6.29 TB/s): {floor / s:.2f} of it",
              flush=True)
    del old_d
    if MODEL:      # what update_graph spends outside the PPR refresh
        x = np.random.default_rng(1).standard_normal((n, cfg["f_in"])).astype(np.float32)
        ppr_host = graph.CSR(old[0].cpu().numpy(), old[1].cpu().numpy(), old[2].cpu().numpy(), n)
        data = D.build_data(ei, x, n, edge_weight=w, eps=eps, ppr=ppr_host)
        torch.manual_seed(0)
        model = lpformer_amd.LinkTransformer(D.train_args_for(cfg), data, device=dev).to(dev).eval()
        model.propagate()
        p = rng.integers(0, n, size=(2, 20))
        t, st = wall(lambda: lpformer_amd.update_graph(model, add=p[:, p[0] != p[1]][:, :16], alpha=ALPHA, eps=eps))
        keep = {k: st[k] for k in ("data_s", "upload_s", "walk_index_s", "gcn_norm_s", "encoder_s") if k in st}
        keep["ppr_total_s"] = st["ppr"]["total_s"]
        keep["wall_s"] = t
        g["update_graph_16_added"] = keep
        print("  update_graph (16 added edges): " + " ".join(f"{k}={v:.4f}" for k, v in keep.items()), flush=True)
        del model, data, ppr_host
    del old
    torch.cuda.empty_cache()
    result["graphs"][name] = g
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)
print(f"wrote {OUT}")
