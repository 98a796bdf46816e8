"""Timing aid: ms per training step of three ways to mask a batch's positives out of the typing adjacency, on the
collab-like config, interleaved in ONE process (same model shapes, same graph, same box): five 10-step windows per path,
taken round-robin, the median of each reported with the windows (tools/train_time.py's protocol).

  tensor    the reference-shaped loop: a coalesced sparse COO tensor of every kept training edge per batch
            (src/train/train_model.py:40-45)                                -- exact, whatever train_pos repeats
  removed   adj_mask=lpformer_amd.RemovedEdges(edges)                        -- exact only when every row is a unique pair
  epoch     lpformer_amd.train_epoch (TrainEdges.mask: lpf_batch_cover)      -- exact; loss read once per window

LPF_TRAIN_BS positives + as many negatives per step; LPF_EPOCH_DUP: share of extra duplicate rows appended to train_pos
(half of them reversed; 0 = every row unique, the setting of profiles/r06_train_modes_final.txt).  Writes JSON to the path
in LPF_EPOCH_OUT when set."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import lpformer_amd
from lpformer_amd import data as D

cfg = D.CONFIGS[os.environ.get("LPF_CFG", "collab")]
n = cfg["n"]; dev = torch.device("cuda:0"); bs = int(os.environ.get("LPF_TRAIN_BS", "8192"))
dup = float(os.environ.get("LPF_EPOCH_DUP", "0"))
ei, w = D.chung_lu_graph(n, cfg["edges"], gamma=cfg["gamma"], seed=0, max_weight=cfg["max_weight"])
x = np.random.default_rng(1).standard_normal((n, cfg["f_in"])).astype(np.float32)
data = D.build_data(ei, x, n, edge_weight=w, eps=cfg["eps"], ppr_device=dev)
targs = dict(D.train_args_for(cfg), att_drop=0.1, dropout=0.1, gnn_drop=0.1, feat_drop=0.1)
rows = ei[:, ei[0] < ei[1]].T
if dup > 0:
    rng = np.random.default_rng(2)
    extra = rows[rng.choice(rows.shape[0], int(dup * rows.shape[0]), replace=False)].copy()
    extra[: extra.shape[0] // 2] = extra[: extra.shape[0] // 2, ::-1]
    rows = np.concatenate([rows, extra])
train_pos = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
data["train_pos"] = train_pos
E = train_pos.shape[0]
K, WINDOWS = 10, 5
assert E >= K * bs, "train_pos is too short for a window of distinct batches"


def make():
    torch.manual_seed(0)
    model = lpformer_amd.LinkTransformer(targs, data, device=dev).to(dev)
    score = lpformer_amd.mlp_score(model.out_dim, model.out_dim, 1, 2, 0.1).to(dev)
    opt = torch.optim.Adam(list(model.parameters()) + list(score.parameters()), lr=1e-3)
    return model, score, opt


def hand_loop(kind):
    model, score, opt = make()

    def window(batches):
        model.train(); score.train()
        for perm in batches:
            edges = train_pos[perm].t()
            if kind == "tensor":
                keep = torch.ones(E, dtype=torch.bool, device=dev); keep[perm] = False
                k = train_pos[keep].t()
                r, c = torch.cat([k[0], k[1]]), torch.cat([k[1], k[0]])
                mask = torch.sparse_coo_tensor(torch.stack([r, c]), torch.ones(r.numel(), dtype=torch.int32, device=dev),
                                               (n, n)).coalesce()
            else:
                mask = lpformer_amd.RemovedEdges(edges)
            pos_loss = -torch.log(score(model(edges, adj_mask=mask)) + 1e-6).mean()
            neg = torch.randint(0, n, (2, perm.numel()), device=dev)
            loss = pos_loss - torch.log(1 - score(model(neg)) + 1e-6).mean()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
            torch.nn.utils.clip_grad_norm_(score.parameters(), 1.0)
            opt.step(); opt.zero_grad()
        return float(loss.detach())
    return window


def epoch_loop():
    model, score, opt = make()
    te = lpformer_amd.TrainEdges(train_pos, n, device=dev)
    return lambda batches: lpformer_amd.train_epoch(model, score, data, opt, batches=batches, train_edges=te)


paths = {"tensor": hand_loop("tensor"), "removed": hand_loop("removed"), "epoch": epoch_loop()}
gen = torch.Generator(device=dev).manual_seed(7)


def batches_of_window():
    order = torch.randperm(E, device=dev, generator=gen)
    return [order[i * bs:(i + 1) * bs] for i in range(K)]


for run in paths.values():                      # warm-up: workspaces sized, Adam state made
    run(batches_of_window()[:3])
torch.cuda.synchronize()
wins = {k: [] for k in paths}
last = {}
for _ in range(WINDOWS):
    for name, run in paths.items():             # round-robin: a drift of the box hits the three alike
        b = batches_of_window()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last[name] = run(b)
        torch.cuda.synchronize()
        wins[name].append((time.perf_counter() - t0) / K * 1e3)
res = {"config": os.environ.get("LPF_CFG", "collab"), "batch": bs, "rows": int(E), "duplicate_share": dup, "ms_per_step": {},
       "windows_ms": wins}
for name, ws in wins.items():
    med = sorted(ws)[len(ws) // 2]
    res["ms_per_step"][name] = round(med, 3)
    print(f"{name:8s} {med:6.2f} ms / step ({bs} positives + {bs} negatives)  windows {' '.join(f'{v:.2f}' for v in ws)}"
          f"  spread {max(ws) - min(ws):.2f}  loss {last[name]:.4f}")
res["spread_ms"] = {k: round(max(v) - min(v), 3) for k, v in wins.items()}
print(json.dumps(res))
if os.environ.get("LPF_EPOCH_OUT"):
    with open(os.environ["LPF_EPOCH_OUT"], "w") as f:
        json.dump(res, f, indent=1)
