"""Tuning aid: phase marks of tail_chain_kernel (tools/tail_stamps.sh): per wavefront start / stage A read /
stage B k-groups done / LayerNorm B done / stage C r_e k-groups done / r_p k-groups done / end; in the three-launch step
(model.fuse_step, the default at D = 128 fp32) also stage E done, and the r_e k-groups then come BEFORE the rows read.
Stage E splits further: its gathered rows arrived (the stamped build waits for them there) / its k-loop done / its
LayerNorm done (= stage E done).  16 words per wavefront: marks 0-9, word 15 = the kind (0 full workgroup, 1 pairs without
selected nodes)."""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import lpformer_amd
from lpformer_amd import data as D, _lib
name = os.environ.get("LPF_CFG", "collab")
cfg = D.CONFIGS[name]
n = cfg["n"]; dev = torch.device("cuda:0")
ei, w = D.chung_lu_graph(n, cfg["edges"], gamma=cfg["gamma"], seed=0, max_weight=cfg["max_weight"])
x = np.random.default_rng(1).standard_normal((n, cfg["f_in"])).astype(np.float32)
data = D.build_data(ei, x, n, edge_weight=w, eps=cfg["eps"], ppr_device=dev)
torch.manual_seed(0)
model = lpformer_amd.LinkTransformer(D.train_args_for(cfg), data, device=dev).to(dev).eval()
score = lpformer_amd.mlp_score(model.out_dim, model.out_dim, 1, 2).to(dev).eval()
model.use_side_stream = False
batches = [torch.from_numpy(D.sample_pairs(ei, n, cfg["batch"], seed=1000 + i)).to(dev) for i in range(3)]
h = model.propagate()
lib = _lib.hip()
fn = lib.lpf_tail_chain_set_stamps
fn.argtypes = [ctypes.c_void_p]; fn.restype = ctypes.c_int
buf = torch.zeros(2048 * 8 * 16, dtype=torch.int64, device=dev)
for b in batches * 3:
    model.score_pairs(b, h, score)
torch.cuda.synchronize()
assert fn(buf.data_ptr()) == 0
names = ["start", "rows read", "stage B loop", "LN B", "C: r_e loop", "C: r_p loop", "end"]
for i, b in enumerate(batches[:2]):
    buf.zero_()
    model.score_pairs(b, h, score)
    torch.cuda.synchronize()
    v = buf.view(-1, 16).cpu().numpy().astype(np.float64)
    v = v[v[:, 0] > 0]
    t0 = v[:, 0].min()
    ew = bool((v[:, 7] > 0).any())     # stage E form: start, E, C: r_e, rows read, stage B, LN B, C: r_p, end
    order = [0, 8, 9, 7, 4, 1, 2, 3, 5, 6] if ew else list(range(7))
    names = ["start", "rows read", "stage B loop", "LN B", "C: r_e loop", "C: r_p loop", "end", "stage E", "E: rows here",
             "E: k-loop"]
    for kind, tag in ((0, "full workgroups"), (1, "workgroups of pairs without selected nodes")):
        s = v[v[:, 15] == kind]
        if not len(s):
            continue
        rel = (s[:, :10] - t0) / 100.0
        print(f"batch {i}, {tag}: {len(s)} wavefronts; last end {rel[:, 6].max():.1f} us")
        for k in order:
            if kind == 1 and k not in ((0, 8, 9, 7, 4, 6) if ew else (0, 6)):
                continue
            print(f"   {names[k]:14s} p10 {np.percentile(rel[:, k], 10):6.1f}  p50 {np.percentile(rel[:, k], 50):6.1f}  "
                  f"p90 {np.percentile(rel[:, k], 90):6.1f}  max {rel[:, k].max():6.1f}")
        if kind == 0:
            d = np.diff(rel[:, order], axis=1)
            print("   phase lengths, median:", " ".join(f"{names[order[k + 1]]} {np.median(d[:, k]):.1f}"
                                                        for k in range(len(order) - 1)))
