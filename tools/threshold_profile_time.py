"""Device time of threshold_profile (lpf_threshold_profile) on the synthetic collab-like graph, next to what the same
numbers cost without it: one prebuilt LinkTransformer per grid point, each running compute_node_mask plus a device
bincount per type.  32,768 pairs from data.sample_pairs, the default 6-point grid; warm-up first, then REPS calls each
between two HIP events, the median reported (and the spread).  Model construction (the PPR filter and the walk index of
each model, built on its first selection) is timed separately with a host clock around a device synchronise.  The
counts of the two ways are compared, so the figures are for equal results.
    LPF_CFG=collab LPF_REPS=20 LPF_SPLITS="0 128 2048" python tools/threshold_profile_time.py"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import lpformer_amd
from lpformer_amd import data as D, sources
from lpformer_amd.threshold_profile import DEFAULT_GRID, threshold_profile

REPS = int(os.environ.get("LPF_REPS", "20"))
SPLITS = [int(s) for s in os.environ.get("LPF_SPLITS", "0 128 2048").split()]
assert torch.cuda.is_available(), "a measurement needs the MI355X"
dev = torch.device("cuda:0")


def timed(fn, reps=REPS, warm=3):
    """Median, minimum and maximum device milliseconds of `reps` calls, each between two HIP events."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), min(ms), max(ms)


name = os.environ.get("LPF_CFG", "collab")
cfg = D.CONFIGS[name]
n = cfg["n"]
t0 = time.perf_counter()
ei, w = D.chung_lu_graph(n, cfg["edges"], gamma=cfg["gamma"], seed=0, max_weight=cfg["max_weight"])
x = np.random.default_rng(1).standard_normal((n, cfg["f_in"])).astype(np.float32)
data = D.build_data(ei, x, n, edge_weight=w, eps=cfg["eps"], ppr_device=dev)
batch = torch.from_numpy(D.sample_pairs(ei, n, 32_768, seed=7)).to(dev)
P = batch.shape[1]
print(f"# {name}: n {n}, {ei.shape[1]} directed edges, PPR nnz {data['ppr'].nnz}, {P} pairs, "
      f"setup {time.perf_counter() - t0:.1f} s", flush=True)
grid = [float(np.float32(t)) for t in DEFAULT_GRID]


def make_model(th):
    args = dict(D.train_args_for(cfg), thresh_cn=th, thresh_1hop=th, thresh_non1hop=th)
    torch.manual_seed(0)
    return lpformer_amd.LinkTransformer(args, data, device=dev).to(dev).eval()


def model_counts(model):
    sel = model.compute_node_mask(batch)
    return [torch.bincount(s[0][0], minlength=P) for s in sel]


# (b) what the parent commit offers: one model per grid point
models, build_s = [], []
for th in grid:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    try:
        m = make_model(th)
        model_counts(m)                      # the first selection builds the model's PPR filter and walk index
    except Exception as exc:                 # noqa: BLE001 -- a grid point the selection cannot size is reported, not hidden
        print(f"  model at threshold {th:g}: FAILED ({type(exc).__name__}: {exc})", flush=True)
        m = None
    torch.cuda.synchronize()
    build_s.append(time.perf_counter() - t0)
    models.append(m)
    print(f"  model at threshold {th:<8g} construction + first selection {build_s[-1] * 1e3:9.1f} ms", flush=True)

# (a) the profile
source = next(m for m in models if m is not None)
prof = threshold_profile(source, batch, DEFAULT_GRID, per_pair=True)
print(prof.table(), flush=True)
_, adj, ppr = sources.model_graphs(source, False, "threshold_profile_time")
deg = (adj.rowptr[1:] - adj.rowptr[:-1])
plen = (ppr.rowptr[1:] - ppr.rowptr[:-1])
walked = torch.stack([deg[batch[0]], deg[batch[1]], torch.minimum(plen[batch[0]], plen[batch[1]])]).cpu().numpy()
L = walked.sum(axis=0)
print(f"  walked slots per pair: N(a) {walked[0].mean():.1f}, N(b) {walked[1].mean():.1f}, shorter PPR row "
      f"{walked[2].mean():.1f}; total mean {L.mean():.1f}, p99 {np.percentile(L, 99):.0f}, max {L.max()}")

agree = True
for j, m in enumerate(models):
    if m is None:
        agree = False
        continue
    for t, c in enumerate(model_counts(m)):
        same = bool(torch.equal(c.to(torch.int32), prof.per_pair[:, t, j]))
        agree &= same
        if not same:
            print(f"  MISMATCH at threshold {grid[j]:g}, type {t}: model {int(c.sum())}, profile "
                  f"{int(prof.per_pair[:, t, j].sum())}")
print(f"  counts of the six models == profile.per_pair: {agree}", flush=True)

a_ms = timed(lambda: threshold_profile(source, batch, DEFAULT_GRID))
a_pp = timed(lambda: threshold_profile(source, batch, DEFAULT_GRID, per_pair=True))
print(f"(a) threshold_profile, per_pair=False   median {a_ms[0]:9.3f} ms  (min {a_ms[1]:.3f}, max {a_ms[2]:.3f}; "
      f"{REPS} calls)")
print(f"    threshold_profile, per_pair=True    median {a_pp[0]:9.3f} ms  (min {a_pp[1]:.3f}, max {a_pp[2]:.3f})")
for thr in SPLITS:
    ms = timed(lambda: threshold_profile(source, batch, DEFAULT_GRID, split_threshold=thr), reps=max(REPS // 2, 3))
    print(f"    split_threshold {thr:5d}              median {ms[0]:9.3f} ms  ({(L > thr).mean() * 100:.2f} % of pairs on "
          f"the workgroup kernel)", flush=True)
if all(m is not None for m in models):
    b_ms = timed(lambda: [model_counts(m) for m in models])
    print(f"(b) six models: compute_node_mask + bincount   median {b_ms[0]:9.3f} ms  (min {b_ms[1]:.3f}, max "
          f"{b_ms[2]:.3f}); without construction ({sum(build_s):.2f} s for the six)")
    print(f"    ratio (b) / (a) = {b_ms[0] / a_ms[0]:.2f}")
else:
    print("(b) not measured: a model could not be built or run (above)")
