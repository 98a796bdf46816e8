"""Time lpformer_amd.explain against the call it grew out of, on one GPU:

    python tools/explain_time.py [--rounds 7] [--configs collab ppa] [--out profiles/explain_timing.json]

Per config (the collab-like and ppa-like synthetic graphs of lpformer_amd.data.CONFIGS, one 32,768-pair batch):

* ``explain(top=8)``, ``explain(weights="all")`` and ``calc_pairwise(..., return_weights=True)`` -- the yardstick: the
  same selection + score launches, then the softmax-gather, the output projection and ``pairwise_lin`` instead of the
  explain launch -- alternating in one process, HIP events around each call (host work and ``_select``'s status
  read-back included), median of the rounds after two warm-up rounds;
* ``lpf_pair_explain_f32`` alone (top = 8 and 32, with and without the pair-major list) on the batch's exported selection
  and scores, against its byte floor: entries x (4 B score + 4 B node + 8 B pa/pb) + 24 B of segment pointers per pair
  + the outputs, at the 8 TB/s DESIGN prices HBM at.

Every config runs in a child process of its own under a time limit; the first one that fails ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEP_LIMIT = 540      # seconds per config (graph and PPR set-up included)
HBM_GBPS = 8000.0


def _timed(fn, dev):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _interleave(sides, rounds, dev):
    times = {k: [] for k in sides}
    for r in range(rounds + 2):
        for k, fn in sides.items():
            t = _timed(fn, dev)
            if r >= 2:
                times[k].append(t)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "rounds": len(v)}
            for k, v in times.items()}


def step(name, rounds):
    import importlib
    import numpy as np
    import torch
    import lpformer_amd
    from lpformer_amd import data as D
    X = importlib.import_module("lpformer_amd.explain")
    dev = torch.device("cuda:0")
    cfg = D.CONFIGS[name]
    n, bs = cfg["n"], 32768
    ei, w = D.chung_lu_graph(n, cfg["edges"], gamma=cfg["gamma"], seed=0, max_weight=cfg["max_weight"])
    x = np.random.default_rng(1).standard_normal((n, cfg["f_in"])).astype(np.float32)
    data = D.build_data(ei, x, n, edge_weight=w, eps=cfg["eps"], ppr_device=dev)
    torch.manual_seed(0)
    model = lpformer_amd.LinkTransformer(D.train_args_for(cfg), data, device=dev).to(dev).eval()
    batch = torch.from_numpy(D.sample_pairs(ei, n, bs, seed=3)).to(dev)
    h = model.propagate()
    res = _interleave({"explain_top8": lambda: lpformer_amd.explain(model, batch, top=8, h=h),
                       "explain_all": lambda: lpformer_amd.explain(model, batch, top=8, weights="all", h=h),
                       "calc_pairwise_return_weights": lambda: model.calc_pairwise(batch, h, return_weights=True)},
                      rounds, dev)
    # the kernel alone, on copies of the batch's exported selection and scores
    with torch.no_grad(), torch.cuda.device(dev):
        s, score, _, _ = model._pair_scores(model._prep_batch(batch), h, False, None)
        tp = s["type_ptr"][:3 * (bs + 1)].view(3, bs + 1).clone()
        nnz = int(tp[:, bs].sum())
        node, pa, pb, sc = (t[:max(nnz, 1)].clone() for t in (s["sel_node"], s["sel_pa"], s["sel_pb"], score))
    lens = (tp[:, 1:] - tp[:, :-1]).sum(dim=0)
    kern = {}
    for top in (8, 32):
        for want_all in (False, True):
            r = _interleave({"k": lambda: X._reduce_device(tp, node, pa, pb, sc, top, want_all, nnz)}, rounds, dev)["k"]
            nbytes = nnz * 16 + 24 * (bs + 1) + bs * (top * 21 + 16) + (nnz * 13 + 8 * (bs + 1) if want_all else 0)
            floor_ms = nbytes / (HBM_GBPS * 1e9) * 1e3
            kern[f"top{top}" + ("_all" if want_all else "")] = {**r, "floor_bytes": nbytes, "floor_ms": floor_ms,
                                                                "fraction_of_floor": floor_ms / r["median_ms"]}
    return {"n": n, "pairs": bs, "dim": cfg["dim"], "entries": nnz, "entries_per_pair_mean": nnz / bs,
            "entries_per_pair_max": int(lens.max()), "pairs_above_1024_entries": int((lens > 1024).sum()),
            "calls": res, "kernel": kern}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--configs", nargs="+", default=["collab", "ppa"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explain_timing.json"))
    ap.add_argument("--step")
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("at least 5 rounds")
    if args.step:     # child: one config, its result as one JSON line
        print("RESULT " + json.dumps(step(args.step, args.rounds)))
        return
    import torch
    result = {"device": None, "rounds": args.rounds, "hbm_gbps_assumed": HBM_GBPS, "torch": torch.__version__}
    for name in args.configs:
        try:
            cp = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--rounds", str(args.rounds)],
                                capture_output=True, text=True, timeout=STEP_LIMIT)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"{name}: no result within {STEP_LIMIT} s; stopping")
        if cp.returncode != 0:
            sys.stderr.write(cp.stdout[-2000:] + cp.stderr[-4000:])
            raise SystemExit(f"{name} failed with exit status {cp.returncode}; stopping")
        line = [ln for ln in cp.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        result[name] = json.loads(line[len("RESULT "):])
        print(f"{name}: {json.dumps(result[name])}", flush=True)
    from lpformer_amd import _lib
    result["device"] = _lib.device_info()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
