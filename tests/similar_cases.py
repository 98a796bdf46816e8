"""Shared builders of the similar_nodes tests (host and MI355X): the exact integer cases, a plain Python restatement of
the ranking, the fixture model, and the fp64 side of the real-valued checks."""
import numpy as np

from lpformer_amd import graph
from lpformer_amd.similar import order_key

N_VALUES = (1, 15, 16, 17, 1000, 3001)
S_VALUES = (1, 17, 33)
D_VALUES = (1, 3, 36, 64, 128, 257)
M_VALUES = (1, 7, 64, 256)
EXCLUSIONS = ("none", "self", "csr", "hub")      # src_ids NULL / src_ids alone / a random CSR / a CSR with one hub row
N_RANGES = (1, 2, 7, -1)


def pad4(k):
    return (k + 3) & ~3


def padded(a, extra=4):
    """``a`` [R, D] as a view of an [R, pad4(D) + extra] buffer whose other columns hold NaN: ld > D, rows 16-byte aligned."""
    a = np.asarray(a, np.float32)
    buf = np.full((a.shape[0], pad4(a.shape[1]) + extra), np.nan, np.float32)
    buf[:, :a.shape[1]] = a
    return buf


def random_csr(n, rng, deg=5):
    """A sorted, duplicate-free exclusion CSR with about ``deg`` entries per row."""
    rows = [np.unique(rng.integers(0, n, size=rng.integers(0, 2 * deg + 1))) for _ in range(n)]
    rowptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    col = (np.concatenate(rows) if n else np.zeros(0)).astype(np.int32)
    return rowptr, col


def hub_csr(n, rng, hub):
    """``random_csr`` with row ``hub`` adjacent to all but 3 nodes (all but min(3, n))."""
    rowptr, col = random_csr(n, rng)
    rows = [col[rowptr[i]:rowptr[i + 1]] for i in range(n)]
    keep = rng.choice(n, size=min(3, n), replace=False)
    rows[hub] = np.setdiff1d(np.arange(n), keep).astype(np.int32)
    rowptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    return rowptr, np.concatenate(rows).astype(np.int32)


def _sources(n, S, rng, first=None):
    """S node ids with duplicates and, from S = 17 on, one id outside [0, n)."""
    src = rng.integers(0, n, size=S).astype(np.int64)
    if S >= 3:
        src[2] = src[1]
    if S >= 17:
        src[5] = n + 3 if S == 17 else -1
    if first is not None:
        src[0] = first
    return src


def make_case(n, S, D, m, exclusion="csr", exclude_self=True, metric="dot", kind="random", seed=0):
    """One exact case: every dot product is an integer (or a special value by construction) in any summation order.

    kind: "random" -- table entries in {-2 .. 2}, queries gathered from the table (free integer vectors without
    src_ids): most nodes tie with another; "increasing" / "decreasing" -- score(s, v) = +-v for every source, so every
    tile beats the threshold / nothing does after the first m; "special" -- scores among +-inf, NaN, +-0.0 and small
    integers.  metric "cosine": power-of-two scales (negative ones too for "special": -0.0 products), so the two
    multiplies are exact."""
    rng = np.random.default_rng([seed, n, S, D, m])
    if kind == "random":
        T = rng.integers(-2, 3, size=(n, D)).astype(np.float32)
    else:
        T = np.zeros((n, D), np.float32)
        if kind == "increasing":
            T[:, 0] = np.arange(n)
        elif kind == "decreasing":
            T[:, 0] = -np.arange(n, dtype=np.float32)
        else:
            pool = np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, 1.0, -1.0, 2.0, 3.0, -np.nan], np.float32)
            T[:, 0] = pool[rng.integers(0, pool.size, size=n)]
    hub = int(rng.integers(0, n))
    src = None if exclusion == "none" else _sources(n, S, rng, hub if exclusion == "hub" else None)
    if kind == "random":
        Q = rng.integers(-2, 3, size=(S, D)).astype(np.float32) if src is None else T[np.clip(src, 0, n - 1)].copy()
    else:
        Q = np.zeros((S, D), np.float32)
        Q[:, 0] = 1.0
    exc = None
    if exclusion == "csr":
        exc = random_csr(n, rng)
    elif exclusion == "hub":
        exc = hub_csr(n, rng, hub)
    qs = ts = None
    if metric == "cosine":
        qs = np.exp2(rng.integers(-3, 4, size=S)).astype(np.float32)
        ts = np.exp2(rng.integers(-3, 4, size=n)).astype(np.float32)
        if kind == "special":
            qs[::2] *= -1
            ts[::3] *= -1
    return {"n": n, "S": S, "D": D, "m": m, "Q": Q, "T": T, "q_scale": qs, "t_scale": ts, "src_ids": src, "exclude": exc,
            "exclude_self": bool(exclude_self), "id": f"{kind}-n{n}-S{S}-D{D}-m{m}-{exclusion}-{metric}-"
                                                        f"self{int(bool(exclude_self))}"}


def exact_specs():
    """About 50 specs out of the cross-product: every value of N_VALUES, S_VALUES, D_VALUES, M_VALUES, EXCLUSIONS, both
    metrics, exclude_self on and off, the two adversarial orders and the special values occur."""
    specs = []
    for i, n in enumerate(N_VALUES):
        for j, D in enumerate(D_VALUES):
            specs.append(dict(n=n, S=S_VALUES[(i + j) % 3], D=D, m=M_VALUES[(i + 2 * j + j // 2) % 4],
                              exclusion=EXCLUSIONS[(i + 3 * j) % 4], exclude_self=(i + j) % 2 == 0,
                              metric=("dot", "cosine")[(i + j // 2) % 2]))
    for n, m, D, S in ((3001, 64, 1, 17), (3001, 256, 36, 33), (3001, 7, 3, 1), (1000, 1, 64, 17)):
        for kind in ("increasing", "decreasing"):
            specs.append(dict(n=n, S=S, D=D, m=m, exclusion="csr", kind=kind))
    for n, m, metric in ((1000, 256, "dot"), (1000, 64, "cosine"), (17, 64, "cosine"), (3001, 7, "dot")):
        specs.append(dict(n=n, S=17, D=3, m=m, exclusion="self", metric=metric, kind="special"))
    for n, m in ((3001, 64), (1000, 256), (17, 7)):        # the hub source has 3 eligible nodes or fewer: count < m
        specs.append(dict(n=n, S=17, D=36, m=m, exclusion="hub", metric="cosine"))
    return specs


def loop_reference(case):
    """The documented result by a plain Python loop: per source the full sort of (score key, ~id) over the eligible
    nodes.  Scores: the exact sum in Python floats (fp64), rounded to fp32, then the two fp32 multiplies."""
    n, S, m = case["n"], case["S"], case["m"]
    Q, T = case["Q"], case["T"]
    ids = np.full((S, m), -1, np.int64)
    out = np.full((S, m), -np.inf, np.float32)
    counts = np.zeros(S, np.int64)
    for s in range(S):
        u = None if case["src_ids"] is None else int(case["src_ids"][s])
        if u is not None and not 0 <= u < n:
            continue
        banned = set()
        if u is not None:
            if case["exclude"] is not None:
                rowptr, col = case["exclude"]
                banned.update(int(c) for c in col[rowptr[u]:rowptr[u + 1]])
            if case["exclude_self"]:
                banned.add(u)
        entries = []
        integer = bool(np.isfinite(T).all() and np.isfinite(Q[s]).all())
        if integer:      # integer entries: the dot products exactly, in int64
            exact = (T.astype(np.int64) * Q[s].astype(np.int64)[None, :]).sum(1)
        for v in range(n):
            if v in banned:
                continue
            with np.errstate(all="ignore"):
                if integer:
                    acc = float(exact[v])
                else:
                    acc = 0.0
                    for k in range(Q.shape[1]):
                        acc += float(Q[s, k]) * float(T[v, k])
                sc = np.float32(acc)
                if case["q_scale"] is not None:
                    sc = np.float32(np.float32(sc * case["q_scale"][s]) * case["t_scale"][v])
            entries.append((int(order_key(sc)), -v, sc))
        entries.sort(reverse=True)
        for e, (key, neg_v, sc) in enumerate(entries[:m]):
            ids[s, e] = -neg_v
            out[s, e] = np.float32(np.nan) if np.isnan(sc) else (np.float32(0.0) if sc == 0 else sc)
        counts[s] = min(m, len(entries))
    return ids, out, counts


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


# ------------------------------------------------------------------------------------------- real-valued checks
U = 2.0 ** -24


def dot_bound(Q, T, D, q_scale=None, t_scale=None):
    """(fp64 scores [S, n], B [S, n]): B(s, v) = gamma sum_k |Q[s][k] T[v][k]| with gamma = (D + 2) u / (1 - (D + 2) u),
    the standard fp32 dot-product bound (D products and additions, two more roundings for the scales)."""
    Qd, Td = np.asarray(Q, np.float64), np.asarray(T, np.float64)
    gamma = (D + 2) * U / (1.0 - (D + 2) * U)
    score, mag = Qd @ Td.T, np.abs(Qd) @ np.abs(Td).T
    if q_scale is not None:
        w = np.asarray(q_scale, np.float64)[:, None] * np.asarray(t_scale, np.float64)[None, :]
        score, mag = score * w, mag * np.abs(w)
    return score, gamma * mag


def check_real(ids, scores, counts, score64, B, eligible, m):
    """(a) returned scores within B of the fp64 scores; (b) rows sorted by the documented key of their own scores, ids
    distinct and eligible, counts = min(m, eligible); (c) no eligible node left out whose fp64 score exceeds the
    smallest returned one by more than 2 max_v B(s, v).  Returns (largest |error| / B, largest slack used / allowed)."""
    worst_a = worst_c = 0.0
    for s in range(ids.shape[0]):
        c = int(counts[s])
        assert c == min(m, int(eligible[s].sum())), (s, c)
        got, sc = ids[s, :c], scores[s, :c]
        assert (ids[s, c:] == -1).all() and np.isneginf(scores[s, c:]).all(), s
        assert np.unique(got).size == c and eligible[s][got].all(), s
        err = np.abs(sc.astype(np.float64) - score64[s, got])
        assert (err <= B[s, got]).all(), (s, float((err / B[s, got]).max()))
        worst_a = max(worst_a, float((err / np.maximum(B[s, got], 1e-300)).max()) if c else 0.0)
        key = (order_key(sc).astype(np.uint64) << np.uint64(32)) | (~got.astype(np.uint32)).astype(np.uint64)
        assert (key[:-1] > key[1:]).all(), s
        rest = eligible[s].copy()
        rest[got] = False
        if c and rest.any():
            allowed = 2.0 * float(B[s][eligible[s]].max())
            over = float(score64[s][rest].max() - score64[s, got].min())
            assert over <= allowed, (s, over, allowed)
            worst_c = max(worst_c, over / allowed)
    return worst_a, worst_c


def eligible_mask(n, src, exclude, exclude_self):
    """bool [S, n]: the nodes each source may return (``exclude``: (rowptr, col) or None)."""
    ok = np.ones((len(src), n), bool)
    for s, u in enumerate(src):
        if not 0 <= u < n:
            ok[s] = False
            continue
        if exclude is not None:
            ok[s, exclude[1][exclude[0][u]:exclude[0][u + 1]]] = False
        if exclude_self:
            ok[s, u] = False
    return ok


# ---------------------------------------------------------------------------------------------------- fixture model
def build_model(fx, dev):
    """Model + score head on ``dev`` from a golden fixture, graph entries as torch sparse COO tensors (restated from
    tests/test_gpu_recommend.py)."""
    import torch

    import lpformer_amd
    n = fx.n
    data = {"x": torch.from_numpy(fx["x"]).to(dev), "num_nodes": n}

    def pack(ei_key, w_key, ppr_prefix):
        ei = fx[ei_key].astype(np.int64)
        adj_t = graph.csr_from_coo(ei[0], ei[1], fx[w_key], n)
        mask = graph.mask_csr(ei, n, symmetric=True)
        ppr = graph.csr_from_coo(fx[ppr_prefix + "row"], fx[ppr_prefix + "col"], fx[ppr_prefix + "val"], n)
        return adj_t.to_torch_sparse_coo().to(dev), mask.to_torch_sparse_coo().to(dev).int(), \
            ppr.to_torch_sparse_coo().to(dev)

    data["adj_t"], data["adj_mask"], data["ppr"] = pack("edge_index", "edge_weight", "ppr_")
    if fx.test_set:
        data["full_adj_t"], data["full_adj_mask"], data["ppr_test"] = pack("full_edge_index", "full_edge_weight",
                                                                            "ppr_test_")
    else:
        data["full_adj_t"], data["full_adj_mask"], data["ppr_test"] = data["adj_t"], data["adj_mask"], data["ppr"]
    cfg = {k: fx.cfg[k] for k in ("thresh_cn", "thresh_1hop", "thresh_non1hop", "dim", "trans_layers", "num_heads",
                                  "att_drop", "dropout", "gnn_drop", "feat_drop", "gcn_cache", "gnn_layers",
                                  "residual", "layer_norm", "relu")}
    model = lpformer_amd.LinkTransformer(cfg, data, device=dev).to(dev)
    score = lpformer_amd.mlp_score(model.out_dim, model.out_dim, 1, fx.cfg["pred_layers"]).to(dev)
    m_sd, s_sd = fx.state_dicts()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in m_sd.items()}, strict=True)
    score.load_state_dict({k: torch.from_numpy(v) for k, v in s_sd.items()}, strict=True)
    return model.eval(), score.eval()


def np_topk(seg_ptr, score, cand, k):
    """``lpf_segment_topk_f32`` in numpy (restated from tests/test_gpu_recommend.py): key descending, then position."""
    S = len(seg_ptr) - 1
    ids = np.full((S, k), -1, np.int64)
    out = np.full((S, k), -np.inf, np.float32)
    cnt = np.zeros(S, np.int64)
    key = order_key(score)
    for s in range(S):
        lo, hi = seg_ptr[s], seg_ptr[s + 1]
        order = np.lexsort((np.arange(hi - lo), -key[lo:hi].astype(np.int64)))[:k]
        c = order.size
        ids[s, :c], out[s, :c], cnt[s] = cand[lo:hi][order], score[lo:hi][order], c
    return ids, out, cnt
